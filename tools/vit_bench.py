#!/usr/bin/env python3
"""Cost of the native frozen ViT backbone (mmfusion.vit.NativeViT, ViT-base/16 at 224 x 224) on one batch of frames
(default 480 = 16 samples x 30 frames, what the reference pushes through its backbone per step):

  * ms per batch, frames/s and TFLOP/s (35.1 GFLOP per frame by operation count: 12 layers x 197 tokens x 12 x 768^2 MACs of
    linears, 0.72 GMAC attention, 0.12 GMAC patch embedding) of ``cls_features`` and of ``forward``, per chunk size;
  * the yardstick: tests/vit_ref.py run in bf16 through stock torch (rocBLAS + torch's attention) on the same inputs with
    the same timing loop;
  * with --table, a per-kernel table of one ``cls_features`` batch from HIP events around every launch (mmfusion.lib.PROFILE):
    time, share, and for the streaming kernels the HBM rate their byte counts give.

    python tools/vit_bench.py [--frames 480] [--chunks 32,96,160,480] [--steps 10] [--warmup 3] [--table] [--no-torch]
Prints one JSON line (the table, when asked for, on the lines before it)."""
import json

from backbone_bench import kernel_table, parser, print_table, sweep, time_eager  # (first: it sets the import path)
import torch

GFLOP_PER_FRAME = 35.1


def _rate(ms: float, frames: int) -> dict:
    return {"ms": round(ms, 3), "frames_per_s": round(frames / ms * 1e3, 1), "tflops": round(GFLOP_PER_FRAME * frames / ms, 1)}


def _bytes(label: str, detail) -> float:
    """HBM bytes a streaming launch has to move (reads + writes), from the shapes its wrapper recorded"""
    if label not in ("bias_gelu_kernel", "vit_patchify_kernel", "vit_embed_tokens_kernel", "ln_fwd_kernel"):
        return 0.0
    a, b = detail[0]
    if label == "bias_gelu_kernel":
        return a * b * 4 + b * 4
    if label == "vit_patchify_kernel":
        return a * b * 6
    if label == "vit_embed_tokens_kernel":
        return a * b * 4 + b * 4
    if label == "ln_fwd_kernel":
        return a * b * 4 + a * 8
    return 0.0


def main():
    ap = parser(steps=10, warmup=3, torch_yardstick=True)
    ap.add_argument("--frames", type=int, default=480)
    args = ap.parse_args()
    import vit_ref
    from mmfusion import vit
    cfg = vit_ref.base_config()
    sd = vit_ref.seeded_weights(cfg, seed=0)
    model = vit.NativeViT(**vit_ref.config_kwargs(cfg))
    model.load_state_dict(sd)
    model = model.cuda().eval()
    N = args.frames
    x = torch.rand(N, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(1)).cuda()
    res = {"model": "ViT-base/16-224, frozen, bf16 storage", "frames": N, "gflop_per_frame": GFLOP_PER_FRAME,
           "default_chunk": vit.DEFAULT_CHUNK, "workspace_mb_per_image": round(model.workspace_bytes_per_image() / 2 ** 20, 2)}

    def measure(c):
        res[f"cls_features_chunk{c}"] = _rate(time_eager(lambda: model.cls_features(x), args.steps, args.warmup), N)
        res[f"forward_chunk{c}"] = _rate(time_eager(lambda: model(x), args.steps, args.warmup), N)
    sweep(model, vit.DEFAULT_CHUNK, args.chunks, measure)
    if args.table:
        res["kernels"] = kernel_table(lambda: model.cls_features(x), bytes_of=_bytes)
        print_table(res["kernels"])
    if not args.no_torch:
        # the yardstick: the restatement itself in bf16 through stock torch, in chunks of the same size (the same memory bound)
        sd16 = {k: v.cuda().to(torch.bfloat16) for k, v in sd.items()}
        x16 = x.to(torch.bfloat16)
        c = vit.DEFAULT_CHUNK

        def stock(cls_only):
            with torch.no_grad():
                return torch.cat([vit_ref.vit_forward(sd16, x16[i:i + c], cfg, dtype=torch.bfloat16, cls_last_only=cls_only, sdpa=True)
                                  for i in range(0, N, c)]).float()
        res["torch_bf16_cls"] = _rate(time_eager(lambda: stock(True), args.steps, args.warmup), N)
        res["torch_bf16_forward"] = _rate(time_eager(lambda: stock(False), args.steps, args.warmup), N)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
