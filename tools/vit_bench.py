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

With --finetune K [--embeddings] it measures fine-tuning instead (``set_trainable_layers(K)``; --embeddings with K = 12), on the
``cls_features`` route at the default chunk: the inference call, the differentiable forward and forward + backward (ms and their
ratio to the inference call), the saved inputs in MB, the per-kernel table of one forward + backward, and the yardstick: the
same restatement in bf16 through stock torch autograd (``sdpa=True``, ``cls_last_only=True``, the top-K leaves requiring a
gradient, the same chunks).

    python tools/vit_bench.py --finetune 1 [--embeddings] [--frames 480] [--steps 5] [--warmup 2] [--no-torch]
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


def _bytes_bwd(label: str, detail) -> float:
    """``_bytes`` and the streaming launches of the backward"""
    if label not in ("ln_bwd_kernel", "bias_gelu_bwd_kernel", "sum_slabs_kernel", "vit_embed_tokens_bwd_kernel", "vit_cls_attn_bwd_kernel"):
        return _bytes(label, detail)
    a, b = detail[0]
    if label == "ln_bwd_kernel":                       # x, dy, dx and, where it is folded in, the residual: counted as 4 passes
        return a * b * 8
    if label == "bias_gelu_bwd_kernel":
        return a * b * 6
    if label == "sum_slabs_kernel":
        return (a + 1) * b * 4
    return a * b * 4                                   # vit_embed_tokens_bwd_kernel; vit_cls_attn_bwd_kernel: k | v in, dk | dv out


def finetune(args, model, cfg, sd, x) -> dict:
    import vit_ref
    from mmfusion import arena, vit
    N, k, L, d = args.frames, args.finetune, cfg.num_hidden_layers, cfg.hidden_size
    res = {"model": "ViT-base/16-224, bf16 storage", "frames": N, "chunk": model.chunk, "trainable_layers": k, "embeddings": args.embeddings}
    with torch.no_grad():
        res["cls_features_ms"] = round(time_eager(lambda: model.cls_features(x), args.steps, args.warmup), 3)
    model.set_trainable_layers(k, embeddings=args.embeddings)
    arena.ensure(model).zero_grad()
    dout = torch.randn(N, d, generator=torch.Generator().manual_seed(2)).cuda()

    def step():
        model.cls_features(x).backward(dout)
    fwd = time_eager(lambda: model.cls_features(x), args.steps, args.warmup)
    both = time_eager(step, args.steps, args.warmup)
    res["differentiable_forward_ms"], res["differentiable_forward_ratio"] = round(fwd, 3), round(fwd / res["cls_features_ms"], 3)
    res["forward_backward_ms"], res["forward_backward_ratio"] = round(both, 3), round(both / res["cls_features_ms"], 3)
    res["saved_inputs_mb"] = round((k * N * model.T + N) * d * 2 / 2 ** 20, 1)
    res["grad_workspace_mb_per_image"] = round(model.grad_workspace_bytes_per_image() / 2 ** 20, 2)
    res["kernels"] = kernel_table(step, bytes_of=_bytes_bwd)
    print_table(res["kernels"])
    if not args.no_torch:
        keys = {n for n in sd if any(n.startswith(f"layers.{i}.") for i in range(L - k, L)) or n.startswith("layernorm.")
                or (args.embeddings and n.startswith("embeddings."))}
        leaves = {n: v.cuda().to(torch.bfloat16).requires_grad_(n in keys) for n, v in sd.items()}
        x16, d16, c = x.to(torch.bfloat16), dout.to(torch.bfloat16), vit.DEFAULT_CHUNK

        def stock(backward):
            for i in range(0, N, c):
                out = vit_ref.vit_forward(leaves, x16[i:i + c], cfg, dtype=torch.bfloat16, cls_last_only=True, sdpa=True)
                if backward:
                    out.backward(d16[i:i + c])
        res["torch_bf16_forward_ms"] = round(time_eager(lambda: stock(False), args.steps, args.warmup), 3)
        res["torch_bf16_forward_backward_ms"] = round(time_eager(lambda: stock(True), args.steps, args.warmup), 3)
        res["speedup_forward_backward"] = round(res["torch_bf16_forward_backward_ms"] / both, 3)
    return res


def main():
    ap = parser(steps=10, warmup=3, torch_yardstick=True)
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--finetune", type=int, default=0, metavar="K")
    ap.add_argument("--embeddings", action="store_true")
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
    if args.finetune:
        print(json.dumps(finetune(args, model, cfg, sd, x)))
        return
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
