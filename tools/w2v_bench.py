#!/usr/bin/env python3
"""Cost of the native frozen Wav2Vec2 backbone (mmfusion.wav2vec2.NativeWav2Vec2, wav2vec2-base) on one batch of clips
(default 16 clips of 160000 samples = 10 s, what the reference pushes through its backbone per step):

  * ms per batch, clips/s and TFLOP/s (by operation count, printed as gflop_per_clip: feature-extractor convolutions,
    positional convolution, 12 layers at T = 499) of ``forward``, per chunk size;
  * the yardstick: tests/w2v_ref.py run in bf16 through stock torch (rocBLAS + torch's attention) on the same inputs with the
    same timing loop and the same chunking;
  * with --table, a per-kernel table of one batch from HIP events around every launch (mmfusion.lib.PROFILE): time, share,
    TFLOP/s where the wrapper counts operations.

    python tools/w2v_bench.py [--clips 16] [--samples 160000] [--chunks 4,8,16] [--steps 5] [--warmup 2] [--table] [--no-torch]
Prints one JSON line (the table, when asked for, on the lines before it)."""
import json

from backbone_bench import kernel_table, parser, print_table, sweep, time_eager  # (first: it sets the import path)
import torch


def gflop_per_clip(cfg, L: int) -> dict:
    from mmfusion.wav2vec2 import feat_lengths
    Ts = feat_lengths(L, cfg.conv_kernel, cfg.conv_stride)
    dims, ks, d, I, T = cfg.conv_dim, cfg.conv_kernel, cfg.hidden_size, cfg.intermediate_size, Ts[-1]
    conv = 2.0 * Ts[0] * dims[0] * ks[0] + sum(2.0 * Ts[i] * dims[i] * dims[i - 1] * ks[i] for i in range(1, len(dims)))
    pos = 2.0 * T * d * (d // cfg.num_conv_pos_embedding_groups) * cfg.num_conv_pos_embeddings
    layers = cfg.num_hidden_layers * (2.0 * T * (4 * d * d + 2 * d * I) + 4.0 * T * T * d) + 2.0 * T * d * dims[-1]
    return {"conv": round(conv / 1e9, 2), "posconv": round(pos / 1e9, 2), "layers": round(layers / 1e9, 2),
            "total": round((conv + pos + layers) / 1e9, 2)}


def main():
    ap = parser(steps=5, warmup=2, torch_yardstick=True)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--samples", type=int, default=160000)
    args = ap.parse_args()
    import w2v_ref
    from mmfusion import wav2vec2
    cfg = w2v_ref.base_config()
    sd = w2v_ref.seeded_weights(cfg, seed=0)
    model = wav2vec2.NativeWav2Vec2(**w2v_ref.config_kwargs(cfg))
    model.load_state_dict(sd)
    model = model.cuda().eval()
    N, L = args.clips, args.samples
    x = (0.5 * torch.randn(N, L, generator=torch.Generator().manual_seed(1))).cuda()
    gf = gflop_per_clip(cfg, L)

    def rate(ms: float) -> dict:
        return {"ms": round(ms, 3), "clips_per_s": round(N / ms * 1e3, 1), "tflops": round(gf["total"] * N / ms, 1)}

    res = {"model": "wav2vec2-base, frozen, bf16 storage", "clips": N, "samples": L, "frames": model.frames(L), "gflop_per_clip": gf,
           "default_chunk": wav2vec2.DEFAULT_CHUNK, "workspace_mb_per_clip": round(model.workspace_bytes_per_clip(L) / 2 ** 20, 2)}

    def measure(c):
        res[f"forward_chunk{c}"] = rate(time_eager(lambda: model(x), args.steps, args.warmup))
    sweep(model, wav2vec2.DEFAULT_CHUNK, args.chunks, measure)
    if args.table:
        res["kernels"] = kernel_table(lambda: model(x))
        print_table(res["kernels"])
    model._ws = None
    torch.cuda.empty_cache()
    if not args.no_torch:
        # the yardstick: the restatement itself in bf16 through stock torch, in chunks of the same size (the same memory bound)
        sd16 = {k: v.cuda().to(torch.bfloat16) for k, v in sd.items()}
        x16 = x.to(torch.bfloat16)
        c = wav2vec2.DEFAULT_CHUNK

        def stock():
            with torch.no_grad():
                return torch.cat([w2v_ref.w2v_forward(sd16, x16[i:i + c], cfg, dtype=torch.bfloat16, sdpa=True) for i in range(0, N, c)]).float()
        res["torch_bf16_forward"] = rate(time_eager(stock, args.steps, args.warmup))
        res["native_over_torch"] = round(res["torch_bf16_forward"]["ms"] / res[f"forward_chunk{c}"]["ms"], 3) if f"forward_chunk{c}" in res else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
