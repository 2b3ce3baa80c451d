#!/usr/bin/env python3
"""Cost of the native frozen WavLM backbone (mmfusion.wavlm.NativeWavLM, wavlm-base sizes, seeded weights) on one batch of clips
(default 16 clips of 160000 samples = 10 s -> 499 frames):

  (a) ``forward`` against HuggingFace's ``WavLMModel`` in bf16 through stock torch on the same GPU, same inputs, same timing loop
      (that model materialises a (B H, T, T) position bias per layer); skipped with --no-torch or where transformers is missing;
  (b) ``mmf_attn_fwd_relbias`` against ``mmf_attn_fwd_grouped`` on the same problem (B = clips, H = 12, T = 499, head_dim 64, the
      fused qkv rows): the plain forward is the yardstick, the ratio is what the bias costs;
  (c) ``mmf_wavlm_gate`` on that batch's layer input, with the bytes it has to move;
  and, with --table, the per-kernel table of one forward from HIP events around every launch (mmfusion.lib.PROFILE).

(b) and (c) are timed in windows of --launches back-to-back launches between two HIP events, the two attention kernels alternating
window by window over --rounds rounds (the median window is reported with the spread), so that a drifting clock or a neighbour on
the host hits both alike.

    python tools/wavlm_bench.py [--clips 16] [--samples 160000] [--steps 5] [--warmup 2] [--launches 200] [--rounds 7] [--table] [--no-torch]
Prints one JSON line (the table, when asked for, on the lines before it)."""
import json
import statistics

from backbone_bench import kernel_table, parser, print_table, time_eager  # (first: it sets the import path)
import torch


def windows(fns: dict, launches: int, rounds: int) -> dict:
    """us per launch of each ``fns[name]``: ``rounds`` windows of ``launches`` launches each, the functions alternating"""
    for fn in fns.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            us[name].append(time_eager(fn, launches, 0) * 1e3)
    return {name: {"us": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for name, v in us.items()}


def kernels(model, n: int, T: int, launches: int, rounds: int) -> dict:
    from mmfusion import lib
    c, dh = model.config, model.head_dim
    H, d = c.num_attention_heads, c.hidden_size
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n * T, d, generator=g).cuda().to(torch.bfloat16)
    qkv = torch.randn(n * T, 3 * d, generator=g).cuda().to(torch.bfloat16)
    att, att2 = torch.empty(n * T, d, dtype=torch.bfloat16, device="cuda"), torch.empty(n * T, d, dtype=torch.bfloat16, device="cuda")
    ws = {"lse": torch.empty(n * H * T, device="cuda")}
    gate = torch.empty(n * H * T, device="cuda")
    table = model._table(T, x.device)
    p, p2 = model._attn_problem(ws, qkv, att, n, T, T), model._attn_problem(ws, qkv, att2, n, T, T)
    w, b, k = model._f("l0_gate_w"), model._f("l0_gate_b"), model._f("l0_gate_c").view(H)
    lib.wavlm_gate(x, w, b, k, gate, n, T, H, dh)
    res = windows({"attn_fwd_relbias": lambda: lib.attn_fwd_relbias(p, dh, dh ** -0.5, gate, table),
                   "attn_fwd_grouped": lambda: lib.attn_fwd_grouped([p2], dh, dh ** -0.5)}, launches, rounds)
    res.update(windows({"wavlm_gate": lambda: lib.wavlm_gate(x, w, b, k, gate, n, T, H, dh)}, launches, rounds))
    flop = 4.0 * n * H * T * T * dh
    for name in ("attn_fwd_relbias", "attn_fwd_grouped"):
        res[name]["tflops"] = round(flop / res[name]["us"] / 1e6, 1)
    res["relbias_over_plain"] = round(res["attn_fwd_relbias"]["us"] / res["attn_fwd_grouped"]["us"], 4)
    nbytes = n * T * d * 2 + n * H * T * 4
    res["wavlm_gate"].update(mbytes=round(nbytes / 2 ** 20, 2), tb_per_s=round(nbytes / res["wavlm_gate"]["us"] / 1e6, 2))
    res["problem"] = {"B": n, "H": H, "T": T, "head_dim": dh, "launches_per_window": launches, "rounds": rounds}
    return res


def main():
    ap = parser(steps=5, warmup=2, torch_yardstick=True)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import wavlm_ref
    from mmfusion import wavlm
    model = wavlm.NativeWavLM(**wavlm.FAMILIES["base"])
    cfg = model.config
    sd = wavlm_ref.seeded_weights(cfg, seed=0)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    N, L = args.clips, args.samples
    T = model.frames(L)
    x = (0.5 * torch.randn(N, L, generator=torch.Generator().manual_seed(1))).cuda()
    res = {"model": "wavlm-base, frozen, bf16 storage", "clips": N, "samples": L, "frames": T, "chunk": model.chunk,
           "workspace_mb_per_clip": round(model.workspace_bytes_per_clip(L) / 2 ** 20, 2)}
    ms = time_eager(lambda: model(x), args.steps, args.warmup)
    res["forward"] = {"ms": round(ms, 3), "clips_per_s": round(N / ms * 1e3, 1)}
    if args.table:
        res["kernels_of_one_forward"] = kernel_table(lambda: model(x))
        print_table(res["kernels_of_one_forward"])
    res["kernels"] = kernels(model, min(model.chunk, N), T, args.launches, args.rounds)
    model._ws = None
    torch.cuda.empty_cache()
    if not args.no_torch:
        try:
            import transformers
        except ImportError:
            transformers = None
        if transformers is None:
            res["torch_bf16_forward"] = "not measured: transformers does not import"
        else:
            keys = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "conv_dim", "conv_kernel", "conv_stride",
                    "conv_bias", "num_conv_pos_embeddings", "num_conv_pos_embedding_groups", "layer_norm_eps", "feat_extract_norm",
                    "do_stable_layer_norm", "num_buckets", "max_bucket_distance")
            hf = transformers.WavLMModel(transformers.WavLMConfig(**{k: getattr(cfg, k) for k in keys})).eval()
            hf.load_state_dict(sd)
            hf = hf.cuda().to(torch.bfloat16)
            x16 = x.to(torch.bfloat16)

            def stock():
                with torch.no_grad():
                    return torch.cat([hf(x16[i:i + model.chunk]).last_hidden_state for i in range(0, N, model.chunk)]).float()
            tms = time_eager(stock, args.steps, args.warmup)
            res["torch_bf16_forward"] = {"ms": round(tms, 3), "clips_per_s": round(N / tms * 1e3, 1)}
            res["native_over_torch"] = round(tms / ms, 3)
            with torch.no_grad():
                a, b = model(x[:2]).last_hidden_state, hf(x16[:2]).last_hidden_state.float()
            res["native_vs_torch_bf16_rel_l2"] = round(float((a - b).norm() / b.norm()), 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
