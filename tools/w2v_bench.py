#!/usr/bin/env python3
"""Cost of the native frozen Wav2Vec2 backbone (mmfusion.wav2vec2.NativeWav2Vec2, wav2vec2-base) on one batch of clips
(default 16 clips of 160000 samples = 10 s, what the reference pushes through its backbone per step):

  * ms per batch, clips/s and TFLOP/s (by operation count, printed as gflop_per_clip: feature-extractor convolutions,
    positional convolution, 12 layers at T = 499) of ``forward``, per chunk size;
  * the yardstick: tests/w2v_ref.py run in bf16 through stock torch (rocBLAS + torch's attention) on the same inputs with the
    same timing loop and the same chunking;
  * with --table, a per-kernel table of one batch from HIP events around every launch (mmfusion.lib.PROFILE): time, share,
    TFLOP/s where the wrapper counts operations.

  * with --finetune K|all|full, instead: forward + backward of ``set_trainable_layers(K)`` (``all``: every layer and the front end;
    ``full``: the feature extractor as well, its tensors leaves of the yardstick too) against the frozen forward, the per-kernel table of one step, stock-torch bf16 autograd through the same restatement with the
    same tensors as leaves, and (``all`` / ``full``) each kernel of the positional convolution's backward on one chunk beside the forward
    ``mmf_w2v_posconv``, which does the same FLOPs.  With --regularise as well: the same step in ``train()`` under
    wav2vec2-base-960h's regularisers (``mmfusion.wav2vec2.REG_960H``), with and without LayerDrop, and its per-kernel table.

  * --family NAME: a key of ``mmfusion.wav2vec2.FAMILIES`` instead of wav2vec2-base (seeded weights at its sizes).  On the
    layer-norm family (``large-lv60``) the yardstick is tests/w2v_ln_ref.py the same way, and --ln-kernels times, instead, the
    family's two kernels against the base family's on the family's own conv shapes and on the same buffers:
    ``mmf_w2v_ln_gelu_window`` against ``mmf_w2v_gelu_window`` and ``mmf_w2v_conv0_ln_gelu`` against ``mmf_w2v_conv0_norm_gelu``.

    python tools/w2v_bench.py [--family base] [--clips 16] [--samples 160000] [--chunks 4,8,16] [--steps 5] [--warmup 2] [--table]
                              [--no-torch] [--finetune K|all|full [--regularise]] [--ln-kernels]
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


def posconv_kernels(model, n: int, T: int, steps: int, warmup: int) -> dict:
    """each kernel of the positional convolution's backward on one chunk of ``n`` clips, ms and its ratio to the forward kernel"""
    from mmfusion import lib
    c = model.config
    d, G, k = c.hidden_size, c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings
    g = torch.Generator().manual_seed(3)
    x, dy = (torch.randn(n, T, d, generator=g).cuda().to(torch.bfloat16) for _ in range(2))
    y, dz = torch.empty_like(x), torch.empty_like(x)
    w, wt, b = model._pos_weight(), model._pos_weight(transposed=True), model._f("pos_b")
    S = model._pos_wgrad_slabs(n, T)
    dw = torch.zeros(d, model.pos_kp, device="cuda")
    partial = torch.empty(S, d * model.pos_kp, device="cuda")

    def wgrad():
        if S > 1:
            lib.w2v_posconv_wgrad(dz, x, partial, n, T, d, G, k, slabs=S)
            lib.sum_slabs(partial, dw.view(-1), True)
        else:
            lib.w2v_posconv_wgrad(dz, x, dw, n, T, d, G, k, accumulate=True)
    runs = {"posconv": lambda: lib.w2v_posconv(x, w, b, y, n, T, d, G, k),
            "posconv_bwd_act": lambda: lib.w2v_posconv_bwd_act(x, w, b, dy, dz, n, T, d, G, k),
            "posconv_dgrad": lambda: lib.w2v_posconv_dgrad(dz, wt, dy, y, n, T, d, G, k),
            "posconv_wgrad": wgrad,
            "weightnorm_bwd": lambda: lib.w2v_weightnorm_bwd(dw, model._f("pos_g"), model._f("pos_v"), torch.zeros_like(model.pos_g),
                                                            torch.empty_like(model.pos_v), True)}
    ms = {name: time_eager(fn, 4 * steps, warmup) for name, fn in runs.items()}
    out = {name: {"ms": round(v, 4), "over_forward_kernel": round(v / ms["posconv"], 3)} for name, v in ms.items()}
    out["wgrad_slabs"], out["gflop"] = S, round(2.0 * n * T * d * (d // G) * k / 1e9, 1)
    return out


def ln_kernels(model, n: int, samples: int, steps: int, warmup: int) -> dict:
    """the layer-norm family's two kernels against the base family's two, which move the same bytes, on one chunk of ``n`` clips at
    the model's conv shapes: ms (the inner layers' summed) and the ratios"""
    from mmfusion import lib
    from mmfusion.wav2vec2 import feat_lengths
    c = model.config
    dims, ks, ss = c.conv_dim, c.conv_kernel, c.conv_stride
    Ts = feat_lengths(samples, ks, ss)
    g = torch.Generator().manual_seed(4)
    wave = (0.5 * torch.randn(n, samples, generator=g)).cuda()
    w0, b0, gamma, beta = model._f("conv0_w"), model._f("conv0_b"), model._f("conv0_gn_w"), model._f("conv0_gn_b")
    stats = torch.empty(n * 2 * dims[0], device="cuda")
    partial = torch.empty(n * lib.W2V_STATS_SLOTS * 2 * dims[0], device="cuda")
    win = torch.empty(n * max(Ts[i] * ks[i] * dims[i - 1] for i in range(1, len(dims))), dtype=torch.bfloat16, device="cuda")
    lib.w2v_conv0_stats(wave, w0, stats, partial, ks[0], ss[0])
    ms = {"conv0_norm_gelu": time_eager(lambda: lib.w2v_conv0_norm_gelu(wave, w0, stats, gamma, beta, win, ks[0], ss[0], ks[1], ss[1], 1e-5), 4 * steps, warmup),
          "conv0_ln_gelu": time_eager(lambda: lib.w2v_conv0_ln_gelu(wave, w0, b0, gamma, beta, win, ks[0], ss[0], ks[1], ss[1], 1e-5), 4 * steps, warmup),
          "gelu_window": 0.0, "ln_gelu_window": 0.0}
    layers = []
    for i in range(1, len(dims) - 1):
        raw = torch.randn(n, Ts[i], dims[i], generator=g).cuda().to(torch.bfloat16)
        lw, lb, k, s = model._f(f"conv{i}_ln_w"), model._f(f"conv{i}_ln_b"), ks[i + 1], ss[i + 1]
        a = time_eager(lambda: lib.w2v_gelu_window(raw, win, n, Ts[i], dims[i], k, s), 4 * steps, warmup)
        b = time_eager(lambda: lib.w2v_ln_gelu_window(raw, lw, lb, win, n, Ts[i], dims[i], k, s, 1e-5), 4 * steps, warmup)
        ms["gelu_window"], ms["ln_gelu_window"] = ms["gelu_window"] + a, ms["ln_gelu_window"] + b
        layers.append({"layer": i, "T_in": Ts[i], "C": dims[i], "k": k, "s": s, "gelu_window_ms": round(a, 4), "ln_gelu_window_ms": round(b, 4),
                       "ratio": round(b / a, 3)})
    return {"clips": n, "samples": samples, "ms": {k: round(v, 4) for k, v in ms.items()}, "layers": layers,
            "ln_gelu_window_over_gelu_window": round(ms["ln_gelu_window"] / ms["gelu_window"], 3),
            "conv0_ln_gelu_over_conv0_norm_gelu": round(ms["conv0_ln_gelu"] / ms["conv0_norm_gelu"], 3)}


def finetune(args, model, cfg, sd, x, w2v_ref) -> dict:
    from mmfusion import arena, wav2vec2
    N, L, d = args.clips, cfg.num_hidden_layers, cfg.hidden_size
    full = args.finetune == "full"
    front = full or args.finetune == "all"
    k = L if front else int(args.finetune)
    T = model.frames(args.samples)
    res = {"model": f"wav2vec2-{args.family}, bf16 storage", "clips": N, "samples": args.samples, "frames": T, "chunk": model.chunk,
           "trainable_layers": k, "front": front, "feature_encoder": full}
    with torch.no_grad():
        res["forward_ms"] = round(time_eager(lambda: model(x), args.steps, args.warmup), 3)
    model.set_trainable_layers(k, front=front, feature_encoder=full)
    arena.ensure(model).zero_grad()
    dout = torch.randn(N, T, d, generator=torch.Generator().manual_seed(2)).cuda()

    def step():
        model(x).last_hidden_state.backward(dout)
    fwd = time_eager(lambda: model(x), args.steps, args.warmup)
    both = time_eager(step, args.steps, args.warmup)
    res["differentiable_forward_ms"], res["forward_backward_ms"] = round(fwd, 3), round(both, 3)
    res["forward_backward_ratio"] = round(both / res["forward_ms"], 3)
    res["saved_inputs_mb"] = round((k * d + (cfg.conv_dim[-1] if front else 0) + (d if cfg.do_stable_layer_norm else 0)) * N * T * 2 / 2 ** 20, 1)
    res["grad_workspace_mb_per_clip"] = round(model.grad_workspace_bytes_per_clip(args.samples) / 2 ** 20, 2)
    res["kernels"] = kernel_table(step)
    print_table(res["kernels"])
    if args.regularise:
        # the same step under wav2vec2-base-960h's training regime (train() mode; LayerDrop skips a tenth of the layers, so the figure
        # with it is an average over the steps' skip patterns, and the one without it is given beside it)
        model.train()
        for name, settings in (("regularised", wav2vec2.REG_960H), ("regularised_no_layerdrop", dict(wav2vec2.REG_960H, layerdrop=0.0))):
            model.set_regularisation(**settings)
            model.layerdrop_generator.manual_seed(0)
            ms = time_eager(step, args.steps, args.warmup)
            res[name + "_forward_backward_ms"], res[name + "_over_plain"] = round(ms, 3), round(ms / both, 4)
        res["regularised_kernels"] = kernel_table(step)               # (no LayerDrop: every layer's launches)
        print_table(res["regularised_kernels"])
        model.set_regularisation(**{n: 0.0 for n in wav2vec2.REG_NAMES[:6]})
        model.eval()
    if front:
        res["posconv_kernels"] = posconv_kernels(model, min(model.chunk, N), T, args.steps, args.warmup)
    if not args.no_torch:
        model._ws = model._gws = model._slabs = None
        torch.cuda.empty_cache()
        keys = {n for n in sd if any(n.startswith(f"encoder.layers.{i}.") for i in range(L - k, L))
                or (front and n.startswith(("feature_projection.", "encoder.pos_conv_embed.", "encoder.layer_norm.")))
                or (cfg.do_stable_layer_norm and n.startswith("encoder.layer_norm."))
                or (full and n.startswith("feature_extractor."))}
        leaves = {n: v.cuda().to(torch.bfloat16).requires_grad_(n in keys) for n, v in sd.items()}
        x16, d16, c = x.to(torch.bfloat16), dout.to(torch.bfloat16), wav2vec2.DEFAULT_CHUNK

        def stock(backward):
            for i in range(0, N, c):
                out = w2v_ref.w2v_forward(leaves, x16[i:i + c], cfg, dtype=torch.bfloat16, sdpa=True)
                if backward:
                    out.backward(d16[i:i + c])
        res["torch_bf16_forward_ms"] = round(time_eager(lambda: stock(False), args.steps, args.warmup), 3)
        res["torch_bf16_forward_backward_ms"] = round(time_eager(lambda: stock(True), args.steps, args.warmup), 3)
        res["speedup_forward_backward"] = round(res["torch_bf16_forward_backward_ms"] / both, 3)
    return res


def main():
    ap = parser(steps=5, warmup=2, torch_yardstick=True)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--finetune", default=None, metavar="K|all|full")
    ap.add_argument("--regularise", action="store_true", help="with --finetune: also time the step under wav2vec2-base-960h's regularisers")
    ap.add_argument("--family", default="base", help="a key of mmfusion.wav2vec2.FAMILIES")
    ap.add_argument("--ln-kernels", action="store_true", help="the layer-norm family's two kernels against the base family's (large-lv60)")
    args = ap.parse_args()
    from mmfusion import wav2vec2
    if args.family not in wav2vec2.FAMILIES:
        ap.error(f"--family {args.family}: one of {', '.join(wav2vec2.FAMILIES)}")
    model = wav2vec2.NativeWav2Vec2(**wav2vec2.FAMILIES[args.family])
    cfg = model.config                                            # (the restatements read the sizes and the three switches from it)
    if cfg.do_stable_layer_norm:
        import w2v_ln_ref as w2v_ref
    else:
        import w2v_ref
    sd = w2v_ref.seeded_weights(cfg, seed=0)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    N, L = args.clips, args.samples
    if args.ln_kernels:
        if not cfg.do_stable_layer_norm:
            ap.error("--ln-kernels goes with a layer-norm family (--family large-lv60)")
        print(json.dumps(ln_kernels(model, min(model.chunk, N), L, args.steps, args.warmup)))
        return
    x = (0.5 * torch.randn(N, L, generator=torch.Generator().manual_seed(1))).cuda()
    if args.finetune is not None:
        print(json.dumps(finetune(args, model, cfg, sd, x, w2v_ref)))
        return
    gf = gflop_per_clip(cfg, L)

    def rate(ms: float) -> dict:
        return {"ms": round(ms, 3), "clips_per_s": round(N / ms * 1e3, 1), "tflops": round(gf["total"] * N / ms, 1)}

    res = {"model": f"wav2vec2-{args.family}, frozen, bf16 storage", "clips": N, "samples": L, "frames": model.frames(L), "gflop_per_clip": gf,
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
