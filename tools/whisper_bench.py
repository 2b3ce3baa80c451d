#!/usr/bin/env python3
"""Cost of the native frozen Whisper encoder (mmfusion.whisper.NativeWhisperEncoder, whisper-small sizes, seeded weights) on one
batch of clips (default 16 clips at the 30 s window -> 3000 mel frames -> 1500 frames, and again at a 10 s window):

  (a) ``forward(waveform)`` (log-mel on the device included) and ``forward(input_features=)`` against HuggingFace's
      ``WhisperEncoder`` in bf16 through stock torch on the same GPU from PRECOMPUTED ``input_features``, same timing loop, and,
      separately, the wall time ``WhisperFeatureExtractor`` takes on the host for the same clips (numpy, one clip at a time), which
      the stock route pays in front of its encoder; skipped with --no-torch or where transformers is missing;
  (b) the log-mel launches alone (``mmf_whisper_logmel``: the window form only, as the forward calls it, and with the features too);
  (c) ``mmf_whisper_gelu_window`` against ``mmf_w2v_gelu_window`` on the same element count (the yardstick: what the bias and the
      padding cost), and ``mmf_whisper_stem_out`` with the bytes it has to move;
  (d) conv1's GEMM at K = 240 (the general ring, what the forward runs) against K = 256 (zero columns: the persistent kernel);
  and, with --table, the per-kernel table of one forward from HIP events around every launch (mmfusion.lib.PROFILE).

(b), (c) and the GEMMs of (d) are timed in windows of --launches back-to-back launches between two HIP events, alternating window by
window over --rounds rounds (the median window is reported with the spread).

    python tools/whisper_bench.py [--clips 16] [--steps 5] [--warmup 2] [--launches 100] [--rounds 7] [--table] [--no-torch]
Prints one JSON line (the table, when asked for, on the lines before it)."""
import json
import time

from backbone_bench import kernel_table, parser, print_table, time_eager  # (first: it sets the import path)
import numpy as np
import torch

from wavlm_bench import windows

BF16 = torch.bfloat16


def build(whisper, sd_of, positions: int, **kw):
    m = whisper.NativeWhisperEncoder(**{**whisper.FAMILIES["small"], "max_source_positions": positions, **kw})
    m.load_state_dict(sd_of(m))
    return m.cuda().eval()


def front_end(model, n: int, launches: int, rounds: int) -> dict:
    """(b), (c) and the GEMMs of (d) on a chunk of ``n`` clips"""
    from mmfusion import lib, ops
    from mmfusion.lib import GEMM_NT
    c = model.config
    T, Tm, d, M = c.max_source_positions, model.mel_frames, c.d_model, c.num_mel_bins
    g = torch.Generator().manual_seed(5)
    wave = (0.3 * torch.randn(n, model.n_samples, generator=g)).cuda()
    tabs = model._tables(wave.device)
    scratch = torch.empty(lib.whisper_logmel_scratch_bytes(n, model.n_samples, M) // 4, device="cuda")
    feats = torch.empty(n, M, Tm, device="cuda")
    win = {K: torch.zeros(n, Tm, K, dtype=BF16, device="cuda") for K in (3 * M, 256)}
    res = windows({"logmel_window_only": lambda: lib.whisper_logmel(wave, *tabs, scratch, model.n_samples, out_window=win[3 * M]),
                   "logmel_window_and_features": lambda: lib.whisper_logmel(wave, *tabs, scratch, model.n_samples, features=feats, out_window=win[3 * M]),
                   "feature_window": lambda: lib.whisper_feature_window(feats, win[3 * M])}, launches, rounds)
    flop = 2.0 * n * Tm * 400 * 402
    for k in ("logmel_window_only", "logmel_window_and_features"):
        res[k]["dft_tflops"] = round(flop / res[k]["us"] / 1e6, 2)
    raw = torch.randn(n * Tm, d, generator=g).cuda().to(BF16)
    bias = torch.randn(d, generator=g).cuda()
    win2 = torch.empty(n * T * 3 * d, dtype=BF16, device="cuda")
    w2v_T = 2 * T + 1                                               # (w2v_T - 3) / 2 + 1 = T rows of 3 d: the same element count
    raw_w2v = torch.randn(n * w2v_T, d, generator=g).cuda().to(BF16)
    res.update(windows({"whisper_gelu_window": lambda: lib.whisper_gelu_window(raw, bias, win2, n, Tm, d, 3, 2, 1),
                        "w2v_gelu_window": lambda: lib.w2v_gelu_window(raw_w2v, win2, n, w2v_T, d, 3, 2)}, launches, rounds))
    res["whisper_over_w2v_gelu_window"] = round(res["whisper_gelu_window"]["us"] / res["w2v_gelu_window"]["us"], 4)
    x = torch.randn(n * T, d, generator=g).cuda().to(BF16)
    out = torch.empty_like(x)
    res.update(windows({"whisper_stem_out": lambda: lib.whisper_stem_out(x, bias, model._f("pos_emb"), out, T)}, launches, rounds))
    nbytes = 2 * x.numel() * 2 + T * d * 4
    res["whisper_stem_out"].update(mbytes=round(nbytes / 2 ** 20, 2), tb_per_s=round(nbytes / res["whisper_stem_out"]["us"] / 1e6, 2))
    nbytes = (raw.numel() + win2.numel()) * 2
    res["whisper_gelu_window"].update(mbytes=round(nbytes / 2 ** 20, 2), tb_per_s=round(nbytes / res["whisper_gelu_window"]["us"] / 1e6, 2))
    w = {K: torch.zeros(d, K, dtype=BF16, device="cuda") for K in win}
    for K in w:
        w[K][:, :3 * M] = torch.randn(d, 3 * M, generator=g).cuda().to(BF16)
    conv1 = torch.empty(n * Tm, d, dtype=BF16, device="cuda")
    gemms = windows({f"conv1_gemm_K{K}": (lambda K=K: ops.gemm(GEMM_NT, win[K].view(n * Tm, K), w[K], conv1)) for K in w}, launches, rounds)
    for K in w:
        ops.gemm(GEMM_NT, win[K].view(n * Tm, K), w[K], conv1)
        gemms[f"conv1_gemm_K{K}"]["impl"] = int(lib.load().mmf_gemm_last_impl())
    res.update(gemms)
    res["problem"] = {"clips": n, "mel_frames": Tm, "frames": T, "d_model": d, "launches_per_window": launches, "rounds": rounds}
    return res


def main():
    ap = parser(steps=5, warmup=2, torch_yardstick=True)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import types

    import whisper_ref
    from mmfusion import whisper
    N = args.clips
    res = {"model": "whisper-small encoder, frozen, bf16 storage", "clips": N}

    def sd_of(m):
        c = m.config
        return whisper_ref.seeded_weights(types.SimpleNamespace(d_model=c.d_model, encoder_layers=c.encoder_layers, encoder_ffn_dim=c.encoder_ffn_dim,
                                                                num_mel_bins=c.num_mel_bins, max_source_positions=c.max_source_positions), seed=0)
    for label, positions in (("window_30s", 1500), ("window_10s", 500)):
        model = build(whisper, sd_of, positions)
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        clips = np.stack([whisper_ref.speech_like(model.n_samples, seed=i) for i in range(N)])
        x = torch.from_numpy(clips).cuda()
        feats = model.features(x)
        r = {"samples": model.n_samples, "frames": positions, "chunk": model.chunk, "conv1_K": model.kw,
             "workspace_mb_per_clip": round(model.workspace_bytes_per_clip() / 2 ** 20, 2)}
        ms = time_eager(lambda: model(x), args.steps, args.warmup)
        r["forward_waveform"] = {"ms": round(ms, 3), "clips_per_s": round(N / ms * 1e3, 1)}
        fms = time_eager(lambda: model(input_features=feats), args.steps, args.warmup)
        r["forward_input_features"] = {"ms": round(fms, 3), "clips_per_s": round(N / fms * 1e3, 1)}
        if args.table and positions == 1500:
            res["kernels_of_one_forward"] = kernel_table(lambda: model(x))
            print_table(res["kernels_of_one_forward"])
        if positions == 1500:
            res["kernels"] = front_end(model, min(model.chunk, N), args.launches, args.rounds)
        model._ws = None
        torch.cuda.empty_cache()
        if not args.no_torch:
            try:
                import transformers
            except ImportError:
                transformers = None
            if transformers is None:
                r["torch_bf16_forward"] = "not measured: transformers does not import"
            else:
                from transformers.models.whisper.modeling_whisper import WhisperEncoder
                c = model.config
                hf = WhisperEncoder(transformers.WhisperConfig(d_model=c.d_model, encoder_layers=c.encoder_layers,
                                                               encoder_attention_heads=c.encoder_attention_heads, encoder_ffn_dim=c.encoder_ffn_dim,
                                                               num_mel_bins=c.num_mel_bins, max_source_positions=positions)).eval()
                hf.load_state_dict(sd)
                hf = hf.cuda().to(BF16)
                f16 = feats.to(BF16)

                def stock():
                    with torch.no_grad():
                        return torch.cat([hf(f16[i:i + model.chunk]).last_hidden_state for i in range(0, N, model.chunk)]).float()
                tms = time_eager(stock, args.steps, args.warmup)
                r["torch_bf16_forward_from_features"] = {"ms": round(tms, 3), "clips_per_s": round(N / tms * 1e3, 1)}
                r["native_waveform_over_torch_features"] = round(tms / ms, 3)
                r["native_features_over_torch_features"] = round(tms / fms, 3)
                with torch.no_grad():
                    a, b = model(x[:2]).last_hidden_state, hf(f16[:2]).last_hidden_state.float()
                r["native_vs_torch_bf16_rel_l2"] = round(float((a - b).norm() / b.norm()), 5)
                fe = transformers.WhisperFeatureExtractor(feature_size=c.num_mel_bins, chunk_length=model.n_samples // 16000)
                fe(list(clips[:1]), sampling_rate=16000, return_tensors="np")
                t0 = time.perf_counter()
                host = fe(list(clips), sampling_rate=16000, return_tensors="np").input_features
                r["host_feature_extractor_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                r["device_features_vs_host_max_abs"] = float(np.abs(feats.cpu().numpy() - host).max())
                del hf
                torch.cuda.empty_cache()
        res[label] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
