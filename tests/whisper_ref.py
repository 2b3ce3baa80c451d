"""An explicit float64 restatement of HuggingFace's Whisper front end and encoder: ``WhisperFeatureExtractor``'s log-mel features
(``_np_extract_fbank_features``), the two padded convolutions and ``WhisperEncoder`` in eval mode.  It imports neither
transformers nor the code under test: the window, the Slaney filter bank and the sinusoids are written out here a second time.

``bf16_storage`` rounds where the HIP path (mmfusion/whisper.py) stores bf16: the log-mel window form, the GEMM weights, both
convolutions' raw outputs, the GELU outputs, the residual stream and every layer buffer.

Named mutants, each a mistake the tests must be able to see (``LOGMEL_MUTANTS`` / ``ENCODER_MUTANTS``):
  symmetric_hann     the symmetric Hann window in place of the periodic one
  no_reflect         zeros in place of the 200 reflected samples on both sides
  last_frame_kept    frames 1 .. Tm of the Tm + 1 in place of 0 .. Tm - 1 (the extractor drops the LAST one)
  batch_max          the clamp's maximum taken over the whole batch, not per clip
  pad0               the convolutions read frames s t + j (no left padding; the zeros all behind the clip)
  pos_before_gelu    the positions added in front of the second GELU
  key_bias           the biases dealt out as though k_proj had one (k, v, q in HuggingFace's order get v's, q's and none).  A true
                     bias on the keys would cancel in the softmax, so this is the form the mistake takes
  post_ln            the layers as post-LN blocks
"""
import functools
import math
import types

import numpy as np
import torch

from backbone_ref import _r, gelu_erf, layer_norm  # noqa: F401

N_FFT, HOP = 400, 160
LOGMEL_MUTANTS = ("symmetric_hann", "no_reflect", "last_frame_kept", "batch_max")
ENCODER_MUTANTS = ("pad0", "pos_before_gelu", "key_bias", "post_ln")


def tiny_config(**over):
    base = dict(d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=256, num_mel_bins=80, max_source_positions=100)
    return types.SimpleNamespace(**{**base, **over})


def config_kwargs(cfg):
    return dict(vars(cfg))


def hf_keys(cfg):
    """the ``WhisperEncoder`` state_dict: key -> shape, in HuggingFace's order (``k_proj`` has no bias)"""
    d, I, M, T = cfg.d_model, cfg.encoder_ffn_dim, cfg.num_mel_bins, cfg.max_source_positions
    out = {"conv1.weight": (d, M, 3), "conv1.bias": (d,), "conv2.weight": (d, d, 3), "conv2.bias": (d,), "embed_positions.weight": (T, d)}
    for i in range(cfg.encoder_layers):
        a = f"layers.{i}."
        out[a + "self_attn.k_proj.weight"] = (d, d)
        for p in ("v_proj", "q_proj", "out_proj"):
            out[a + f"self_attn.{p}.weight"], out[a + f"self_attn.{p}.bias"] = (d, d), (d,)
        out[a + "self_attn_layer_norm.weight"], out[a + "self_attn_layer_norm.bias"] = (d,), (d,)
        out[a + "fc1.weight"], out[a + "fc1.bias"] = (I, d), (I,)
        out[a + "fc2.weight"], out[a + "fc2.bias"] = (d, I), (d,)
        out[a + "final_layer_norm.weight"], out[a + "final_layer_norm.bias"] = (d,), (d,)
    out["layer_norm.weight"], out["layer_norm.bias"] = (d,), (d,)
    return out


def sinusoids(length: int, channels: int) -> torch.Tensor:
    """float32, in HuggingFace's order of operations"""
    inc = math.log(10000.0) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2))
    t = torch.arange(length).view(-1, 1) * inv.view(1, -1)
    return torch.cat([t.sin(), t.cos()], dim=1)


def seeded_weights(cfg, seed: int = 0):
    """1/sqrt(fan_in)-scaled matrices (q / k 1.5 times that: softmax rows far from uniform), non-trivial biases and LayerNorm
    parameters; ``embed_positions`` is the sinusoid table plus a little noise, so that a copy of it is told from a rebuilt table"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in hf_keys(cfg).items():
        t = torch.randn(shape, generator=g)
        if k.endswith("layer_norm.weight"):
            t = 1.0 + 0.2 * t
        elif k.endswith(".bias"):
            t = 0.1 * t
        elif k == "embed_positions.weight":
            t = sinusoids(*shape) + 0.05 * t
        else:
            t = t / math.sqrt(t[0].numel()) * (1.5 if ("q_proj" in k or "k_proj" in k) else 1.0)
        sd[k] = t
    return sd


# ---- the log-mel features -------------------------------------------------------------------------------------------------
def hann(n: int = N_FFT, periodic: bool = True) -> np.ndarray:
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / (n if periodic else n - 1)) for i in range(n)])


def slaney_mel(hz: float) -> float:
    return 3.0 * hz / 200.0 if hz < 1000.0 else 15.0 + math.log(hz / 1000.0) * 27.0 / math.log(6.4)


def slaney_hz(mel: float) -> float:
    return 200.0 * mel / 3.0 if mel < 15.0 else 1000.0 * math.exp(math.log(6.4) / 27.0 * (mel - 15.0))


@functools.lru_cache(maxsize=None)
def filter_bank(n_mels: int, n_bins: int = 201, sr: int = 16000, f_max: float = 8000.0) -> np.ndarray:
    """(n_bins, n_mels): triangles between consecutive mel-spaced edges, each scaled by 2 / (its width in Hz), one entry at a time
    (cached: read it, do not write to it)"""
    top = slaney_mel(f_max)
    edges = [slaney_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    fb = np.zeros((n_bins, n_mels))
    for b in range(n_bins):
        hz = (sr / 2.0) * b / (n_bins - 1)
        for m in range(n_mels):
            lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
            v = min((hz - lo) / (mid - lo), (hi - hz) / (hi - mid))
            if v > 0.0:
                fb[b, m] = v * 2.0 / (hi - lo)
    return fb


def frames_of(wave, n_samples: int, mutant=None) -> np.ndarray:
    """wave (L,) -> the windowless frames (Tm + 1, 400) of the clip padded to ``n_samples`` and then by 200 on both sides"""
    x = np.zeros(n_samples)
    x[:len(wave)] = np.asarray(wave, dtype=np.float64)
    padded = np.pad(x, 200, mode="constant" if mutant == "no_reflect" else "reflect")
    count = 1 + n_samples // HOP
    return np.stack([padded[HOP * t:HOP * t + N_FFT] for t in range(count)])


def power_and_mel(wave, n_mels: int, max_source_positions: int, mutant=None):
    """one clip -> (|X| (frames, 201), mel (frames, n_mels), sum_t |x_t w_t| per frame) over the frames the extractor keeps"""
    w = hann(periodic=mutant != "symmetric_hann")
    fr = frames_of(wave, 320 * max_source_positions, mutant) * w
    fr = fr[1:] if mutant == "last_frame_kept" else fr[:-1]
    mag = np.abs(np.fft.rfft(fr, axis=1))
    return mag, (mag ** 2) @ filter_bank(n_mels), np.abs(fr).sum(axis=1)


def log_mel(waves, n_mels: int, max_source_positions: int, mutant=None) -> np.ndarray:
    """waves: (B, L) or a list of (L_i,) -> (B, n_mels, Tm) float64, HuggingFace's ``input_features``"""
    logs = [np.log10(np.maximum(power_and_mel(np.asarray(w), n_mels, max_source_positions, mutant)[1], 1e-10)).T for w in waves]
    out = []
    for lg in logs:
        top = max(l.max() for l in logs) if mutant == "batch_max" else lg.max()
        out.append((np.maximum(lg, top - 8.0) + 4.0) / 4.0)
    return np.stack(out)


def log_mel_bound(waves, n_mels: int, max_source_positions: int) -> np.ndarray:
    """The per-element bound of an f32 DFT against ``log_mel`` (tests/test_whisper_kernels_gpu.py's docstring derives it):
    2^-16 + (E / mel) / (4 ln 10) with E = sum_f M[f][m] (2 |X_f| e + e^2) + 2^-22 mel and e = 2^-21 sum_t |x_t w_t| of the frame,
    raised to the bound of the clip's arg-max element (the clamp is 1-Lipschitz in both arguments).  (B, n_mels, Tm)"""
    fb = filter_bank(n_mels)
    out = []
    for w in waves:
        mag, mel, l1 = power_and_mel(np.asarray(w), n_mels, max_source_positions)
        e = (2.0 ** -21) * l1[:, None]
        E = (2.0 * mag * e + e * e) @ fb + (2.0 ** -22) * mel
        b = 2.0 ** -16 + (E / np.maximum(mel, 1e-10)) / (4.0 * math.log(10.0))
        b = np.maximum(b, b.flat[np.argmax(mel)])
        out.append(b.T)
    return np.stack(out)


def window_form(feat: torch.Tensor, k: int, s: int, pad: int, left: bool = True) -> torch.Tensor:
    """(N, T_in, C) -> (N, T_out, k C): row t holds frames s t + j - pad, j = 0 .. k - 1, zeros outside the clip.  ``left`` False:
    the ``pad0`` mutant's indexing (frames s t + j, all 2 pad zeros behind the clip)"""
    N, T_in, C = feat.shape
    T_out = (T_in + 2 * pad - k) // s + 1
    z = feat.new_zeros(N, pad, C)
    padded = torch.cat([z, feat, z], dim=1) if left else torch.cat([feat, z, z], dim=1)
    return torch.stack([padded[:, s * t:s * t + k].reshape(N, k * C) for t in range(T_out)], dim=1)


# ---- the encoder ----------------------------------------------------------------------------------------------------------
def stem_forward(sd, feats, cfg, dtype=torch.float64, bf16_storage: bool = False, mutant=None):
    """input_features (N, M, Tm) -> the residual stream's first value (N, T, d)"""
    on = bf16_storage
    W = lambda k: _r(sd[k].to(dtype), on, dtype)
    F = lambda k: sd[k].to(dtype)
    d, left = cfg.d_model, mutant != "pad0"
    x = _r(torch.as_tensor(feats).to(dtype).transpose(1, 2), on, dtype)                  # (N, Tm, M): the window form's bf16
    w1 = W("conv1.weight").permute(0, 2, 1).reshape(d, -1)                               # column (tap, channel)
    raw1 = _r(window_form(x, 3, 1, 1, left) @ w1.T, on, dtype)
    g1 = _r(gelu_erf(raw1 + F("conv1.bias")), on, dtype)
    w2 = W("conv2.weight").permute(0, 2, 1).reshape(d, -1)
    raw2 = _r(window_form(g1, 3, 2, 1, left) @ w2.T, on, dtype)
    pos = F("embed_positions.weight")
    if mutant == "pos_before_gelu":
        return _r(gelu_erf(raw2 + F("conv2.bias") + pos), on, dtype)
    return _r(gelu_erf(raw2 + F("conv2.bias")) + pos, on, dtype)


def encoder_forward(sd, feats, cfg, dtype=torch.float64, bf16_storage: bool = False, mutant=None, eps: float = 1e-5):
    """input_features (N, M, Tm) -> last_hidden_state (N, T, d) in ``dtype``"""
    on = bf16_storage
    W = lambda k: _r(sd[k].to(dtype), on, dtype)
    F = lambda k: sd[k].to(dtype)
    d, H = cfg.d_model, cfg.encoder_attention_heads
    dh = d // H
    x = stem_forward(sd, feats, cfg, dtype, on, mutant)
    N, T = x.shape[:2]
    for i in range(cfg.encoder_layers):
        a, b = f"layers.{i}.self_attn.", f"layers.{i}."
        ln_a = lambda t: layer_norm(t, F(b + "self_attn_layer_norm.weight"), F(b + "self_attn_layer_norm.bias"), eps)
        ln_f = lambda t: layer_norm(t, F(b + "final_layer_norm.weight"), F(b + "final_layer_norm.bias"), eps)
        zero = torch.zeros(d, dtype=dtype)
        bq, bk, bv = F(a + "q_proj.bias"), zero, F(a + "v_proj.bias")
        if mutant == "key_bias":
            bk, bv, bq = F(a + "v_proj.bias"), F(a + "q_proj.bias"), zero
        post = mutant == "post_ln"
        src = x if post else _r(ln_a(x), on, dtype)
        q, k, v = (_r(src @ W(a + f"{p}_proj.weight").T + bias, on, dtype).reshape(N, T, H, dh).transpose(1, 2)
                   for p, bias in (("q", bq), ("k", bk), ("v", bv)))
        p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh), dim=-1)
        att = _r((p @ v).transpose(1, 2).reshape(N, T, d), on, dtype)
        y = _r(att @ W(a + "out_proj.weight").T + F(a + "out_proj.bias") + x, on, dtype)
        if post:
            y = _r(ln_a(y), on, dtype)
        src = y if post else _r(ln_f(y), on, dtype)
        h = _r(src @ W(b + "fc1.weight").T, on, dtype)                                   # the GELU input as stored (bias added in f32)
        g = _r(gelu_erf(h + F(b + "fc1.bias")), on, dtype)
        x = _r(g @ W(b + "fc2.weight").T + F(b + "fc2.bias") + y, on, dtype)
        if post:
            x = _r(ln_f(x), on, dtype)
    return _r(layer_norm(x, F("layer_norm.weight"), F("layer_norm.bias"), eps), on, dtype)


def whisper_forward(sd, wave, cfg, dtype=torch.float64, bf16_storage: bool = False, mutant=None):
    """waveform (N, L) -> last_hidden_state: ``log_mel`` in float64, then ``encoder_forward``"""
    feats = torch.from_numpy(log_mel(np.asarray(wave, dtype=np.float64), cfg.num_mel_bins, cfg.max_source_positions,
                                     mutant if mutant in LOGMEL_MUTANTS else None))
    return encoder_forward(sd, feats, cfg, dtype, bf16_storage, mutant if mutant in ENCODER_MUTANTS else None)


def speech_like(L: int, seed: int = 0) -> np.ndarray:
    """a decaying 150 Hz pulse train plus a gated 2.3 kHz tone plus 1e-3 noise: 60 dB between its loud and quiet bins"""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / 16000.0
    phase = (t * 150.0) % 1.0
    pulses = np.exp(-phase * 12.0) * np.exp(-t * 1.5)
    gate = ((t * 4.0) % 1.0) < 0.4
    return (0.6 * pulses + 0.2 * gate * np.sin(2.0 * np.pi * 2300.0 * t) + 1e-3 * rng.standard_normal(L)).astype(np.float32)


def load_golden(path):
    """-> (state dict, waveform (N, L) f32, input_features (N, M, Tm) f32, last_hidden_state (N, T, d) f32) as captured from
    HuggingFace on the CPU (tools/capture_whisper_golden.py: matrices as four-level int8 codes times a scale, the waveform as int16
    over 2^15, both exact)"""
    z = np.load(path)
    sd = {}
    for name in z.files:
        tag, _, k = name.partition(":")
        if tag == "q":
            sd[k] = torch.from_numpy(z[name].astype(np.float32)) * float(z["s:" + k])
        elif tag == "f":
            sd[k] = torch.from_numpy(z[name])
    cfg = tiny_config()
    sd = {k: sd[k] for k in hf_keys(cfg)}
    wave = torch.from_numpy(z["wave_q15"].astype(np.float32) / 32768.0)
    return sd, wave, torch.from_numpy(z["input_features"]), torch.from_numpy(z["last_hidden_state"])


class RefWhisper(torch.nn.Module):
    """``whisper_forward`` behind the ``backbone=`` protocol of the encoders (``.config.hidden_size``, a waveform)"""

    def __init__(self, sd, cfg, dtype=torch.float32):
        super().__init__()
        self.sd, self.cfg, self.dtype = sd, cfg, dtype
        self.config = types.SimpleNamespace(hidden_size=cfg.d_model)

    def forward(self, waveform):
        with torch.no_grad():
            out = whisper_forward(self.sd, waveform.detach().cpu().numpy(), self.cfg, dtype=self.dtype).float()
        return types.SimpleNamespace(last_hidden_state=out.to(waveform.device))
