"""Whisper's encoder on the HIP kernels: 16 kHz waveforms (or HuggingFace's ``input_features``) -> frame states, frozen.

``NativeWhisperEncoder`` is HuggingFace's ``WhisperEncoder`` in eval mode rebuilt from its sizes alone, with HuggingFace's
``state_dict`` surface, and in front of it ``WhisperFeatureExtractor``'s log-mel spectrogram, which HuggingFace computes on the host
in numpy one clip at a time and this module computes on the device (``mmfusion.prep``'s position: what a decoder emits goes to the
GPU as it is, the kernels make the backbones' inputs).  The layer is the pre-LN block the other backbones share
(mmfusion/backbone.py); what is this model's own is the front end, csrc/whisper.hip.  With T = ``max_source_positions`` frames out
of Tm = 2 T mel frames of a window of ``n_samples`` = 320 T samples, the launch list of a chunk of ``n`` clips:

      log-mel -> conv1's window     mmf_whisper_logmel (two launches)    wave -> win (n Tm, Kw) bf16, Kw = 3 num_mel_bins
        (``input_features=``)       mmf_whisper_feature_window           features -> the same window, the same bits
      conv1                         mmf_gemm_grouped NT                  win x conv1.weight repacked to (d, Kw) -> raw (n Tm, d)
      + bias, GELU, conv2's window  mmf_whisper_gelu_window              raw -> win (n T, 3 d): kernel 3, stride 2, padding 1
      conv2                         mmf_gemm_grouped NT                  win x conv2.weight repacked to (d, 3 d) -> x (n T, d)
      + bias, GELU, + positions     mmf_whisper_stem_out (in place)      x: the residual stream's first value
      per layer                     FrozenBackbone._pre_ln_layer         (the plain fused attention; no key bias: the k third of the
                                                                          fused q/k/v bias is an internal zero)
      layer_norm                    mmf_layernorm_fwd_grouped            x -> ln
      result                        mmf_cast_bf16_to_f32                 ln -> last_hidden_state

A convolution over time with zero padding is one NT GEMM over a window form whose rows hold the kernel's three frames side by
side, zeros where a frame is outside the clip, so both convolutions run on the project's GEMM and nothing is transposed: the
activations are (time, channels) from the log-mel kernel's own store on.  The convolution weights are stored with their last two
dims swapped, (out, tap, in), which is the repacked operand itself.  Kw = 240 for 80 mel bins is a multiple of 8 but not of 32, so
conv1's GEMM is the general ring's.  Zero columns up to 256 would put it on the persistent kernel, which is 9 us a chunk faster at
whisper-small sizes and changes no bit, but the forward as a whole measured the same either way ("Whisper"), so
the operand stays as it is and no padded copy of the weight is kept.

The log-mel tables (the periodic Hann window, the 400-point DFT's cos | sin table, the Slaney filter bank) are made on the host in
float64, rounded to f32 once and kept per device (``_derived``); the device evaluates no sine or cosine, and its DFT is an
f32-input MFMA product, since speech spans 60 dB and bf16 operands lose every bin 25 dB under a frame's strongest.  The filter bank,
the window and ``sinusoids`` (``embed_positions``' initial value) are restated here; nothing imports transformers.

Frozen forward only.  Refused, each with an error that names ``NativeWhisperEncoder``: ``set_trainable_layers(k > 0)``, every
dropout and ``encoder_layerdrop`` above 0, ``apply_spec_augment``, an attention mask, ``activation_function`` other than "gelu", a
head_dim outside 64 / 96, a waveform longer than the window, the fp32 parity mode, CPU tensors.
"""
from __future__ import annotations

import math
import types
from typing import Optional

import numpy as np
import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BF16, BackboneOutput, FrozenBackbone, WsTable, _check_probability
from .lib import GEMM_NT

DEFAULT_CHUNK = 8
N_FFT, HOP, SAMPLE_RATE = 400, 160, 16000
DROPOUTS = ("dropout", "attention_dropout", "activation_dropout", "encoder_layerdrop")

# constructor kwargs of the released families over the defaults (whisper-small).  "large" is large-v3 (128 mel bins; v1 / v2 have
# 80: pass num_mel_bins=80): at d = 1280 the head_dim is 64 and the LayerNorm forward's chunk form takes the width
FAMILIES = {"tiny": dict(d_model=384, encoder_layers=4, encoder_attention_heads=6, encoder_ffn_dim=1536),
            "base": dict(d_model=512, encoder_layers=6, encoder_attention_heads=8, encoder_ffn_dim=2048),
            "small": dict(d_model=768, encoder_layers=12, encoder_attention_heads=12, encoder_ffn_dim=3072),
            "medium": dict(d_model=1024, encoder_layers=24, encoder_attention_heads=16, encoder_ffn_dim=4096),
            "large": dict(d_model=1280, encoder_layers=32, encoder_attention_heads=20, encoder_ffn_dim=5120, num_mel_bins=128)}


# ---- the tables, in float64 ---------------------------------------------------------------------------------------------
def hann_window(n: int = N_FFT) -> np.ndarray:
    """the periodic Hann window (``window_function(n, "hann")``)"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)


def mel_filter_bank(n_mels: int, n_bins: int = N_FFT // 2 + 1, f_max: float = 8000.0, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """(n_bins, n_mels) float64: triangular filters on the Slaney mel scale from 0 Hz to ``f_max`` with Slaney's area
    normalisation (``mel_filter_bank(norm="slaney", mel_scale="slaney")``)"""
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(f_max), n_mels + 2))
    bins = np.linspace(0.0, sample_rate // 2, n_bins)
    width = np.diff(edges)
    slopes = edges[None, :] - bins[:, None]
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / width[:-1], slopes[:, 2:] / width[1:]))
    return fb * (2.0 / (edges[2:n_mels + 2] - edges[:n_mels]))[None, :]


def dft_table() -> np.ndarray:
    """(400, 2 * 224) float64: cos(2 pi b k / 400) for the 201 bins b, zero columns up to 224, then sin likewise
    (``mmf_whisper_logmel``'s ``dft``).  The angle is reduced in integers first, so a large k b loses nothing before the cosine"""
    cols = lib.WHISPER_DFT_COLS
    k, b = np.arange(N_FFT)[:, None], np.arange(N_FFT // 2 + 1)[None, :]
    angle = 2.0 * np.pi * ((k * b) % N_FFT).astype(np.float64) / N_FFT
    out = np.zeros((N_FFT, 2 * cols), dtype=np.float64)
    out[:, :b.shape[1]], out[:, cols:cols + b.shape[1]] = np.cos(angle), np.sin(angle)
    return out


def sinusoids(length: int, channels: int, max_timescale: float = 10000.0) -> torch.Tensor:
    """HuggingFace's ``sinusoids``, operation for operation in float32: ``embed_positions``' value in a model built from sizes"""
    if channels % 2:
        raise ValueError(f"sinusoids: channels {channels} must be even")
    inc = math.log(max_timescale) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2))
    t = torch.arange(length).view(-1, 1) * inv.view(1, -1)
    return torch.cat([t.sin(), t.cos()], dim=1)


class NativeWhisperEncoder(FrozenBackbone):
    """HuggingFace ``WhisperEncoder`` (eval mode) behind ``WhisperFeatureExtractor``'s log-mel, defaults = whisper-small
    (``FAMILIES``).

    ``forward(waveform)``: (B, L) f32 at 16 kHz on the GPU, 1 <= L <= 320 ``max_source_positions``; a shorter clip is zero-padded
    to the window as the extractor pads it.  ``forward(input_features=...)``: (B, num_mel_bins, 2 ``max_source_positions``) f32,
    HuggingFace's features.  Exactly one of the two; both return ``.last_hidden_state`` (B, ``max_source_positions``, ``d_model``)
    f32.  ``features(waveform)`` returns HuggingFace's ``input_features``.  ``max_source_positions`` is an ordinary size (500: a
    10 s window).  ``state_dict()`` has the keys, shapes and order of ``WhisperEncoder``: q/k/v are stored fused and split on the
    way, ``k_proj`` has no bias."""

    def __init__(self, d_model: int = 768, encoder_layers: int = 12, encoder_attention_heads: int = 12, encoder_ffn_dim: int = 3072,
                 num_mel_bins: int = 80, max_source_positions: int = 1500, activation_function: str = "gelu", dropout: float = 0.0,
                 attention_dropout: float = 0.0, activation_dropout: float = 0.0, encoder_layerdrop: float = 0.0,
                 apply_spec_augment: bool = False, layer_norm_eps: float = 1e-5, chunk: int = DEFAULT_CHUNK):
        who = "NativeWhisperEncoder"
        d, H, I, T, M = int(d_model), int(encoder_attention_heads), int(encoder_ffn_dim), int(max_source_positions), int(num_mel_bins)
        if activation_function != "gelu":
            raise ValueError(f"{who}: activation_function={activation_function!r}: only the exact 'gelu' is built")
        super().__init__(d, H, chunk, ln_any_width=True)
        if M not in (80, 128):
            raise ValueError(f"{who}: num_mel_bins {M} must be 80 or 128 (the log-mel kernel's forms)")
        if T < 1 or encoder_layers < 1 or chunk < 1 or I < 8 or I % 8:
            raise ValueError(f"{who}: max_source_positions {T}, encoder_layers {encoder_layers} and chunk {chunk} at least 1, "
                             f"encoder_ffn_dim {I} a multiple of 8")
        self.config = types.SimpleNamespace(
            d_model=d, hidden_size=d, encoder_layers=int(encoder_layers), num_hidden_layers=int(encoder_layers),
            encoder_attention_heads=H, num_attention_heads=H, encoder_ffn_dim=I, intermediate_size=I, num_mel_bins=M,
            max_source_positions=T, activation_function="gelu", layer_norm_eps=float(layer_norm_eps), model_type="whisper",
            apply_spec_augment=False, **{n: 0.0 for n in DROPOUTS})
        self.set_regularisation(dropout=dropout, attention_dropout=attention_dropout, activation_dropout=activation_dropout,
                                encoder_layerdrop=encoder_layerdrop, apply_spec_augment=apply_spec_augment)
        self.n_samples, self.mel_frames = 2 * HOP * T, 2 * T
        self.kw = 3 * M                                        # conv1's K: the window form's row
        # the convolutions' weights as the GEMMs read them: (out, tap, in), HuggingFace's (out, in, tap) with the last two dims swapped
        self._add("conv1_w", (d, 3, M), "conv1.weight", swapped=True, std=(3 * M) ** -0.5)
        self._add("conv1_b", (d,), "conv1.bias", std=0.0)
        self._add("conv2_w", (d, 3, d), "conv2.weight", swapped=True, std=(3 * d) ** -0.5)
        self._add("conv2_b", (d,), "conv2.bias", std=0.0)
        self._add("pos_emb", (T, d), "embed_positions.weight")
        with torch.no_grad():
            self.pos_emb.copy_(sinusoids(T, d))
        for i in range(encoder_layers):
            a = f"layers.{i}."
            self._add_layer(i, d, I, {"k": a + "self_attn.k_proj", "v": a + "self_attn.v_proj", "q": a + "self_attn.q_proj",
                                      "o": a + "self_attn.out_proj", "ln1": a + "self_attn_layer_norm", "fc1": a + "fc1",
                                      "fc2": a + "fc2", "ln2": a + "final_layer_norm"})
            del self._hf[a + "self_attn.k_proj.bias"]          # HuggingFace's k_proj has none: that third of the fused bias stays zero
        self._add("ln_f_w", (d,), "layer_norm.weight", ones=True)
        self._add("ln_f_b", (d,), "layer_norm.bias", std=0.0)

    # -- frozen only ------------------------------------------------------------------------------------------
    def set_trainable_layers(self, k: int, front: bool = False, feature_encoder: bool = False) -> None:
        """0 only: a frozen backbone (no backward of the stem is built)"""
        if isinstance(k, bool) or k != 0 or front or feature_encoder:
            raise ValueError(f"NativeWhisperEncoder: set_trainable_layers({k!r}, front={front!r}, feature_encoder={feature_encoder!r}): "
                             "the backbone is frozen; no backward of the log-mel front end and the convolution stem is built yet")
        self._trainable = 0
        self._require_grad(())

    def set_regularisation(self, **settings) -> None:
        """every setting must stay 0 / False: the dropouts, LayerDrop and SpecAugment act in a training call, which this frozen model
        has none of.  Takes ``WhisperConfig``'s names; other names (another audio backbone's regularisers) must be 0 as well"""
        who = "NativeWhisperEncoder: set_regularisation"
        for name, p in settings.items():
            if isinstance(p, bool) or name == "apply_spec_augment":
                if p:
                    raise ValueError(f"{who}({name}={p!r}): not built for this frozen backbone; it stays off")
            elif name in DROPOUTS:
                _check_probability(who, name, p)
                if p != 0:
                    raise ValueError(f"{who}({name}={p!r}): training-mode regularisers are not built for this frozen backbone; it stays at 0")
            elif name not in ("mask_time_length", "mask_time_min_masks") and p != 0:
                raise ValueError(f"{who}({name}={p!r}): training-mode regularisers are not built for this frozen backbone; it stays at 0")

    # -- shapes / workspace -----------------------------------------------------------------------------
    def _ws_table(self, size=None) -> WsTable:
        """per clip (the window is the model's own size)"""
        c = self.config
        T, Tm, d, M = c.max_source_positions, self.mel_frames, c.d_model, c.num_mel_bins
        mel = lib.whisper_logmel_scratch_bytes(1, self.n_samples, M) // 4
        return [("win", max(Tm * self.kw, T * 3 * d), BF16), ("raw", Tm * d, BF16), ("mel", mel, torch.float32)] \
            + self._token_table(T, T * c.intermediate_size)

    def workspace_bytes_per_clip(self) -> int:
        return self._bytes_per_item(self._ws_table())

    # -- what is derived ---------------------------------------------------------------------------------------
    def _tables(self, dev) -> tuple:
        """(window [400], dft (400, 448), filter bank (201, num_mel_bins)) f32 on ``dev``: float64 on the host, rounded once"""
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dev)
        return self._derived(f"logmel_tables_{dev}", (), lambda: (f32(hann_window()), f32(dft_table()), f32(mel_filter_bank(self.config.num_mel_bins))))

    # -- launches ---------------------------------------------------------------------------------------
    def _check_wave(self, waveform) -> torch.Tensor:
        who = "NativeWhisperEncoder"
        self._check_input(waveform, "waveform")
        if waveform.dim() != 2 or waveform.shape[0] < 1:
            raise ValueError(f"{who}: waveform {tuple(waveform.shape)} is not (B, L)")
        if not 1 <= waveform.shape[1] <= self.n_samples:
            raise ValueError(f"{who}: {waveform.shape[1]} samples: 1 .. {self.n_samples} (the window of max_source_positions "
                             f"{self.config.max_source_positions}: 320 samples a position); cut longer audio into windows")
        return waveform.detach().contiguous()

    def features(self, waveform: torch.Tensor) -> torch.Tensor:
        """HuggingFace's ``input_features`` of ``waveform`` (B, L): (B, num_mel_bins, 2 max_source_positions) f32"""
        wave = self._check_wave(waveform)
        dev = wave.device
        ws = self._workspace(dev)
        out = torch.empty((wave.shape[0], self.config.num_mel_bins, self.mel_frames), dtype=torch.float32, device=dev)
        for n0, n in self._chunks(wave.shape[0]):
            lib.whisper_logmel(wave[n0:n0 + n], *self._tables(dev), ws["mel"], self.n_samples, features=out[n0:n0 + n])
        return out

    def forward(self, waveform: Optional[torch.Tensor] = None, attention_mask=None, input_features: Optional[torch.Tensor] = None) -> BackboneOutput:
        who, c = "NativeWhisperEncoder", self.config
        if attention_mask is not None:
            raise NotImplementedError(f"{who}: attention_mask is not implemented (Whisper's encoder attends over the whole window)")
        if (waveform is None) == (input_features is None):
            raise ValueError(f"{who}: exactly one of waveform / input_features")
        if waveform is not None:
            src, by_wave = self._check_wave(waveform), True
        else:
            self._check_input(input_features, "input_features")
            want = (c.num_mel_bins, self.mel_frames)
            if input_features.dim() != 3 or tuple(input_features.shape[1:]) != want or input_features.shape[0] < 1:
                raise ValueError(f"{who}: input_features {tuple(input_features.shape)} is not (B, num_mel_bins, 2 max_source_positions) "
                                 f"= (B, {want[0]}, {want[1]})")
            src, by_wave = input_features.detach().contiguous(), False
        _arena.ensure(self)
        with torch.no_grad():
            return BackboneOutput(self._run(src, by_wave))

    def _run(self, src: torch.Tensor, by_wave: bool) -> torch.Tensor:
        """the launch list on checked inputs -> (N, T, d) f32"""
        c, dev, N = self.config, src.device, src.shape[0]
        T, Tm, d, Kw = c.max_source_positions, self.mel_frames, c.d_model, self.kw
        ws = self._workspace(dev)
        out = torch.empty((N, T, d), dtype=torch.float32, device=dev)
        w1, w2 = self._w("conv1_w").view(d, Kw), self._w("conv2_w").view(d, 3 * d)
        for n0, n in self._chunks(N):
            win1 = ws["win"][:n * Tm * Kw].view(n, Tm, Kw)
            if by_wave:
                lib.whisper_logmel(src[n0:n0 + n], *self._tables(dev), ws["mel"], self.n_samples, out_window=win1)
            else:
                lib.whisper_feature_window(src[n0:n0 + n], win1)
            raw, x, ln = self._rows(ws, "raw", n * Tm, d), self._rows(ws, "x", n * T, d), self._rows(ws, "ln", n * T, d)
            ops.gemm(GEMM_NT, win1.view(n * Tm, Kw), w1, raw)
            lib.whisper_gelu_window(raw, self._f("conv1_b"), ws["win"][:n * T * 3 * d], n, Tm, d, 3, 2, 1)
            ops.gemm(GEMM_NT, self._rows(ws, "win", n * T, 3 * d), w2, x)
            lib.whisper_stem_out(x, self._f("conv2_b"), self._f("pos_emb"), x, T)
            for i in range(c.num_hidden_layers):
                self._pre_ln_layer(i, ws, n, T)
            self._ln(ws, x, ln, "ln_f_w", "ln_f_b")
            self._widen(ln, out[n0:n0 + n])
        return out
