"""Frozen Wav2Vec2 backbone on the HIP kernels: waveforms -> frame states, forward only.

The reference pushes every clip through HuggingFace's ``Wav2Vec2Model`` per step (reference models/encoders.py:116,144).
``NativeWav2Vec2`` is that model rebuilt from its sizes alone (nothing is fetched), with HuggingFace's ``state_dict``
surface, so published checkpoints and the reference's ``.pth`` files load.  Only the base family is built: group-norm
feature extractor without conv biases, post-LN encoder.

Activations are channel-last ``(time, channels)`` bf16, so a convolution over time is one GEMM over a window form and the
transformer needs no transpose.  Launch list for a chunk of ``n`` clips (the layer's two blocks: mmfusion/backbone.py):

    conv layer 0 statistics       mmf_w2v_conv0_stats                  wave -> mean / variance per (clip, channel)
    conv 0 + GroupNorm + GELU     mmf_w2v_conv0_norm_gelu              wave -> window form of layer 1
    conv layer i >= 1             mmf_gemm_grouped NT                  window (n T_i, k_i C_{i-1}) -> raw (n T_i, C_i)
    GELU + next window            mmf_w2v_gelu_window                  raw -> window form of layer i + 1
    GELU after the last layer     mmf_bias_gelu_bf16 (no bias)         raw, in place
    LayerNorm(conv_dim)           mmf_layernorm_fwd_grouped
    projection + bias             mmf_gemm_grouped NT, BIAS            -> x (n T, hidden)
    x + gelu(pos_conv(x) + b)     mmf_w2v_posconv                      x -> y
    LayerNorm                                                          y -> x
    per post-LN layer:
      _attention(x, + x)                                               x  -> qkv -> att -> y
      LayerNorm                                                        y  -> ln
      _ffn(ln, + ln)                                                   ln -> h -> y
      LayerNorm                                                        y  -> x
    widening cast                 mmf_cast_bf16_to_f32                 x  -> result

Clips are processed in chunks of ``chunk`` through one workspace sized by the chunk and the longest waveform seen so far
(a longer one reallocates it once; shorter ones use its leading part).  Forward only, frozen, bf16 storage only, nothing
synchronises with the host (mmfusion/backbone.py).
"""
from __future__ import annotations

import types
from typing import Dict, List, Sequence, Tuple

import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BF16, BackboneOutput, FrozenBackbone, WsTable
from .lib import EPI_BIAS, GEMM_NT

# clips per pass through the workspace.  NOT chosen by measurement yet: 8 clips keep the workspace at 0.57 GB for 10 s clips
# and give the layer GEMMs 3992 rows; tools/w2v_bench.py --chunks is the sweep that should decide it
DEFAULT_CHUNK = 16
POS_GROUP_WIDTHS = (16, 32, 48, 64)        # the forms of mmf_w2v_posconv

_WN = "encoder.pos_conv_embed.conv."
_WN_NEW = (_WN + "parametrizations.weight.original0", _WN + "parametrizations.weight.original1")
_WN_OLD = (_WN + "weight_g", _WN + "weight_v")
_WN_TO_NEW = dict(zip(_WN_OLD, _WN_NEW))
_WN_TO_OLD = dict(zip(_WN_NEW, _WN_OLD))


def feat_lengths(L: int, kernels: Sequence[int], strides: Sequence[int]) -> List[int]:
    """frames after each feature-extractor layer (HuggingFace's ``_get_feat_extract_output_lengths``); 0 once too short"""
    out = []
    for k, s in zip(kernels, strides):
        L = (L - k) // s + 1 if L >= k else 0
        out.append(L)
    return out


class NativeWav2Vec2(FrozenBackbone):
    """HuggingFace ``Wav2Vec2Model`` (inference, no mask), defaults = wav2vec2-base.

    ``forward(input_values)`` -> ``.last_hidden_state`` (N, T, hidden) f32; ``input_values``: (N, L) f32 on the GPU.
    ``state_dict()`` has the keys, shapes and order of ``Wav2Vec2Model``; ``load_state_dict`` also takes the older weight-norm
    names (``weight_g`` / ``weight_v``).  Q/K/V are stored fused, the inner conv weights as ``(C_out, k, C_in)`` (the GEMM's
    operand), and split / permuted on the way.  ``masked_spec_embed`` is kept as an unused parameter."""

    def __init__(self, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, conv_dim: Sequence[int] = (512,) * 7,
                 conv_kernel: Sequence[int] = (10, 3, 3, 3, 3, 2, 2), conv_stride: Sequence[int] = (5, 2, 2, 2, 2, 2, 2),
                 conv_bias: bool = False, num_conv_pos_embeddings: int = 128, num_conv_pos_embedding_groups: int = 16,
                 layer_norm_eps: float = 1e-5, feat_extract_norm: str = "group", do_stable_layer_norm: bool = False,
                 in_channels: int = 1, chunk: int = DEFAULT_CHUNK):
        d, H, I = int(hidden_size), int(num_attention_heads), int(intermediate_size)
        dims, ks, ss = tuple(int(v) for v in conv_dim), tuple(int(v) for v in conv_kernel), tuple(int(v) for v in conv_stride)
        pk, pg = int(num_conv_pos_embeddings), int(num_conv_pos_embedding_groups)
        who = "NativeWav2Vec2"
        if feat_extract_norm != "group":
            raise ValueError(f"{who}: feat_extract_norm={feat_extract_norm!r}: only the 'group' (base) family is built")
        if do_stable_layer_norm:
            raise ValueError(f"{who}: do_stable_layer_norm=True (the large-lv60 family) is not built")
        if conv_bias:
            raise ValueError(f"{who}: conv_bias=True is not built (the base family has no conv biases)")
        if not (len(dims) == len(ks) == len(ss)) or len(dims) < 2 or min(dims + ks + ss) < 1:
            raise ValueError(f"{who}: conv_dim, conv_kernel and conv_stride must be positive and of one length of at least 2")
        super().__init__(d, H, chunk, ln_widths={"conv_dim[-1]": dims[-1]})
        if in_channels != 1:
            raise ValueError(f"{who}: the first conv layer takes one input channel (a waveform), not {in_channels}")
        if ks[0] > 16 or dims[0] > 2048:
            raise ValueError(f"{who}: layer 0 with kernel {ks[0]} (at most 16) / {dims[0]} channels (at most 2048) has no kernel form")
        for i in range(1, len(dims)):
            if (dims[i - 1] * ks[i]) % 32 or ks[i] < ss[i]:
                raise ValueError(f"{who}: conv layer {i}: C_in * kernel = {dims[i - 1]} * {ks[i]} must be a multiple of 32 and kernel >= "
                                 f"stride {ss[i]} (the window form would skip frames)")
        if pg < 1 or d % pg:
            raise ValueError(f"{who}: hidden_size {d} is not a multiple of num_conv_pos_embedding_groups {pg}")
        cg = d // pg
        if any(c % 8 for c in dims) or I % 8 or cg % 8:
            raise ValueError(f"{who}: conv_dim {dims}, intermediate_size {I} and the positional group width {cg} must be multiples of 8")
        kp = (pk * cg + 31) // 32 * 32
        if cg not in POS_GROUP_WIDTHS or pk < 1 or (127 * cg + kp) * 2 > 65536:
            raise ValueError(f"{who}: positional convolution with group width {cg} (one of {POS_GROUP_WIDTHS}) and kernel {pk} has no "
                             "kernel form (its LDS image must fit 64 KiB)")
        if num_hidden_layers < 1 or chunk < 1:
            raise ValueError(f"{who}: layers and chunk at least 1")
        self.config = types.SimpleNamespace(
            hidden_size=d, num_hidden_layers=int(num_hidden_layers), num_attention_heads=H, intermediate_size=I, conv_dim=dims,
            conv_kernel=ks, conv_stride=ss, conv_bias=False, num_conv_pos_embeddings=pk, num_conv_pos_embedding_groups=pg,
            layer_norm_eps=float(layer_norm_eps), feat_extract_norm="group", do_stable_layer_norm=False, hidden_act="gelu",
            feat_extract_activation="gelu", num_feat_extract_layers=len(dims), model_type="wav2vec2")
        self.pos_cg, self.pos_kp = cg, kp
        add = self._add
        add("masked_spec_embed", (d,), "masked_spec_embed", std=1.0)
        fe = "feature_extractor.conv_layers."
        add("conv0_w", (dims[0], 1, ks[0]), fe + "0.conv.weight", std=0.3)
        add("conv0_gn_w", (dims[0],), fe + "0.layer_norm.weight", ones=True)
        add("conv0_gn_b", (dims[0],), fe + "0.layer_norm.bias", std=0.0)
        for i in range(1, len(dims)):
            add(f"conv{i}_w", (dims[i], ks[i], dims[i - 1]), f"{fe}{i}.conv.weight", std=(dims[i - 1] * ks[i]) ** -0.5, swapped=True)
        add("fp_ln_w", (dims[-1],), "feature_projection.layer_norm.weight", ones=True)
        add("fp_ln_b", (dims[-1],), "feature_projection.layer_norm.bias", std=0.0)
        add("fp_w", (d, dims[-1]), "feature_projection.projection.weight")
        add("fp_b", (d,), "feature_projection.projection.bias", std=0.0)
        add("pos_b", (d,), _WN + "bias", std=0.0)
        add("pos_g", (1, 1, pk), _WN_NEW[0], ones=True)
        add("pos_v", (d, cg, pk), _WN_NEW[1], std=(cg * pk) ** -0.5)
        with torch.no_grad():
            self.pos_g.copy_(self.pos_v.norm(dim=(0, 1), keepdim=True))        # weight_norm's start: the effective weight is v
        add("enc_ln_w", (d,), "encoder.layer_norm.weight", ones=True)
        add("enc_ln_b", (d,), "encoder.layer_norm.bias", std=0.0)
        for i in range(num_hidden_layers):
            a = f"encoder.layers.{i}."
            self._add_layer(i, d, I, {"k": a + "attention.k_proj", "v": a + "attention.v_proj", "q": a + "attention.q_proj",
                                      "o": a + "attention.out_proj", "ln1": a + "layer_norm", "fc1": a + "feed_forward.intermediate_dense",
                                      "fc2": a + "feed_forward.output_dense", "ln2": a + "final_layer_norm"})

    # -- HuggingFace state_dict surface ----------------------------------------------------------------
    def _canonical_key(self, key: str) -> str:
        return _WN_TO_NEW.get(key, key)

    def hf_state_dict(self, legacy_weight_norm: bool = False) -> Dict[str, torch.Tensor]:
        """``state_dict()`` with the positional convolution's weight norm spelled as current torch does
        (``parametrizations.weight.original0`` / ``original1``, the default surface) or the older ``weight_g`` / ``weight_v``."""
        sd = self.state_dict()
        return {_WN_TO_OLD.get(k, k): v for k, v in sd.items()} if legacy_weight_norm else sd

    # -- shapes / workspace -----------------------------------------------------------------------------
    def frames(self, L: int) -> int:
        """T for a waveform of L samples (0 when L is shorter than the receptive field)"""
        return feat_lengths(int(L), self.config.conv_kernel, self.config.conv_stride)[-1]

    def _conv_elements(self, L: int) -> Tuple[int, int]:
        c = self.config
        Ts = feat_lengths(L, c.conv_kernel, c.conv_stride)
        n = len(Ts)
        win = max(Ts[i] * c.conv_kernel[i] * c.conv_dim[i - 1] for i in range(1, n))
        win = max(win, Ts[-1] * c.conv_dim[-1])              # the feature LayerNorm's output takes the window buffer's place
        raw = max(Ts[i] * c.conv_dim[i] for i in range(1, n))
        return win, raw

    def _ws_table(self, L: int) -> WsTable:
        """per clip of ``L`` samples"""
        c, T = self.config, self.frames(L)
        win, raw = self._conv_elements(L)
        return [("win", win, BF16), ("raw", raw, BF16)] + self._token_table(T, T * c.intermediate_size) \
            + [("stats", 2 * c.conv_dim[0], torch.float32), ("partial", lib.W2V_STATS_SLOTS * 2 * c.conv_dim[0], torch.float32)]

    def workspace_bytes_per_clip(self, L: int) -> int:
        return self._bytes_per_item(self._ws_table(L))

    # -- weights ----------------------------------------------------------------------------------------
    def _pos_weight(self) -> torch.Tensor:
        """The positional convolution's effective weight g v / ||v|| (norm over dims (0, 1) per tap, ``weight_norm(dim=2)``),
        folded in f32, repacked to (groups, cg, Kp) column (tap, channel) and rounded to bf16 once per weight version."""
        def build():
            g, v = self._f("pos_g"), self._f("pos_v")
            w = g * v / v.norm(dim=(0, 1), keepdim=True)                                          # (C, cg, k)
            C, cg, k = w.shape
            packed = torch.zeros(C, self.pos_kp, dtype=BF16, device=w.device)
            packed[:, :k * cg] = w.permute(0, 2, 1).reshape(C, k * cg).to(BF16)
            return packed
        return self._derived("pos_w16", ("pos_g", "pos_v"), build)

    # -- launches ---------------------------------------------------------------------------------------
    def _features(self, ws, wave: torch.Tensor, n: int, Ts: List[int]) -> torch.Tensor:
        """the feature extractor: wave (n, L) f32 -> (n * T, conv_dim[-1]) bf16 after the last layer's GELU"""
        c = self.config
        dims, ks, ss = c.conv_dim, c.conv_kernel, c.conv_stride
        w0 = self._f("conv0_w")
        lib.w2v_conv0_stats(wave, w0, ws["stats"], ws["partial"], ks[0], ss[0])
        lib.w2v_conv0_norm_gelu(wave, w0, ws["stats"], self._f("conv0_gn_w"), self._f("conv0_gn_b"), ws["win"], ks[0], ss[0],
                                ks[1], ss[1], 1e-5)                                   # (nn.GroupNorm's own eps, not layer_norm_eps)
        last = len(dims) - 1
        for i in range(1, last + 1):
            rows, K = n * Ts[i], ks[i] * dims[i - 1]
            win, raw = self._rows(ws, "win", rows, K), self._rows(ws, "raw", rows, dims[i])
            ops.gemm(GEMM_NT, win, self._w(f"conv{i}_w").view(dims[i], K), raw)
            if i < last:
                lib.w2v_gelu_window(ws["raw"], ws["win"], n, Ts[i], dims[i], ks[i + 1], ss[i + 1])
            else:
                lib.bias_gelu(raw)
        return raw

    def forward(self, input_values: torch.Tensor, attention_mask=None) -> BackboneOutput:
        c = self.config
        if attention_mask is not None:
            raise NotImplementedError("NativeWav2Vec2: attention_mask is not implemented (the reference never passes one)")
        self._check_input(input_values, "input_values")
        if input_values.dim() != 2:
            raise ValueError(f"NativeWav2Vec2: input_values {tuple(input_values.shape)} is not (N, L)")
        N, L = input_values.shape
        Ts = feat_lengths(L, c.conv_kernel, c.conv_stride)
        T, d = Ts[-1], c.hidden_size
        if T < 1:
            raise ValueError(f"NativeWav2Vec2: {L} samples are shorter than the feature extractor's receptive field")
        wave = input_values.contiguous()
        _arena.ensure(self)
        pos_w = self._pos_weight()
        ws = self._workspace(wave.device, L)
        out = torch.empty((N, T, d), dtype=torch.float32, device=wave.device)
        for n0 in range(0, N, self.chunk):
            n = min(self.chunk, N - n0)
            rows = n * T
            feat = self._features(ws, wave[n0:n0 + n], n, Ts)
            x, y = self._rows(ws, "x", rows, d), self._rows(ws, "y", rows, d)
            fln = self._rows(ws, "win", rows, feat.shape[1])
            self._ln(ws, feat, fln, "fp_ln_w", "fp_ln_b")
            ops.gemm(GEMM_NT, fln, self._w("fp_w"), x, bias=self._f("fp_b"), epilogue=EPI_BIAS)
            lib.w2v_posconv(x, pos_w, self._f("pos_b"), y, n, T, d, c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings)
            self._ln(ws, y, x, "enc_ln_w", "enc_ln_b")
            for i in range(c.num_hidden_layers):
                self._post_ln_layer(i, ws, n, T)
            self._widen(x, out[n0:n0 + n])
        return BackboneOutput(out)
