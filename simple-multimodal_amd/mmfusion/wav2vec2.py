"""Frozen Wav2Vec2 backbone on the HIP kernels: waveforms -> frame states, forward only.

The reference pushes every clip through HuggingFace's ``Wav2Vec2Model`` per step (reference models/encoders.py:116,144).
``NativeWav2Vec2`` is that model rebuilt from its sizes alone (nothing is fetched), with HuggingFace's ``state_dict``
surface, so published checkpoints and the reference's ``.pth`` files load.  Only the base family is built: group-norm
feature extractor without conv biases, post-LN encoder.

Activations are channel-last ``(time, channels)`` bf16, so a convolution over time is one GEMM over a window form and the
transformer needs no transpose.  Launch list for a chunk of ``n`` clips:

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
      fused Q/K/V linear + bias   mmf_gemm_grouped NT, BIAS            x   -> qkv
      attention                   mmf_attn_fwd_grouped                 qkv -> att
      out-projection + bias + x   mmf_gemm_grouped NT, BIAS | ADD_AUX  att -> y
      LayerNorm                                                        y   -> ln
      fc1                         mmf_gemm_grouped NT                  ln  -> h
      + bias, exact GELU          mmf_bias_gelu_bf16 (in place)        h
      fc2 + bias + ln             mmf_gemm_grouped NT, BIAS | ADD_AUX  h   -> y
      LayerNorm                                                        y   -> x
    widening cast                 mmf_cast_bf16_to_f32                 x   -> result

Clips are processed in chunks of ``chunk`` through one workspace sized by the chunk and the longest waveform seen so far
(a longer one reallocates it once; shorter ones use its leading part).  Nothing synchronises
with the host: a fixed-shape call can be captured by ``torch.cuda.graph``.  Forward only and frozen; bf16 storage only: in
the fp32 parity mode (``ops.fp32_mode()``) the forward raises instead of computing something else.
"""
from __future__ import annotations

import types
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import arena as _arena
from . import lib, ops
from .lib import EPI_ADD_AUX, EPI_BIAS, GEMM_NT, AttnProblem, LnProblem

BF16 = torch.bfloat16
# clips per pass through the workspace.  NOT chosen by measurement yet: 8 clips keep the workspace at 0.57 GB for 10 s clips
# and give the layer GEMMs 3992 rows; tools/w2v_bench.py --chunks is the sweep that should decide it
DEFAULT_CHUNK = 16
LN_WIDTHS = (256, 512, 768, 1024)          # the lane forms of layernorm.hip
POS_GROUP_WIDTHS = (16, 32, 48, 64)        # the forms of mmf_w2v_posconv

_WN = "encoder.pos_conv_embed.conv."
_WN_NEW = (_WN + "parametrizations.weight.original0", _WN + "parametrizations.weight.original1")
_WN_OLD = (_WN + "weight_g", _WN + "weight_v")
_WN_TO_NEW = dict(zip(_WN_OLD, _WN_NEW))
_WN_TO_OLD = dict(zip(_WN_NEW, _WN_OLD))


class Wav2Vec2Output:
    """What the encoders read from a backbone's result."""

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state


def feat_lengths(L: int, kernels: Sequence[int], strides: Sequence[int]) -> List[int]:
    """frames after each feature-extractor layer (HuggingFace's ``_get_feat_extract_output_lengths``); 0 once too short"""
    out = []
    for k, s in zip(kernels, strides):
        L = (L - k) // s + 1 if L >= k else 0
        out.append(L)
    return out


class NativeWav2Vec2(nn.Module):
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
        super().__init__()
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
        if H <= 0 or d % H or d // H not in (64, 96):
            raise ValueError(f"{who}: hidden_size {d} / num_attention_heads {H} must give a head_dim of 64 or 96 "
                             "(the fused attention kernel's forms)")
        if not (len(dims) == len(ks) == len(ss)) or len(dims) < 2 or min(dims + ks + ss) < 1:
            raise ValueError(f"{who}: conv_dim, conv_kernel and conv_stride must be positive and of one length of at least 2")
        if d not in LN_WIDTHS or dims[-1] not in LN_WIDTHS:
            raise ValueError(f"{who}: hidden_size {d} and conv_dim[-1] {dims[-1]} must be among the LayerNorm kernel's widths {LN_WIDTHS}")
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
        self.chunk = int(chunk)
        self.head_dim, self.pos_cg, self.pos_kp = d // H, cg, kp
        # HuggingFace key -> (parameter, row range | None, stored with the last two dims swapped)
        self._hf: Dict[str, Tuple[str, Optional[Tuple[int, int]], bool]] = {}

        def add(name: str, shape, key: Optional[str], ones: bool = False, std: float = 0.02, swapped: bool = False):
            p = nn.Parameter(torch.empty(shape), requires_grad=False)
            if ones:
                nn.init.ones_(p)
            elif std > 0:
                nn.init.normal_(p, std=std)
            else:
                nn.init.zeros_(p)
            self.register_parameter(name, p)
            if key is not None:
                self._hf[key] = (name, None, swapped)

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
            # HuggingFace's order inside a layer: k, v, q, out_proj, layer_norm, intermediate, output, final_layer_norm
            for n, r in (("k", (d, 2 * d)), ("v", (2 * d, 3 * d)), ("q", (0, d))):
                self._hf[f"{a}attention.{n}_proj.weight"] = (f"l{i}_qkv_w", r, False)
                self._hf[f"{a}attention.{n}_proj.bias"] = (f"l{i}_qkv_b", r, False)
            add(f"l{i}_qkv_w", (3 * d, d), None)
            add(f"l{i}_qkv_b", (3 * d,), None, std=0.0)
            add(f"l{i}_o_w", (d, d), a + "attention.out_proj.weight")
            add(f"l{i}_o_b", (d,), a + "attention.out_proj.bias", std=0.0)
            add(f"l{i}_ln1_w", (d,), a + "layer_norm.weight", ones=True)
            add(f"l{i}_ln1_b", (d,), a + "layer_norm.bias", std=0.0)
            add(f"l{i}_fc1_w", (I, d), a + "feed_forward.intermediate_dense.weight")
            add(f"l{i}_fc1_b", (I,), a + "feed_forward.intermediate_dense.bias", std=0.0)
            add(f"l{i}_fc2_w", (d, I), a + "feed_forward.output_dense.weight")
            add(f"l{i}_fc2_b", (d,), a + "feed_forward.output_dense.bias", std=0.0)
            add(f"l{i}_ln2_w", (d,), a + "final_layer_norm.weight", ones=True)
            add(f"l{i}_ln2_b", (d,), a + "final_layer_norm.bias", std=0.0)
        self._ws: Optional[dict] = None
        self._pos_w16: Optional[torch.Tensor] = None
        self._pos_stamp = None

    # -- HuggingFace state_dict surface ----------------------------------------------------------------
    def _view(self, name: str, rows, swapped: bool, keep_vars: bool = False) -> torch.Tensor:
        p = getattr(self, name)
        t = p if keep_vars else p.detach()
        if rows is not None:
            t = t[rows[0]:rows[1]]
        return t.permute(0, 2, 1) if swapped else t

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for key, (name, rows, swapped) in self._hf.items():
            destination[prefix + key] = self._view(name, rows, swapped, keep_vars)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        found = {}
        for key in list(state_dict.keys()):
            if not key.startswith(prefix):
                continue
            k = _WN_TO_NEW.get(key[len(prefix):], key[len(prefix):])
            if k in self._hf:
                found[k] = state_dict[key]
            elif strict:
                unexpected_keys.append(key)
        with torch.no_grad():
            for k, (name, rows, swapped) in self._hf.items():
                if k not in found:
                    missing_keys.append(prefix + k)
                    continue
                dst, src = self._view(name, rows, swapped), found[k]
                if tuple(src.shape) != tuple(dst.shape):
                    error_msgs.append(f"size mismatch for {prefix + k}: copying a param with shape {tuple(src.shape)} from "
                                      f"checkpoint, the shape in current model is {tuple(dst.shape)}.")
                    continue
                dst.copy_(src)                 # in place: the version counter moves, so the shadow is re-cast and the weight norm re-folded

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

    def workspace_bytes_per_clip(self, L: int) -> int:
        c = self.config
        T, d = self.frames(L), c.hidden_size
        win, raw = self._conv_elements(L)
        return 2 * (win + raw + T * (4 * d + 3 * d + c.intermediate_size)) \
            + 4 * (2 * T + c.num_attention_heads * T + (2 + 2 * lib.W2V_STATS_SLOTS) * c.conv_dim[0])

    def _workspace(self, dev, L: int) -> dict:
        ws = self._ws
        if ws is not None and ws["dev"] == dev and ws["chunk"] == self.chunk and ws["L"] >= L:
            return ws                                        # every buffer grows with L: a shorter clip uses the leading part
        c, n, d = self.config, self.chunk, self.config.hidden_size
        rows = n * self.frames(L)
        win, raw = self._conv_elements(L)

        def buf(numel, dtype=BF16):
            return torch.empty(numel, dtype=dtype, device=dev)
        ws = {"dev": dev, "chunk": n, "L": L, "win": buf(n * win), "raw": buf(n * raw), "x": buf(rows * d), "y": buf(rows * d),
              "ln": buf(rows * d), "att": buf(rows * d), "qkv": buf(rows * 3 * d), "h": buf(rows * c.intermediate_size),
              "mean": buf(rows, torch.float32), "rstd": buf(rows, torch.float32),
              "lse": buf(rows * c.num_attention_heads, torch.float32), "stats": buf(n * 2 * c.conv_dim[0], torch.float32),
              "partial": buf(n * lib.W2V_STATS_SLOTS * 2 * c.conv_dim[0], torch.float32)}
        self._ws = ws
        return ws

    # -- weights ----------------------------------------------------------------------------------------
    def _w(self, name: str) -> torch.Tensor:
        return ops.shadow(getattr(self, name))

    def _f(self, name: str) -> torch.Tensor:
        return getattr(self, name).detach()

    def _pos_weight(self) -> torch.Tensor:
        """The positional convolution's effective weight g v / ||v|| (norm over dims (0, 1) per tap, ``weight_norm(dim=2)``),
        folded in f32, repacked to (groups, cg, Kp) column (tap, channel) and rounded to bf16 once per weight version."""
        g, v = self.pos_g, self.pos_v
        stamp = (g.data_ptr(), g._version, v.data_ptr(), v._version)
        if self._pos_w16 is None or stamp != self._pos_stamp:
            with torch.no_grad():
                w = g.detach() * v.detach() / v.detach().norm(dim=(0, 1), keepdim=True)          # (C, cg, k)
                C, cg, k = w.shape
                packed = torch.zeros(C, self.pos_kp, dtype=BF16, device=w.device)
                packed[:, :k * cg] = w.permute(0, 2, 1).reshape(C, k * cg).to(BF16)
            self._pos_w16, self._pos_stamp = packed, stamp
        return self._pos_w16

    # -- launches ---------------------------------------------------------------------------------------
    def _ln(self, ws, src: torch.Tensor, dst: torch.Tensor, gamma: str, beta: str) -> None:
        rows, width = src.shape
        with lib._Timed("ln_fwd_kernel", 0.0, [(rows, width)]):
            lib.layernorm_fwd_grouped([LnProblem(src.data_ptr(), dst.data_ptr(), self._f(gamma).data_ptr(), self._f(beta).data_ptr(),
                                                 ws["mean"].data_ptr(), ws["rstd"].data_ptr(), None, None, None, None, rows)],
                                      width, self.config.layer_norm_eps)

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
            win = ws["win"][:rows * K].view(rows, K)
            raw = ws["raw"][:rows * dims[i]].view(rows, dims[i])
            ops.gemm(GEMM_NT, win, self._w(f"conv{i}_w").view(dims[i], K), raw)
            if i < last:
                lib.w2v_gelu_window(ws["raw"], ws["win"], n, Ts[i], dims[i], ks[i + 1], ss[i + 1])
            else:
                lib.bias_gelu(raw)
        return raw

    def _layer(self, i: int, ws, n: int, T: int) -> None:
        c, d, I = self.config, self.config.hidden_size, self.config.intermediate_size
        rows = n * T
        x, y, ln, att = (ws[k][:rows * d].view(rows, d) for k in ("x", "y", "ln", "att"))
        qkv, h = ws["qkv"][:rows * 3 * d].view(rows, 3 * d), ws["h"][:rows * I].view(rows, I)
        ops.gemm(GEMM_NT, x, self._w(f"l{i}_qkv_w"), qkv, bias=self._f(f"l{i}_qkv_b"), epilogue=EPI_BIAS)
        base = qkv.data_ptr()
        lib.attn_fwd_grouped([AttnProblem(base, base + 2 * d, base + 4 * d, att.data_ptr(), ws["lse"].data_ptr(), None, None, None,
                                          None, None, n, c.num_attention_heads, T, T, 3 * d, 3 * d, 3 * d, d)],
                             self.head_dim, self.head_dim ** -0.5)
        ops.gemm(GEMM_NT, att, self._w(f"l{i}_o_w"), y, bias=self._f(f"l{i}_o_b"), aux=x, epilogue=EPI_BIAS | EPI_ADD_AUX)
        self._ln(ws, y, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        ops.gemm(GEMM_NT, ln, self._w(f"l{i}_fc1_w"), h)
        lib.bias_gelu(h, self._f(f"l{i}_fc1_b"))
        ops.gemm(GEMM_NT, h, self._w(f"l{i}_fc2_w"), y, bias=self._f(f"l{i}_fc2_b"), aux=ln, epilogue=EPI_BIAS | EPI_ADD_AUX)
        self._ln(ws, y, x, f"l{i}_ln2_w", f"l{i}_ln2_b")

    def forward(self, input_values: torch.Tensor, attention_mask=None) -> Wav2Vec2Output:
        c = self.config
        if attention_mask is not None:
            raise NotImplementedError("NativeWav2Vec2: attention_mask is not implemented (the reference never passes one)")
        if ops.fp32_mode():
            raise RuntimeError("NativeWav2Vec2 runs with bf16 storage only: it has no form for the fp32 parity mode (and no eager fallback)")
        if not isinstance(input_values, torch.Tensor) or not input_values.is_cuda:
            raise RuntimeError("NativeWav2Vec2 runs on the GPU only (no CPU fallback)")
        if input_values.dtype != torch.float32:
            raise TypeError(f"NativeWav2Vec2: input_values must be float32, got {input_values.dtype}")
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
            x, y = (ws[k][:rows * d].view(rows, d) for k in ("x", "y"))
            fln = ws["win"][:rows * feat.shape[1]].view(rows, feat.shape[1])
            self._ln(ws, feat, fln, "fp_ln_w", "fp_ln_b")
            ops.gemm(GEMM_NT, fln, self._w("fp_w"), x, bias=self._f("fp_b"), epilogue=EPI_BIAS)
            lib.w2v_posconv(x, pos_w, self._f("pos_b"), y, n, T, d, c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings)
            self._ln(ws, y, x, "enc_ln_w", "enc_ln_b")
            for i in range(c.num_hidden_layers):
                self._layer(i, ws, n, T)
            lib.check(lib.load().mmf_cast_bf16_to_f32(x.data_ptr(), out[n0:n0 + n].data_ptr(), rows * d, lib.stream_ptr()))
        return Wav2Vec2Output(out)
