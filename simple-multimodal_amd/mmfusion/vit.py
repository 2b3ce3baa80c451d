"""Frozen ViT backbone on the HIP kernels: video frames -> token states / CLS features, forward only.

The reference pushes ``B x 30`` frames through HuggingFace's ``ViTModel`` per step and keeps the CLS token of each
(reference models/encoders.py:179,216-226).  ``NativeViT`` is that model rebuilt from its sizes alone (nothing is
fetched), with HuggingFace's ``state_dict`` surface, so published checkpoints and the reference's ``.pth`` files load.

Launch list of one pre-LN layer on a chunk of ``n`` images (rows = n * T tokens, bf16 residual stream like MulT's):

    LayerNorm                     mmf_layernorm_fwd_grouped            x   -> ln
    fused Q/K/V linear + bias     mmf_gemm_grouped NT, BIAS            ln  -> qkv (rows, 3 d)
    attention, H heads of 64/96   mmf_attn_fwd_grouped                 qkv -> att
    out-projection + bias + x     mmf_gemm_grouped NT, BIAS | ADD_AUX  att -> y
    LayerNorm                                                          y   -> ln
    fc1                           mmf_gemm_grouped NT                  ln  -> h (rows, intermediate)
    + bias, exact GELU            mmf_bias_gelu_bf16 (in place)        h
    fc2 + bias + y                mmf_gemm_grouped NT, BIAS | ADD_AUX  h   -> x

In front of the layers: ``mmf_vit_patchify`` -> patch-embedding GEMM + bias -> ``mmf_vit_embed_tokens``; behind them the
final LayerNorm and one widening cast into the f32 result.  ``cls_features`` runs the LAST layer for the CLS rows only:
K and V for every token, but Q, the out-projection, the MLP and the final LayerNorm for row 0 of each image (``Tq = 1``).

Frames are processed in chunks of ``chunk`` images through one workspace allocated once, so memory does not grow with
``B x frames``.  Nothing synchronises with the host: a fixed-shape call can be captured by ``torch.cuda.graph``.

Forward only and frozen: every parameter has ``requires_grad = False`` and the outputs carry no autograd graph
(fine-tuning the backbone is not implemented).  bf16 storage only: in the fp32 parity mode (``ops.fp32_mode()``) the
forward raises instead of computing something else.
"""
from __future__ import annotations

import re
import types
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import arena as _arena
from . import lib, ops
from .lib import EPI_ADD_AUX, EPI_BIAS, GEMM_NT, AttnProblem, LnProblem

BF16 = torch.bfloat16
# images per pass through the workspace (tools/vit_bench.py --chunks; DESIGN.md section 8 has the numbers)
DEFAULT_CHUNK = 160
LN_WIDTHS = (256, 512, 768, 1024)          # the lane forms of layernorm.hip

_V4_LAYER = (("attention.attention.query.", "attention.q_proj."), ("attention.attention.key.", "attention.k_proj."),
             ("attention.attention.value.", "attention.v_proj."), ("attention.output.dense.", "attention.o_proj."),
             ("intermediate.dense.", "mlp.fc1."), ("output.dense.", "mlp.fc2."),
             ("layernorm_before.", "layernorm_before."), ("layernorm_after.", "layernorm_after."))
_V4_RE = re.compile(r"^encoder\.layer\.(\d+)\.(.+)$")
_V5_RE = re.compile(r"^layers\.(\d+)\.(.+)$")


def hf_key_to_v5(key: str) -> str:
    """A transformers 4.x ``ViTModel`` state_dict key in the naming of 5.x (5.x keys pass through)."""
    m = _V4_RE.match(key)
    if not m:
        return key
    for old, new in _V4_LAYER:
        if m.group(2).startswith(old):
            return f"layers.{m.group(1)}.{new}{m.group(2)[len(old):]}"
    return key


def hf_key_to_v4(key: str) -> str:
    """The inverse of ``hf_key_to_v5``."""
    m = _V5_RE.match(key)
    if not m:
        return key
    for old, new in _V4_LAYER:
        if m.group(2).startswith(new):
            return f"encoder.layer.{m.group(1)}.{old}{m.group(2)[len(new):]}"
    return key


class ViTOutput:
    """What the encoders read from a backbone's result."""

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = None


class NativeViT(nn.Module):
    """ViT encoder (HuggingFace ``ViTModel`` without the pooler's arithmetic), defaults = ViT-base/16 at 224 x 224.

    ``forward(pixel_values)`` -> ``.last_hidden_state`` (N, T, hidden) f32 after the final LayerNorm;
    ``cls_features(pixel_values)`` -> (N, hidden) f32, row 0 of the same with the last layer run for those rows only.
    ``pixel_values``: (N, C, H, W) f32 on the GPU.  ``state_dict()`` has the keys and shapes of transformers 5.x;
    ``load_state_dict`` takes those and the 4.x names (``encoder.layer.N.attention.attention.query...``); Q/K/V are
    stored fused and split / merged on the way.  ``pooler.dense`` is kept as an unused parameter pair so that a round
    trip loses nothing."""

    def __init__(self, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, image_size: int = 224, patch_size: int = 16, num_channels: int = 3,
                 layer_norm_eps: float = 1e-12, chunk: int = DEFAULT_CHUNK):
        super().__init__()
        d, H = int(hidden_size), int(num_attention_heads)
        if H <= 0 or d % H or d // H not in (64, 96):
            raise ValueError(f"NativeViT: hidden_size {d} / num_attention_heads {H} must give a head_dim of 64 or 96 "
                             "(the fused attention kernel's forms)")
        if d not in LN_WIDTHS:
            raise ValueError(f"NativeViT: hidden_size {d} is not one of the LayerNorm kernel's widths {LN_WIDTHS}")
        if patch_size <= 0 or patch_size % 8 or image_size % patch_size:
            raise ValueError(f"NativeViT: patch_size {patch_size} must be a multiple of 8 that divides image_size {image_size}")
        if intermediate_size % 8 or num_hidden_layers < 1 or num_channels < 1 or chunk < 1:
            raise ValueError("NativeViT: intermediate_size must be a multiple of 8; layers, channels and chunk at least 1")
        self.config = types.SimpleNamespace(
            hidden_size=d, num_hidden_layers=int(num_hidden_layers), num_attention_heads=H,
            intermediate_size=int(intermediate_size), image_size=int(image_size), patch_size=int(patch_size),
            num_channels=int(num_channels), layer_norm_eps=float(layer_norm_eps), hidden_act="gelu", qkv_bias=True,
            model_type="vit")
        self.chunk = int(chunk)
        self.head_dim = d // H
        self.num_patches = (image_size // patch_size) ** 2
        self.T = self.num_patches + 1
        self.patch_dim = num_channels * patch_size * patch_size
        I, T = int(intermediate_size), self.T
        self._hf: Dict[str, Tuple[str, Optional[Tuple[int, int]]]] = {}      # 5.x key -> (parameter, row range | None)

        def add(name: str, shape, hf: List[Tuple[str, Optional[Tuple[int, int]]]], ones: bool = False, std: float = 0.02):
            p = nn.Parameter(torch.empty(shape), requires_grad=False)
            if ones:
                nn.init.ones_(p)
            elif std > 0:
                nn.init.normal_(p, std=std)
            else:
                nn.init.zeros_(p)
            self.register_parameter(name, p)
            for key, rows in hf:
                self._hf[key] = (name, rows)

        add("cls_token", (1, 1, d), [("embeddings.cls_token", None)])
        add("position_embeddings", (1, T, d), [("embeddings.position_embeddings", None)])
        add("patch_weight", (d, num_channels, patch_size, patch_size), [("embeddings.patch_embeddings.projection.weight", None)])
        add("patch_bias", (d,), [("embeddings.patch_embeddings.projection.bias", None)], std=0.0)
        for i in range(num_hidden_layers):
            a = f"layers.{i}.attention."
            qkv = [(0, d), (d, 2 * d), (2 * d, 3 * d)]
            # (HuggingFace's order inside a layer: q, k, v, o, layernorm_before, layernorm_after, fc1, fc2)
            for n, r in zip("qkv", qkv):
                self._hf[f"{a}{n}_proj.weight"] = (f"l{i}_qkv_w", r)
                self._hf[f"{a}{n}_proj.bias"] = (f"l{i}_qkv_b", r)
            add(f"l{i}_qkv_w", (3 * d, d), [])
            add(f"l{i}_qkv_b", (3 * d,), [], std=0.0)
            add(f"l{i}_o_w", (d, d), [(f"{a}o_proj.weight", None)])
            add(f"l{i}_o_b", (d,), [(f"{a}o_proj.bias", None)], std=0.0)
            add(f"l{i}_ln1_w", (d,), [(f"layers.{i}.layernorm_before.weight", None)], ones=True)
            add(f"l{i}_ln1_b", (d,), [(f"layers.{i}.layernorm_before.bias", None)], std=0.0)
            add(f"l{i}_ln2_w", (d,), [(f"layers.{i}.layernorm_after.weight", None)], ones=True)
            add(f"l{i}_ln2_b", (d,), [(f"layers.{i}.layernorm_after.bias", None)], std=0.0)
            add(f"l{i}_fc1_w", (I, d), [(f"layers.{i}.mlp.fc1.weight", None)])
            add(f"l{i}_fc1_b", (I,), [(f"layers.{i}.mlp.fc1.bias", None)], std=0.0)
            add(f"l{i}_fc2_w", (d, I), [(f"layers.{i}.mlp.fc2.weight", None)])
            add(f"l{i}_fc2_b", (d,), [(f"layers.{i}.mlp.fc2.bias", None)], std=0.0)
        add("ln_w", (d,), [("layernorm.weight", None)], ones=True)
        add("ln_b", (d,), [("layernorm.bias", None)], std=0.0)
        add("pooler_w", (d, d), [("pooler.dense.weight", None)])
        add("pooler_b", (d,), [("pooler.dense.bias", None)], std=0.0)
        self._ws: Optional[dict] = None

    # -- HuggingFace state_dict surface ----------------------------------------------------------------
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for key, (name, rows) in self._hf.items():
            p = getattr(self, name)
            t = p if keep_vars else p.detach()
            destination[prefix + key] = t if rows is None else t[rows[0]:rows[1]]

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        found = {}
        for key in list(state_dict.keys()):
            if not key.startswith(prefix):
                continue
            k5 = hf_key_to_v5(key[len(prefix):])
            if k5 in self._hf:
                found[k5] = state_dict[key]
            elif strict:
                unexpected_keys.append(key)
        with torch.no_grad():
            for k5, (name, rows) in self._hf.items():
                if k5 not in found:
                    missing_keys.append(prefix + k5)
                    continue
                p = getattr(self, name)
                dst = p if rows is None else p[rows[0]:rows[1]]
                src = found[k5]
                if tuple(src.shape) != tuple(dst.shape):
                    error_msgs.append(f"size mismatch for {prefix + k5}: copying a param with shape {tuple(src.shape)} from "
                                      f"checkpoint, the shape in current model is {tuple(dst.shape)}.")
                    continue
                dst.copy_(src)                 # in place: the version counter moves, so the bf16 shadow is re-cast before the next forward

    def hf_state_dict(self, generation: int = 5) -> Dict[str, torch.Tensor]:
        """``state_dict()`` in the key naming of transformers 5.x (the default surface) or 4.x."""
        if generation not in (4, 5):
            raise ValueError("generation must be 4 or 5")
        sd = self.state_dict()
        return sd if generation == 5 else {hf_key_to_v4(k): v for k, v in sd.items()}

    # -- workspace --------------------------------------------------------------------------------------
    def workspace_bytes_per_image(self) -> int:
        c = self.config
        T, d = self.T, c.hidden_size
        h = max(T * c.intermediate_size, self.num_patches * (self.patch_dim + d))
        return 2 * (T * d * 4 + T * 3 * d + h) + 4 * (2 * T + c.num_attention_heads * T)

    def _workspace(self, dev) -> dict:
        ws = self._ws
        if ws is not None and ws["dev"] == dev and ws["chunk"] == self.chunk:
            return ws
        c, n, T, d = self.config, self.chunk, self.T, self.config.hidden_size
        rows = n * T
        h_el = n * max(T * c.intermediate_size, self.num_patches * (self.patch_dim + d))

        def buf(numel, dtype=BF16):
            return torch.empty(numel, dtype=dtype, device=dev)
        ws = {"dev": dev, "chunk": n, "x": buf(rows * d), "y": buf(rows * d), "ln": buf(rows * d), "att": buf(rows * d),
              "qkv": buf(rows * 3 * d), "h": buf(h_el), "mean": buf(rows, torch.float32), "rstd": buf(rows, torch.float32),
              "lse": buf(n * c.num_attention_heads * T, torch.float32)}
        self._ws = ws
        return ws

    # -- launches ---------------------------------------------------------------------------------------
    def _w(self, name: str) -> torch.Tensor:
        return ops.shadow(getattr(self, name))

    def _f(self, name: str) -> torch.Tensor:
        return getattr(self, name).detach()

    def _ln(self, ws, src: torch.Tensor, dst: torch.Tensor, gamma: str, beta: str) -> None:
        rows = src.shape[0]
        with lib._Timed("ln_fwd_kernel", 0.0, [(rows, src.shape[1])]):
            lib.layernorm_fwd_grouped([LnProblem(src.data_ptr(), dst.data_ptr(), self._f(gamma).data_ptr(), self._f(beta).data_ptr(),
                                                 ws["mean"].data_ptr(), ws["rstd"].data_ptr(), None, None, None, None, rows)],
                                      self.config.hidden_size, self.config.layer_norm_eps)

    def _attn(self, ws, qkv: torch.Tensor, att: torch.Tensor, n: int, Tq: int) -> None:
        c, T, d = self.config, self.T, self.config.hidden_size
        base = qkv.data_ptr()
        lib.attn_fwd_grouped([AttnProblem(base, base + 2 * d, base + 4 * d, att.data_ptr(), ws["lse"].data_ptr(), None, None, None,
                                          None, None, n, c.num_attention_heads, Tq, T, 3 * d if Tq == T else T * 3 * d, 3 * d, 3 * d, d)],
                             self.head_dim, self.head_dim ** -0.5)

    def _mlp(self, i: int, ws, y: torch.Tensor, x_out: torch.Tensor, rows: int) -> None:
        """LayerNorm -> fc1 -> bias + GELU -> fc2 + bias + residual on the leading ``rows`` rows of ``y``"""
        d, I = self.config.hidden_size, self.config.intermediate_size
        ln, h = ws["ln"][:rows * d].view(rows, d), ws["h"][:rows * I].view(rows, I)
        self._ln(ws, y, ln, f"l{i}_ln2_w", f"l{i}_ln2_b")
        ops.gemm(GEMM_NT, ln, self._w(f"l{i}_fc1_w"), h)
        lib.bias_gelu(h, self._f(f"l{i}_fc1_b"))
        ops.gemm(GEMM_NT, h, self._w(f"l{i}_fc2_w"), x_out, bias=self._f(f"l{i}_fc2_b"), aux=y, epilogue=EPI_BIAS | EPI_ADD_AUX)

    def _layer(self, i: int, ws, n: int) -> None:
        T, d = self.T, self.config.hidden_size
        rows = n * T
        x, y, ln, att = (ws[k][:rows * d].view(rows, d) for k in ("x", "y", "ln", "att"))
        qkv = ws["qkv"][:rows * 3 * d].view(rows, 3 * d)
        self._ln(ws, x, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        ops.gemm(GEMM_NT, ln, self._w(f"l{i}_qkv_w"), qkv, bias=self._f(f"l{i}_qkv_b"), epilogue=EPI_BIAS)
        self._attn(ws, qkv, att, n, T)
        ops.gemm(GEMM_NT, att, self._w(f"l{i}_o_w"), y, bias=self._f(f"l{i}_o_b"), aux=x, epilogue=EPI_BIAS | EPI_ADD_AUX)
        self._mlp(i, ws, y, x, rows)

    def _layer_cls(self, i: int, ws, n: int) -> None:
        """The last layer for the CLS rows: K / V of every token, everything else on row 0 of each image.  Leaves the
        layer's output for those rows in the leading ``n`` rows of ``x``."""
        T, d = self.T, self.config.hidden_size
        rows = n * T
        x, ln = (ws[k][:rows * d].view(rows, d) for k in ("x", "ln"))
        qkv = ws["qkv"][:rows * 3 * d].view(rows, 3 * d)
        att, y = ws["att"][:n * d].view(n, d), ws["y"][:n * d].view(n, d)
        self._ln(ws, x, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        w, b = self._w(f"l{i}_qkv_w"), self._f(f"l{i}_qkv_b")
        row0 = lambda t, width: t.view(n, T * width)[:, :d]          # row 0 of each image, as an (n, d) row-strided view
        ops.gemm_group(GEMM_NT, [(ln, w[d:], qkv[:, d:], b[d:], None), (row0(ln, d), w[:d], row0(qkv, 3 * d), b[:d], None)], EPI_BIAS)
        self._attn(ws, qkv, att, n, 1)
        ops.gemm(GEMM_NT, att, self._w(f"l{i}_o_w"), y, bias=self._f(f"l{i}_o_b"), aux=row0(x, d), epilogue=EPI_BIAS | EPI_ADD_AUX)
        self._mlp(i, ws, y, ws["x"][:n * d].view(n, d), n)

    def _embed(self, ws, pixels: torch.Tensor, n: int) -> None:
        c, T, d, K, NP = self.config, self.T, self.config.hidden_size, self.patch_dim, self.num_patches
        patches = ws["h"][:n * NP * K].view(n * NP, K)
        off = self.chunk * NP * K
        pe = ws["h"][off:off + n * NP * d].view(n * NP, d)
        lib.vit_patchify(pixels, patches, n, c.num_channels, c.image_size, c.image_size, c.patch_size)
        ops.gemm(GEMM_NT, patches, self._w("patch_weight").view(d, K), pe, bias=self._f("patch_bias"), epilogue=EPI_BIAS)
        lib.vit_embed_tokens(pe, self._f("cls_token"), self._f("position_embeddings"), ws["x"], n, T, d)

    def _run(self, pixel_values: torch.Tensor, cls_only: bool) -> torch.Tensor:
        c = self.config
        if ops.fp32_mode():
            raise RuntimeError("NativeViT runs with bf16 storage only: it has no form for the fp32 parity mode (and no eager fallback)")
        if not isinstance(pixel_values, torch.Tensor) or not pixel_values.is_cuda:
            raise RuntimeError("NativeViT runs on the GPU only (no CPU fallback)")
        if pixel_values.dtype != torch.float32:
            raise TypeError(f"NativeViT: pixel_values must be float32, got {pixel_values.dtype}")
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (c.num_channels, c.image_size, c.image_size):
            raise ValueError(f"NativeViT: pixel_values {tuple(pixel_values.shape)} is not (N, {c.num_channels}, {c.image_size}, "
                             f"{c.image_size}) (position embeddings are not interpolated)")
        pixel_values = pixel_values.contiguous()
        _arena.ensure(self)
        N, T, d = pixel_values.shape[0], self.T, c.hidden_size
        ws = self._workspace(pixel_values.device)
        out = torch.empty((N, d) if cls_only else (N, T, d), dtype=torch.float32, device=pixel_values.device)
        L = c.num_hidden_layers
        for n0 in range(0, N, self.chunk):
            n = min(self.chunk, N - n0)
            self._embed(ws, pixel_values[n0:n0 + n], n)
            for i in range(L - 1 if cls_only else L):
                self._layer(i, ws, n)
            if cls_only:
                self._layer_cls(L - 1, ws, n)
            rows = n if cls_only else n * T
            x, ln = ws["x"][:rows * d].view(rows, d), ws["ln"][:rows * d].view(rows, d)
            self._ln(ws, x, ln, "ln_w", "ln_b")
            lib.check(lib.load().mmf_cast_bf16_to_f32(ln.data_ptr(), out[n0:n0 + n].data_ptr(), rows * d, lib.stream_ptr()))
        return out

    def forward(self, pixel_values: torch.Tensor) -> ViTOutput:
        return ViTOutput(self._run(pixel_values, cls_only=False))

    def cls_features(self, pixel_values: torch.Tensor) -> torch.Tensor:
        return self._run(pixel_values, cls_only=True)
