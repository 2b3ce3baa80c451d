"""Frozen ViT backbone on the HIP kernels: video frames -> token states / CLS features, forward only.

The reference pushes ``B x 30`` frames through HuggingFace's ``ViTModel`` per step and keeps the CLS token of each
(reference models/encoders.py:179,216-226).  ``NativeViT`` is that model rebuilt from its sizes alone (nothing is
fetched), with HuggingFace's ``state_dict`` surface, so published checkpoints and the reference's ``.pth`` files load.

One pre-LN layer on a chunk of ``n`` images (rows = n * T tokens), in the blocks whose launch rows mmfusion/backbone.py lists:

    LayerNorm                     x -> ln
    _attention(ln, + x)           ln -> qkv -> att -> y
    LayerNorm                     y -> ln
    _ffn(ln, + y)                 ln -> h -> x

In front of the layers: ``mmf_vit_patchify`` -> patch-embedding GEMM + bias -> ``mmf_vit_embed_tokens``; behind them the
final LayerNorm and one widening cast into the f32 result.  Decoded uint8 ``(N, Hs, Ws, 3)`` frames are taken too: then
``mmf_video_prepare_patches`` (mmfusion/prep.py) resizes them straight into the patch matrix, with the same bits as
``mmf_vit_patchify`` of the prepared f32 frames, which are never written.  ``cls_features`` runs the LAST layer for the CLS rows only:
K and V for every token, but Q, the out-projection, the MLP and the final LayerNorm for row 0 of each image (``Tq = 1``).

Frames are processed in chunks of ``chunk`` images through one workspace allocated once, so memory does not grow with
``B x frames``.  Forward only, frozen, bf16 storage only, nothing synchronises with the host (mmfusion/backbone.py).
"""
from __future__ import annotations

import re
import types
from typing import Dict, Optional

import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BackboneOutput, FrozenBackbone, WsTable
from .lib import EPI_BIAS, GEMM_NT
from .prep import VideoAug

# images per pass through the workspace (tools/vit_bench.py --chunks; DESIGN.md section 8 has the numbers)
DEFAULT_CHUNK = 160

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


class NativeViT(FrozenBackbone):
    """ViT encoder (HuggingFace ``ViTModel`` without the pooler's arithmetic), defaults = ViT-base/16 at 224 x 224.

    ``forward(pixel_values)`` -> ``.last_hidden_state`` (N, T, hidden) f32 after the final LayerNorm;
    ``cls_features(pixel_values)`` -> (N, hidden) f32, row 0 of the same with the last layer run for those rows only.
    ``pixel_values``: (N, C, H, W) f32 on the GPU, or decoded frames (N, Hs, Ws, 3) uint8 of any size, which are resized to
    the model's on the way into the patch matrix; ``aug`` (a ``prep.VideoAug``, uint8 input only) says how.  ``state_dict()`` has the keys and shapes of transformers 5.x;
    ``load_state_dict`` takes those and the 4.x names (``encoder.layer.N.attention.attention.query...``); Q/K/V are
    stored fused and split / merged on the way.  ``pooler.dense`` is kept as an unused parameter pair so that a round
    trip loses nothing."""

    def __init__(self, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, image_size: int = 224, patch_size: int = 16, num_channels: int = 3,
                 layer_norm_eps: float = 1e-12, chunk: int = DEFAULT_CHUNK):
        d, H = int(hidden_size), int(num_attention_heads)
        super().__init__(d, H, chunk)
        if patch_size <= 0 or patch_size % 8 or image_size % patch_size:
            raise ValueError(f"NativeViT: patch_size {patch_size} must be a multiple of 8 that divides image_size {image_size}")
        if intermediate_size % 8 or num_hidden_layers < 1 or num_channels < 1 or chunk < 1:
            raise ValueError("NativeViT: intermediate_size must be a multiple of 8; layers, channels and chunk at least 1")
        self.config = types.SimpleNamespace(
            hidden_size=d, num_hidden_layers=int(num_hidden_layers), num_attention_heads=H,
            intermediate_size=int(intermediate_size), image_size=int(image_size), patch_size=int(patch_size),
            num_channels=int(num_channels), layer_norm_eps=float(layer_norm_eps), hidden_act="gelu", qkv_bias=True,
            model_type="vit")
        self.num_patches = (image_size // patch_size) ** 2
        self.T = self.num_patches + 1
        self.patch_dim = num_channels * patch_size * patch_size
        I, T, add = int(intermediate_size), self.T, self._add
        add("cls_token", (1, 1, d), "embeddings.cls_token")
        add("position_embeddings", (1, T, d), "embeddings.position_embeddings")
        add("patch_weight", (d, num_channels, patch_size, patch_size), "embeddings.patch_embeddings.projection.weight")
        add("patch_bias", (d,), "embeddings.patch_embeddings.projection.bias", std=0.0)
        for i in range(num_hidden_layers):
            a = f"layers.{i}."
            self._add_layer(i, d, I, {"q": a + "attention.q_proj", "k": a + "attention.k_proj", "v": a + "attention.v_proj",
                                      "o": a + "attention.o_proj", "ln1": a + "layernorm_before", "ln2": a + "layernorm_after",
                                      "fc1": a + "mlp.fc1", "fc2": a + "mlp.fc2"})
        add("ln_w", (d,), "layernorm.weight", ones=True)
        add("ln_b", (d,), "layernorm.bias", std=0.0)
        add("pooler_w", (d, d), "pooler.dense.weight")
        add("pooler_b", (d,), "pooler.dense.bias", std=0.0)

    # -- HuggingFace state_dict surface ----------------------------------------------------------------
    def _canonical_key(self, key: str) -> str:
        return hf_key_to_v5(key)

    def hf_state_dict(self, generation: int = 5) -> Dict[str, torch.Tensor]:
        """``state_dict()`` in the key naming of transformers 5.x (the default surface) or 4.x."""
        if generation not in (4, 5):
            raise ValueError("generation must be 4 or 5")
        sd = self.state_dict()
        return sd if generation == 5 else {hf_key_to_v4(k): v for k, v in sd.items()}

    # -- workspace --------------------------------------------------------------------------------------
    def _ws_table(self, size=None) -> WsTable:
        """per image (the model fixes its size); ``h`` also holds the patches and their embeddings in front of the layers"""
        c = self.config
        return self._token_table(self.T, max(self.T * c.intermediate_size, self.num_patches * (self.patch_dim + c.hidden_size)))

    def workspace_bytes_per_image(self) -> int:
        return self._bytes_per_item(self._ws_table())

    # -- launches ---------------------------------------------------------------------------------------
    def _layer(self, i: int, ws, n: int) -> None:
        rows, d = n * self.T, self.config.hidden_size
        x, ln = self._rows(ws, "x", rows, d), self._rows(ws, "ln", rows, d)
        self._ln(ws, x, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        y = self._attention(i, ws, ln, x, n, self.T)
        self._ln(ws, y, ln, f"l{i}_ln2_w", f"l{i}_ln2_b")
        self._ffn(i, ws, ln, y, x)

    def _layer_cls(self, i: int, ws, n: int) -> None:
        """The last layer for the CLS rows: K / V of every token, everything else on row 0 of each image.  Leaves the
        layer's output for those rows in the leading ``n`` rows of ``x``."""
        T, d = self.T, self.config.hidden_size
        rows = n * T
        x, ln, qkv = self._rows(ws, "x", rows, d), self._rows(ws, "ln", rows, d), self._rows(ws, "qkv", rows, 3 * d)
        att, y, ln0 = (self._rows(ws, k, n, d) for k in ("att", "y", "ln"))
        self._ln(ws, x, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        w, b = self._w(f"l{i}_qkv_w"), self._f(f"l{i}_qkv_b")
        row0 = lambda t, width: t.view(n, T * width)[:, :d]          # row 0 of each image, as an (n, d) row-strided view
        ops.gemm_group(GEMM_NT, [(ln, w[d:], qkv[:, d:], b[d:], None), (row0(ln, d), w[:d], row0(qkv, 3 * d), b[:d], None)], EPI_BIAS)
        self._attn(ws, qkv, att, n, 1, T)
        self._out_proj(i, att, row0(x, d), y)
        self._ln(ws, y, ln0, f"l{i}_ln2_w", f"l{i}_ln2_b")
        self._ffn(i, ws, ln0, y, self._rows(ws, "x", n, d))

    def _embed(self, ws, pixels: torch.Tensor, n: int, aug: Optional[VideoAug]) -> None:
        c, T, d, K, NP = self.config, self.T, self.config.hidden_size, self.patch_dim, self.num_patches
        patches = ws["h"][:n * NP * K].view(n * NP, K)
        off = self.chunk * NP * K
        pe = ws["h"][off:off + n * NP * d].view(n * NP, d)
        if pixels.dtype == torch.uint8:
            lib.video_prepare(pixels, patches, c.image_size, c.image_size, c.patch_size, aug.bgr, aug.live, aug.brightness, aug.flip)
        else:
            lib.vit_patchify(pixels, patches, n, c.num_channels, c.image_size, c.image_size, c.patch_size)
        ops.gemm(GEMM_NT, patches, self._w("patch_weight").view(d, K), pe, bias=self._f("patch_bias"), epilogue=EPI_BIAS)
        lib.vit_embed_tokens(pe, self._f("cls_token"), self._f("position_embeddings"), ws["x"], n, T, d)

    def _run(self, pixel_values: torch.Tensor, cls_only: bool, aug: Optional[VideoAug] = None) -> torch.Tensor:
        c = self.config
        frames = isinstance(pixel_values, torch.Tensor) and pixel_values.dtype == torch.uint8
        if frames:
            self._check_input(pixel_values, "pixel_values", torch.uint8)
            if pixel_values.dim() != 4 or pixel_values.shape[3] != 3 or c.num_channels != 3:
                raise ValueError(f"NativeViT: uint8 pixel_values {tuple(pixel_values.shape)} is not (N, Hs, Ws, 3) decoded frames "
                                 f"for a 3-channel model")
            aug = aug if aug is not None else VideoAug()
        else:
            self._check_input(pixel_values, "pixel_values")
            if aug is not None:
                raise ValueError("NativeViT: aug goes with uint8 (N, Hs, Ws, 3) frames; f32 pixel_values are taken as prepared")
        if not frames and (pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (c.num_channels, c.image_size, c.image_size)):
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
            self._embed(ws, pixel_values[n0:n0 + n], n, aug.rows(n0, n0 + n) if frames else None)
            for i in range(L - 1 if cls_only else L):
                self._layer(i, ws, n)
            if cls_only:
                self._layer_cls(L - 1, ws, n)
            rows = n if cls_only else n * T
            x, ln = self._rows(ws, "x", rows, d), self._rows(ws, "ln", rows, d)
            self._ln(ws, x, ln, "ln_w", "ln_b")
            self._widen(ln, out[n0:n0 + n])
        return out

    def forward(self, pixel_values: torch.Tensor, aug: Optional[VideoAug] = None) -> BackboneOutput:
        return BackboneOutput(self._run(pixel_values, cls_only=False, aug=aug))

    def cls_features(self, pixel_values: torch.Tensor, aug: Optional[VideoAug] = None) -> torch.Tensor:
        return self._run(pixel_values, cls_only=True, aug=aug)
