"""ViT backbone on the HIP kernels: video frames -> token states / CLS features; frozen by default, with the weight gradients of
the top layers marked trainable (fine-tuning).

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
``B x frames``.  Frozen by default, bf16 storage only, nothing synchronises with the host (mmfusion/backbone.py).

The top-K weight gradients.  ``set_trainable_layers(k, embeddings=False)`` marks the parameters of layers ``L - k .. L - 1`` and the
final LayerNorm trainable (with ``k == L`` and ``embeddings``: the CLS token, the position embeddings and the patch projection
too).  With grad mode on every call is then one ``torch.autograd.Function`` around the launch list above (the trainable
parameters are its inputs, so the result carries a graph; there is no gradient with respect to the pixels) plus one copy per
walked layer: it keeps the bf16 input ``x`` of layers ``>= L - k`` and of the final LayerNorm.  The backward, per chunk: the final
LayerNorm's backward, then per layer top down the layer's forward again from its saved ``x`` up to the GELU output (nothing
behind fc2 is read by a pre-LN layer's backward) and

      fc2 wgrad, dgrad              mmf_gemm_grouped TN (COLSUM_A) / NN      gx -> dg
      GELU backward                 mmf_bias_gelu_bwd_bf16 (in place)        dg, h -> dh
      fc1 wgrad, dgrad              TN / NN                                  dh -> dln2
      LayerNorm backward + gx       mmf_layernorm_bwd_add_grouped            dln2, y (+ gx) -> dy
      out-projection wgrad, dgrad   TN / NN                                  dy -> datt
      attention backward            mmf_attn_bwd_grouped on the fused rows   datt -> dqkv
      Q/K/V wgrad, dgrad            TN / NN                                  dqkv -> dln1
      LayerNorm backward + dy       mmf_layernorm_bwd_add_grouped            dln1, x (+ dy) -> gx of the layer below

The residual gradient of a pre-LN layer joins behind a LayerNorm backward, where no GEMM epilogue can add it: the LayerNorm
backward takes it as one more operand (f32 add in front of dx's one rounding, in place).  The key bias gets no column sum: its
exact gradient is zero (a shift of every key by one vector moves every score of a row equally), what a sum of dK would add is
the bf16 residue of delta and dK.  A weight gradient over a chunk's rows is a few 256 x 256 output tiles under tens of
thousands of rows; ``_slabs_for`` cuts the rows into K-slabs that one grouped launch multiplies and ``mmf_sum_slabs_f32`` sums
(mmfusion/backbone.py ``_wgrad_launch``; DESIGN.md section 8 has the rule and its measurements).  On the ``cls_features`` route
the last layer's backward has ``_layer_cls``'s form: MLP, out-projection and both LayerNorms on one row per image, the attention
backward of that one query per image as ``mmf_vit_cls_attn_bwd`` (dQ for row 0, dK | dV for every row; plain f32 with
delta = sum_j p_j dp_j: ``mmf_attn_bwd_grouped``'s delta = dO . O carries the rounding of the bf16 O, which a single query's dQ and
dK do not average out), the Q rows of the weight gradient over those ``n`` rows and the
K | V rows over all; dln1 is the K | V input gradient plus, on row 0, the Q one (through a zeroed buffer the K | V GEMM's epilogue
adds), and the residual gradient reaches row 0 only (a zeroed buffer with those rows copied in).  With the embeddings trainable,
``mmf_vit_embed_tokens_bwd`` sums the CLS / position gradients over the images and the patch matrix is built again for the patch
projection's weight gradient.  Gradients are added into the parameters' f32 ``.grad`` (the arena's lazy-zero protocol as
``ops.queue_wgrad`` keeps it) in stream order; what the backward holds beside the forward workspace is ``_grad_table``.
"""
from __future__ import annotations

import re
import types
from typing import Dict, Optional

import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BF16, BackboneOutput, FrozenBackbone, WsTable
from .lib import EPI_ADD_AUX, EPI_BIAS, GEMM_NN, GEMM_NT
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


class _Differentiable(torch.autograd.Function):
    """``NativeViT._launches``, differentiable with respect to the trainable parameters (``params``; never to the pixels).  They
    are inputs so that the result carries a graph; their gradients are not returned but added into their f32 ``.grad`` by the
    backward's own launches, as ``ops.queue_wgrad``'s are."""

    @staticmethod
    def forward(ctx, model: "NativeViT", pixels: torch.Tensor, cls_only: bool, aug: Optional[VideoAug], *params) -> torch.Tensor:
        N, T, d, L = pixels.shape[0], model.T, model.config.hidden_size, model.config.num_hidden_layers
        first = L - model.trainable_layers                             # the lowest layer the backward walks
        keep = model._keep(first, N * T, pixels.device)
        final = torch.empty((N if cls_only else N * T, d), dtype=BF16, device=pixels.device)
        out = model._launches(pixels, cls_only, aug, keep, first, final)
        ctx.model, ctx.cls_only, ctx.aug, ctx.first, ctx.embeddings = model, cls_only, aug, first, model.trainable_embeddings
        ctx.save_for_backward(pixels, keep, final)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        pixels, keep, final = ctx.saved_tensors
        if any(ctx.needs_input_grad[4:]):
            ctx.model._backward(pixels, ctx.cls_only, ctx.aug, keep, final, ctx.first, ctx.embeddings, dout.contiguous())
        return (None,) * len(ctx.needs_input_grad)


class NativeViT(FrozenBackbone):
    """ViT encoder (HuggingFace ``ViTModel`` without the pooler's arithmetic), defaults = ViT-base/16 at 224 x 224.

    ``forward(pixel_values)`` -> ``.last_hidden_state`` (N, T, hidden) f32 after the final LayerNorm;
    ``cls_features(pixel_values)`` -> (N, hidden) f32, row 0 of the same with the last layer run for those rows only.
    Frozen by default; after ``set_trainable_layers(k)``, ``k > 0``, both carry the top ``k`` layers' weight gradients when
    called in grad mode (never a gradient with respect to ``pixel_values``).
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
        self._embeddings = False                       # set_trainable_layers(L, embeddings=True)

    # -- fine-tuning --------------------------------------------------------------------------------------
    _EMBEDDING_PARAMS = ("cls_token", "position_embeddings", "patch_weight", "patch_bias")

    @property
    def trainable_embeddings(self) -> bool:
        return self._embeddings

    def _trainable_names(self) -> list:
        """the parameters that require a gradient, in the order the differentiable forward takes them"""
        L, k = self.config.num_hidden_layers, self._trainable
        names = list(self._EMBEDDING_PARAMS) if self._embeddings else []
        names += [n for i in range(L - k, L) for n in self._layer_params(i)]
        return names + (["ln_w", "ln_b"] if k else [])

    def set_trainable_layers(self, k: int, embeddings: bool = False) -> None:
        """The parameters of the top ``k`` layers (``L - k .. L - 1``) and, for ``k >= 1``, the final LayerNorm get
        ``requires_grad = True``, every other parameter ``False``; 0 freezes the backbone again.  ``embeddings=True`` (with
        ``k == L`` only: the gradient reaches them through every layer) also trains the CLS token, the position embeddings and
        the patch projection.  With grad mode on and ``k > 0``, ``forward`` and ``cls_features`` return a result that carries a
        graph; its backward adds those parameters' gradients into their f32 ``.grad`` (the module's parameter arena) and stops
        below layer ``L - k``.  ``pooler.dense`` stays frozen whatever ``k`` (nothing reads it), there is no gradient with respect
        to the pixels, the backbone's dropout is not built, and the fp32 parity mode is refused as everywhere in this class."""
        self._check_trainable(k, "embeddings", embeddings, "the embeddings train", "their gradient comes through every layer")
        self._trainable, self._embeddings = k, embeddings
        self._require_grad(self._trainable_names())

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
    def _layer_cls(self, i: int, ws, n: int) -> None:
        """The last layer for the CLS rows: K / V of every token, everything else on row 0 of each image.  Leaves the
        layer's output for those rows in the leading ``n`` rows of ``x``."""
        d = self.config.hidden_size
        y, ln0 = self._cls_attention(i, ws, ws, self._rows(ws, "x", n * self.T, d), n), self._rows(ws, "ln", n, d)
        self._ln(ws, y, ln0, f"l{i}_ln2_w", f"l{i}_ln2_b")
        self._ffn(i, ws, ln0, y, self._rows(ws, "x", n, d))

    def _row0(self, t: torch.Tensor, n: int) -> torch.Tensor:
        """row 0 of each image's leading ``hidden`` columns of a contiguous (n T, width) buffer, as an (n, hidden) row-strided view"""
        return t.view(n, self.T * t.shape[1])[:, :self.config.hidden_size]

    def _cls_attention(self, i: int, ws, st, x: torch.Tensor, n: int) -> torch.Tensor:
        """the attention block of ``_layer_cls`` on the layer input ``x`` (n T rows) -> y (n rows) = row 0 of x + the
        out-projection; ``ln`` keeps LayerNorm(x) of every row and ``st`` (``mean`` / ``rstd``) its statistics"""
        T, d = self.T, self.config.hidden_size
        rows = n * T
        ln, qkv = self._rows(ws, "ln", rows, d), self._rows(ws, "qkv", rows, 3 * d)
        att, y = self._rows(ws, "att", n, d), self._rows(ws, "y", n, d)
        self._ln(st, x, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        w, b = self._w(f"l{i}_qkv_w"), self._f(f"l{i}_qkv_b")
        ops.gemm_group(GEMM_NT, [(ln, w[d:], qkv[:, d:], b[d:], None), (self._row0(ln, n), w[:d], self._row0(qkv, n), b[:d], None)], EPI_BIAS)
        self._attn(ws, qkv, att, n, 1, T)
        self._out_proj(i, att, self._row0(x, n), y)
        return y

    def _patches(self, ws, pixels: torch.Tensor, n: int, aug: Optional[VideoAug]) -> torch.Tensor:
        """the chunk's patch matrix (n patches, C P P) bf16, in the leading part of ``h``"""
        c, K, NP = self.config, self.patch_dim, self.num_patches
        patches = ws["h"][:n * NP * K].view(n * NP, K)
        if pixels.dtype == torch.uint8:
            lib.video_prepare(pixels, patches, c.image_size, c.image_size, c.patch_size, aug.bgr, aug.live, aug.brightness, aug.flip)
        else:
            lib.vit_patchify(pixels, patches, n, c.num_channels, c.image_size, c.image_size, c.patch_size)
        return patches

    def _embed(self, ws, pixels: torch.Tensor, n: int, aug: Optional[VideoAug]) -> None:
        T, d, K, NP = self.T, self.config.hidden_size, self.patch_dim, self.num_patches
        patches = self._patches(ws, pixels, n, aug)
        off = self.chunk * NP * K
        pe = ws["h"][off:off + n * NP * d].view(n * NP, d)
        ops.gemm(GEMM_NT, patches, self._w("patch_weight").view(d, K), pe, bias=self._f("patch_bias"), epilogue=EPI_BIAS)
        lib.vit_embed_tokens(pe, self._f("cls_token"), self._f("position_embeddings"), ws["x"], n, T, d)


    def _checked(self, pixel_values: torch.Tensor, aug: Optional[VideoAug]):
        """-> (the contiguous input, its ``aug``: a ``VideoAug`` for uint8 frames, None for f32 pixels)"""
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
        return pixel_values.contiguous(), aug

    def _run(self, pixel_values: torch.Tensor, cls_only: bool, aug: Optional[VideoAug] = None) -> torch.Tensor:
        pixels, aug = self._checked(pixel_values, aug)
        if torch.is_grad_enabled() and self._trainable > 0:
            return _Differentiable.apply(self, pixels.detach(), cls_only, aug, *(getattr(self, n) for n in self._trainable_names()))
        return self._launches(pixels, cls_only, aug)

    def _launches(self, pixels: torch.Tensor, cls_only: bool, aug: Optional[VideoAug], keep: Optional[torch.Tensor] = None,
                  first: int = 0, final: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the launch list on checked inputs -> (N, d) / (N, T, d) f32.  The differentiable call's: ``keep`` (layers - first, N T, d)
        bf16 also takes a copy of the input of every layer from ``first`` up, ``final`` one of the final LayerNorm's input"""
        c = self.config
        _arena.ensure(self)
        N, T, d = pixels.shape[0], self.T, c.hidden_size
        ws = self._workspace(pixels.device)
        out = torch.empty((N, d) if cls_only else (N, T, d), dtype=torch.float32, device=pixels.device)
        L = c.num_hidden_layers
        for n0, n in self._chunks(N):
            self._embed(ws, pixels[n0:n0 + n], n, aug.rows(n0, n0 + n) if aug is not None else None)
            for i in range(L):
                if keep is not None and i >= first:
                    keep[i - first, n0 * T:(n0 + n) * T].copy_(self._rows(ws, "x", n * T, d))
                if cls_only and i == L - 1:
                    self._layer_cls(i, ws, n)
                else:
                    self._pre_ln_layer(i, ws, n, T)
            rows, r0 = (n, n0) if cls_only else (n * T, n0 * T)
            x, ln = self._rows(ws, "x", rows, d), self._rows(ws, "ln", rows, d)
            if final is not None:
                final[r0:r0 + rows].copy_(x)
            self._ln(ws, x, ln, "ln_w", "ln_b")
            self._widen(ln, out[n0:n0 + n])
        return out

    def forward(self, pixel_values: torch.Tensor, aug: Optional[VideoAug] = None) -> BackboneOutput:
        return BackboneOutput(self._run(pixel_values, cls_only=False, aug=aug))

    def cls_features(self, pixel_values: torch.Tensor, aug: Optional[VideoAug] = None) -> torch.Tensor:
        return self._run(pixel_values, cls_only=True, aug=aug)

    # -- the backward: the trainable layers' weight gradients ------------------------------------------------------------
    def _grad_table(self, size=None) -> WsTable:
        """what the backward holds beside the forward workspace, per image: ``_grad_rows`` with the second LayerNorm's output
        ``ln2`` (``ln`` keeps the first's: the Q/K/V weight gradient reads it).  lse is the forward workspace's"""
        return self._grad_rows(self.T, "ln2")

    def grad_workspace_bytes_per_image(self) -> int:
        return self._bytes_per_item(self._grad_table())

    def _attn_bwd(self, ws, g, qkv: torch.Tensor, att: torch.Tensor, datt: torch.Tensor, dqkv: torch.Tensor, n: int, Tq: int) -> None:
        """``_attn``'s backward: dQ | dK | dV into the fused ``dqkv`` rows, laid out as ``qkv``.  ``Tq == 1`` (``mmf_vit_cls_attn_bwd``):
        the query and ``datt`` rows are one per image, dQ lands in the leading columns of each image's row 0 and the dQ columns
        of the other rows are not written"""
        if Tq == 1:
            lib.vit_cls_attn_bwd(qkv, datt, dqkv, n, self.config.num_attention_heads, self.T, self.head_dim, self.head_dim ** -0.5)
            return
        lib.attn_bwd_grouped([self._attn_problem(ws, qkv, att, n, Tq, self.T, datt, g["delta"], dqkv)], self.head_dim, self.head_dim ** -0.5)

    def _qkv_wgrad(self, i: int, g, dqkv: torch.Tensor, ln: torch.Tensor, n: int, cls: bool) -> None:
        """layer ``i``'s fused Q/K/V weight and bias gradients from ``dqkv`` and the first LayerNorm's output ``ln``
        (``FrozenBackbone._qkv_wgrad_roles``: the key bias takes no column sum).  ``cls``: dQ is row 0 of each image only, so the Q
        rows of the weight are a launch of their own over those ``n`` rows"""
        d = self.config.hidden_size
        w, b = self._grads(i, "qkv")
        over = self._first_touch(w)
        if cls:
            self._wgrad_launch([(self._row0(dqkv, n), self._row0(ln, n), w[:d], b[:d])], over)
        self._qkv_wgrad_roles(i, g["junk"], dqkv, ln, (1, 2) if cls else (0, 1, 2), over)

    def _layer_grad(self, i: int, ws, g, xin: torch.Tensor, n: int, cls: bool) -> None:
        """layer ``i`` again from its saved input ``xin`` up to the GELU output, then its backward with the weight, bias and
        LayerNorm gradients added into the parameters' ``.grad``.  ``ga`` holds the gradient of the layer's output on entry and
        of ``xin`` (n T rows) on return.  Every row: ``_pre_ln_layer_grad`` (mmfusion/backbone.py).  ``cls``: the layer in
        ``_layer_cls``'s form, below; on entry ``ga`` then is n rows, one per image"""
        if not cls:
            self._pre_ln_layer_grad(i, ws, g, xin, n, self.T, lambda qkv, att, datt, dqkv: self._attn_bwd(ws, g, qkv, att, datt, dqkv, n, self.T),
                                    lambda dqkv, ln1: self._qkv_wgrad(i, g, dqkv, ln1, n, False), self._slabs_for)
            return
        c, T = self.config, self.T
        d, I, R, rows = c.hidden_size, c.intermediate_size, self._rows, n * T
        ln1, qkv, dqkv = R(ws, "ln", rows, d), R(ws, "qkv", rows, 3 * d), R(g, "dqkv", rows, 3 * d)
        att, h, ln2, gel, ga, gb, dh = R(ws, "att", n, d), R(ws, "h", n, I), R(g, "ln2", n, d), R(g, "g", n, I), R(g, "ga", n, d), R(g, "gb", n, d), R(g, "dh", n, I)
        st1, st2 = self._stats(g, 1), self._stats(g, 2)
        slabs = lambda M, N: self._slabs_for(n, self._tiles(M, N))
        W, F = lambda r: self._w(f"l{i}_{r}_w"), lambda r: self._f(f"l{i}_{r}_b")
        # the forward again, up to the GELU output (nothing behind fc2 is read by a pre-LN layer's backward)
        y = self._cls_attention(i, ws, st1, xin, n)
        self._ln(st2, y, ln2, f"l{i}_ln2_w", f"l{i}_ln2_b")
        ops.gemm(GEMM_NT, ln2, W("fc1"), h)
        lib.bias_gelu_to(h, F("fc1"), gel)
        # the MLP
        self._wgrad(ga, gel, f"l{i}_fc2", slabs(d, I))
        ops.gemm(GEMM_NN, ga, W("fc2"), dh)                                            # dg
        lib.bias_gelu_bwd(dh, h, F("fc1"), dh)
        self._wgrad(dh, ln2, f"l{i}_fc1", slabs(I, d))
        ops.gemm(GEMM_NN, dh, W("fc1"), gb)                                            # dln2
        self._ln_bwd(st2, y, gb, ga, f"l{i}_ln2_w", self._grads(i, "ln2"), resid=ga)   # ga = dy: the MLP branch + the residual
        # the attention
        self._wgrad(ga, att, f"l{i}_o", slabs(d, d))
        ops.gemm(GEMM_NN, ga, W("o"), gb)                                              # datt
        self._attn_bwd(ws, g, qkv, att, gb, dqkv, n, 1)
        self._qkv_wgrad(i, g, dqkv, ln1, n, True)
        gx, gl = R(g, "ga", rows, d), R(g, "gb", rows, d)
        # dln1 = the K | V input gradient of every row + the Q one on row 0 of each image: the latter goes into a zeroed buffer
        # (``g``: the GELU output is done with) that the former's epilogue adds; the residual gradient reaches row 0 only, so it
        # is a zeroed buffer too (``ln2``) with ``ga``'s n rows copied in
        z, resid = R(g, "g", rows, d), R(g, "ln2", rows, d)
        z.zero_()
        ops.gemm(GEMM_NN, self._row0(dqkv, n), W("qkv")[:d], self._row0(z, n))
        ops.gemm(GEMM_NN, dqkv[:, d:], W("qkv")[d:], gl, aux=z, epilogue=EPI_ADD_AUX)
        resid.zero_()
        self._row0(resid, n).copy_(ga)
        self._ln_bwd(st1, xin, gl, gx, f"l{i}_ln1_w", self._grads(i, "ln1"), resid=resid)

    def _backward(self, pixels: torch.Tensor, cls_only: bool, aug: Optional[VideoAug], keep: torch.Tensor, final: torch.Tensor,
                  first: int, embeddings: bool, dout: torch.Tensor) -> None:
        """for the gradient ``dout`` (N, d) / (N, T, d) f32 of the result: the gradients of the final LayerNorm, of layers
        ``first`` .. L - 1 and, with ``embeddings``, of the CLS token, the position embeddings and the patch projection, added
        into their ``.grad``.  ``keep``: the saved inputs of the layers from ``first`` up, ``final``: of the final LayerNorm"""
        c, d, dev = self.config, self.config.hidden_size, pixels.device
        self._refuse_fp32()
        N, T, L, NP, K = pixels.shape[0], self.T, c.num_hidden_layers, self.num_patches, self.patch_dim
        ws, g = self._workspace(dev), self._grad_workspace(dev)
        st = self._stats(g, 1)
        dout = dout.view(N, -1)
        for n0, n in self._chunks(N):
            rows, r0 = (n, n0) if cls_only else (n * T, n0 * T)
            ga, gb, xf = self._rows(g, "ga", rows, d), self._rows(g, "gb", rows, d), final[r0:r0 + rows]
            self._narrow(dout[n0:n0 + n], gb)
            self._ln(st, xf, self._rows(ws, "ln", rows, d), "ln_w", "ln_b")            # for its statistics; the output is not read
            self._ln_bwd(st, xf, gb, ga, "ln_w", (self.ln_w.grad, self.ln_b.grad))
            for i in reversed(range(first, L)):
                self._layer_grad(i, ws, g, keep[i - first, n0 * T:(n0 + n) * T], n, cls_only and i == L - 1)
            if embeddings:
                dtok, dpe = self._rows(g, "ga", n * T, d), self._rows(g, "gb", n * NP, d)
                lib.vit_embed_tokens_bwd(dtok, self.cls_token.grad, self.position_embeddings.grad, dpe, n, T, d)
                patches = self._patches(ws, pixels[n0:n0 + n], n, aug.rows(n0, n0 + n) if aug is not None else None)
                wg = self.patch_weight.grad
                self._wgrad_launch([(dpe, patches, wg.view(d, K), self.patch_bias.grad)], self._first_touch(wg),
                                   self._slabs_for(n * NP, self._tiles(d, K)))
