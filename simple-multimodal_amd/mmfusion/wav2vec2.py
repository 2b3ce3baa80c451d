"""Wav2Vec2 backbone on the HIP kernels: waveforms -> frame states; frozen by default, with the weight gradients of the top layers
and of the front end (everything above the convolutional feature extractor) where they are marked trainable, and those of the
feature extractor itself where it is.

The reference pushes every clip through HuggingFace's ``Wav2Vec2Model`` per step (reference models/encoders.py:116,144).
``NativeWav2Vec2`` is that model rebuilt from its sizes alone (nothing is fetched), with HuggingFace's ``state_dict``
surface, so published checkpoints and the reference's ``.pth`` files load.  Two families are built, by one switch with three
spellings: the base family (group-norm feature extractor without conv biases, post-LN encoder; the launch list below) and the
layer-norm family (``feat_extract_norm="layer"``, ``conv_bias=True``, ``do_stable_layer_norm=True``: "The layer-norm family"
below).  ``FAMILIES`` holds the released sizes as constructor kwargs.

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
(a longer one reallocates it once; shorter ones use its leading part).  Frozen by default, bf16 storage only, nothing
synchronises with the host (mmfusion/backbone.py).

Fine-tuning.  ``set_trainable_layers(k, front=False)`` marks the parameters of layers ``L - k .. L - 1`` trainable and, with
``k == L`` and ``front``, everything between the feature extractor and layer 0 (HuggingFace's ``freeze_feature_encoder()`` regime).
With grad mode on every call is then one ``torch.autograd.Function`` around the launch list above (the trainable parameters are
its inputs, so the result carries a graph; there is no gradient with respect to the waveform) plus one copy per walked layer: it
keeps the bf16 input of layers ``>= L - k`` and, with ``front``, ``feat``, the feature LayerNorm's input.  The backward, per chunk
and per layer top down, is the post-LN layer's (``_post_ln_layer_grad``, mmfusion/backbone.py has its rows) with

      attention backward            mmf_attn_delta_f32, then                 datt -> dqkv (delta = sum_j p_ij dp_ij in f32, not dO . O
                                    mmf_attn_bwd_grouped_delta               from the bf16 O: see below)

(the dgrad of the lowest walked layer is not launched unless the front end trains).  The attention backward is the shared MFMA one
with its delta as an input: its own delta = dO . O reads the bf16 O, so a row of dS sums to dO . (O - bf16(O)) instead of zero, an
absolute residue; where the frames of a clip have grown alike (twelve layers deep they do) dS nearly vanishes and that residue was
up to 18 times the q / k projections' exact gradients at base sizes (tests/test_w2v_finetune_gpu.py).  The d x d and d x I weight gradients take the
K-slab form where ``_slabs_for`` says so, and the key bias gets no column sum (mmfusion/backbone.py).  The front end, per chunk:
``LN(feat)``, the projection and the positional convolution are computed again (the conv stack is not, unless it trains: "The
feature encoder" below), then

      encoder LayerNorm backward    mmf_layernorm_bwd_grouped                gx -> dy
      dz = dy gelu'(b + conv(x0))   mmf_w2v_posconv_bwd_act                  the forward's MFMA loop again; db += colsum(dz)
      dW_eff += dz (*) x0           mmf_w2v_posconv_wgrad (+ mmf_sum_slabs)  f32, packed as the forward reads it, summed over the chunks
      dx0 = dy + conv^T(dz)         mmf_w2v_posconv_dgrad                    the forward's kernel on the reversed, swapped weight
      projection wgrad, dgrad       TN / NN                                  dx0 -> dfln
      feature LayerNorm backward    mmf_layernorm_bwd_grouped                for its dgamma / dbeta; dx is not kept

and once per backward ``mmf_w2v_weightnorm_bwd`` turns the summed dW_eff into the gradients of the weight norm's g and v (the
forward rounds the effective weight to bf16; the gradient passes straight through that rounding).  Gradients are added into the
parameters' f32 ``.grad`` (the arena's lazy-zero protocol as ``ops.queue_wgrad`` keeps it) in stream order.

The feature encoder.  ``set_trainable_layers(L, front=True, feature_encoder=True)`` also trains the seven convolutions and layer 0's
GroupNorm, as a ``Wav2Vec2Model`` nobody froze does.  The forward keeps nothing more (the waveform is saved already).  Per chunk,
after the front end's backward has left ``dfeat``, ``_conv_grad`` runs the conv stack again with every layer's raw output kept side
by side and walks it top down (dr_i: the gradient of layer i's raw output; it takes the place of the raw output it is formed from):

      dr_last = dfeat gelu'(r_last)  mmf_bias_gelu_bwd_bf16 (no bias)         in place on dfeat
      per layer i = last .. 1:
        win_i again                 mmf_w2v_gelu_window                      r_{i-1} -> win (i = 1: mmf_w2v_conv0_norm_gelu; i = last: still there)
        dW_i (+)= dr_i^T win_i      TN, K-slabs where _slabs_for says so     straight into the (C_out, k, C_in) parameter's .grad
        dwin_i = dr_i W_i           NN
        dr_{i-1}                    mmf_w2v_window_fold_gelu_bwd             gelu'(r_{i-1}) x the fold of dwin_i, zeros on unread frames
      layer 0                       mmf_w2v_conv0_bwd_stats                  dwin_1 -> S1 = sum dy, S2 = sum dy xhat; dgamma, dbeta
                                    mmf_w2v_conv0_bwd_wgrad                  dW0 over ALL frames (an unread one has dy = 0, not dc = 0)

No host synchronisation and no floating-point atomics in any of these; the inner conv weights' bf16 shadows are the arena's, which
the optimiser writes with the masters (tests/test_w2v_feature_encoder_gpu.py steps it and checks the next forward).

The layer-norm family (wav2vec2-large-lv60, large-960h-lv60-self, large-robust, xlsr-53, XLS-R).  Every conv layer is Conv1d(bias) ->
LayerNorm over the channels of a frame (eps 1e-5, affine) -> GELU, and the encoder is HuggingFace's ``Wav2Vec2EncoderStableLayerNorm``:
nothing behind the positional convolution, pre-LN layers, ``encoder.layer_norm`` on top.  Launch list for a chunk:

    conv 0 + bias + LN + GELU     mmf_w2v_conv0_ln_gelu                wave -> window form of layer 1, one pass, no statistics
    conv layer i >= 1             mmf_gemm_grouped NT, BIAS            window -> raw (n T_i, C_i)
    LN + GELU + next window       mmf_w2v_ln_gelu_window               raw -> window form of layer i + 1 (k = 0 behind the last layer: in place)
    LayerNorm(conv_dim), projection + bias                             as above; the projection lands in ``y``
    x + gelu(pos_conv(x) + b)     mmf_w2v_posconv                      y -> x, layer 0's input
    per pre-LN layer (``_pre_ln_layer``, mmfusion/backbone.py: ViT's):
      LayerNorm                                                        x  -> ln
      _attention(ln, + x)                                              ln -> qkv -> att -> y
      LayerNorm                                                        y  -> ln
      _ffn(ln, + y)                                                    ln -> h -> x
    encoder.layer_norm, widening cast                                  x  -> y -> result

bf16 is stored where the table has an arrow: layer 0 after its GELU, each raw conv output after the bias, each LN + GELU output, then
as the base family.  The C_i / 8 lanes that own a frame reduce its statistics among themselves (csrc/wav2vec2.hip), so C_i / 8 must
be a power of two up to 256.  Fine-tuning is HuggingFace's ``freeze_feature_encoder()`` regime: ``set_trainable_layers(k)`` trains
the top ``k`` layers and, from ``k = 1`` on, ``encoder.layer_norm`` above them; ``front=True`` (``k == L``) adds the feature
projection, its LayerNorm and the positional convolution.  The forward also keeps the input of ``encoder.layer_norm``; the backward
starts with that LayerNorm's, walks ``_pre_ln_layer_grad`` (ViT's layer backward, with this class's exact-delta attention backward,
K-slab weight gradients and no column sum for the key bias; a pre-LN layer's Q/K/V input gradient is always formed, since its first
LayerNorm's own gradients come out of it) and ends in the front end's backward above without the encoder LayerNorm.  Refused on this
family, each with a ``ValueError``: ``feature_encoder=True`` (the backward of the LayerNorm over channels is not built), any
regulariser above 0, and every mixed setting of the three switches (no released checkpoint has one).

Regularisers.  HuggingFace's model in ``train()`` masks time spans with ``masked_spec_embed``, drops at seven kinds of place and
skips layers, and the reference trains it that way; here they are opt-in (``set_regularisation``, all off by default) and act only in a
differentiable call in ``train()`` mode.  Such a call takes 3 + 4 L sites from ``ops.next_site()`` (``_Reg``) in HuggingFace's order:

    1  feature-projection dropout   mmf_w2v_mask_drop (in place, with 2)   x = in_span ? bf16(masked_spec_embed) : keep ? proj c : 0
    2  the time mask's spans        mmf_w2v_mask_spans, once per call      (N, slots) int32 span starts for the whole batch
    3  after encoder.layer_norm     mmf_hidden_dropout (in place)          x = dropout(LayerNorm(y))
    per layer: attention probabilities (mmf_attn_fwd_grouped_keyed), attention output and MLP output (NT, BIAS then
    mmf_hidden_dropout with the residual: ``_closing``'s ``join``), GELU output (mmf_bias_gelu_drop_bf16_to: ``_ffn``'s ``act``)

The keying (state, site, clip [* H + head], element), and why results do not depend on ``chunk``, is mmfusion/backbone.py's
("Training-mode dropout").  The backward draws the masks again: ``mmf_attn_delta_f32_keyed`` + ``mmf_attn_bwd_grouped_delta_keyed``, ``mmf_bias_gelu_drop_bwd_bf16``, the gradient
forms of the two streaming kernels, and ``mmf_w2v_mask_embed_grad`` + ``mmf_sum_slabs_f32`` for ``masked_spec_embed``'s gradient (a
fixed-order sum).  LayerDrop is a host draw per layer and call; a skipped layer launches nothing ("Regularisers").
"""
from __future__ import annotations

import types
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BF16, BackboneOutput, FrozenBackbone, WsTable, _CallDropout, _check_probability
from .lib import EPI_BIAS, GEMM_NN, GEMM_NT

# clips per pass through the workspace: 16 clips of 10 s give the layer GEMMs 7984 rows.  NOT chosen by measurement yet:
# tools/w2v_bench.py --chunks is the sweep that should decide it
DEFAULT_CHUNK = 16
POS_WGRAD_BLOCK = 128                      # time rows per unit of mmf_w2v_posconv_wgrad (WG_TT of csrc/wav2vec2.hip)
POS_WGRAD_TAPS = 8                         # taps per workgroup of it
POS_GROUP_WIDTHS = (16, 32, 48, 64)        # the forms of mmf_w2v_posconv

# constructor kwargs of the released families.  "large-lv60" is the layer-norm family (wav2vec2-large-lv60, large-960h-lv60-self,
# large-robust, xlsr-53, the XLS-R models): ``config.audio_backbone_kwargs = FAMILIES["large-lv60"]``
_LARGE = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)
FAMILIES = {
    "base": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072),
    "large": dict(_LARGE),
    "large-lv60": dict(_LARGE, feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True),
}

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


REG_NAMES = ("hidden_dropout", "attention_dropout", "activation_dropout", "feat_proj_dropout", "layerdrop", "mask_time_prob",
             "mask_time_length", "mask_time_min_masks")
# wav2vec2-base-960h's training regime
REG_960H = dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, layerdrop=0.1,
                mask_time_prob=0.05, mask_time_length=10, mask_time_min_masks=2)


def span_count(num: int, T: int, length: int, min_masks: int) -> int:
    """the spans of a clip of ``T`` frames for a drawn count ``num``: HuggingFace's ``_compute_mask_indices`` without an attention
    mask (``w2v_span_count`` of csrc/wav2vec2.hip)"""
    num = max(num, min_masks)
    if num * length > T:
        num = T // length
    return max(min(num, T - (length - 1)), 0)


def span_slots(T: int, prob: float, length: int, min_masks: int) -> int:
    """the slots per clip of the span table: the most spans ``mmf_w2v_mask_spans`` can draw, int(prob T / length) + 1 finished"""
    return max(1, span_count(int(prob * T / length) + 1, T, length, min_masks))


class _Reg(_CallDropout):
    """The regularisers of one differentiable training call (mmfusion/backbone.py).  Its 3 + 4 L sites in HuggingFace's call order:
    the feature projection's dropout, the time-mask draw, the dropout after ``encoder.layer_norm``, then per layer the attention
    probabilities, the attention output, the GELU output and the MLP output, whether or not LayerDrop skips the layer.
    What the call keeps beside them: ``starts`` (N, slots) int32, the time mask's span starts (drawn here, once, for the whole batch),
    and ``skip``, LayerDrop's decision per layer (drawn by the host before the chunk loop, so every chunk agrees)."""
    PROBS, OUT, ACT, MLP = range(4)

    def __init__(self, c, N: int, T: int, dev, skip: List[bool]):
        super().__init__(c.hidden_dropout, c.attention_dropout, 3, c.num_hidden_layers)
        self.p_act, self.p_fp = c.activation_dropout, c.feat_proj_dropout
        self.H, self.length, self.skip = c.num_attention_heads, c.mask_time_length, skip
        self.fp, self.mask, self.enc = self.lead
        self.starts = None
        if c.mask_time_prob > 0.0:
            self.starts = torch.empty((N, span_slots(T, c.mask_time_prob, c.mask_time_length, c.mask_time_min_masks)), dtype=torch.int32,
                                      device=dev)
            lib.w2v_mask_spans(self.starts, T, c.mask_time_prob, c.mask_time_length, c.mask_time_min_masks, ops.rng_state(), self.mask, 0)

    @property
    def front(self) -> bool:
        """whether the projection's output is masked or dropped"""
        return self.starts is not None or self.p_fp > 0.0

    def spans(self, n0: int, n: int) -> Optional[torch.Tensor]:
        return None if self.starts is None else self.starts[n0:n0 + n]

    def feat_proj(self, item0: int) -> tuple:
        return self.key(self.p_fp, self.fp, item0)

    def probs(self, i: int, item0: int) -> Optional[tuple]:
        """the attention's (p, state, site, stream base): stream id = clip * H + head over the whole batch"""
        return self.key(self.p_a, self.layers[i][self.PROBS], item0 * self.H) if self.p_a > 0.0 else None

    def act(self, i: int, item0: int) -> Optional[tuple]:
        return self.key(self.p_act, self.layers[i][self.ACT], item0) if self.p_act > 0.0 else None


class _Differentiable(torch.autograd.Function):
    """``NativeWav2Vec2._launches``, differentiable with respect to the trainable parameters (``params``; never to the waveform).
    They are inputs so that the result carries a graph; their gradients are not returned but added into their f32 ``.grad`` by the
    backward's own launches, as ``ops.queue_wgrad``'s are.  ``reg``: the call's regularisers or None."""

    @staticmethod
    def forward(ctx, model: "NativeWav2Vec2", wave: torch.Tensor, reg: Optional[_Reg], *params) -> torch.Tensor:
        c = model.config
        N, T, L = wave.shape[0], model.frames(wave.shape[1]), c.num_hidden_layers
        first = L - model.trainable_layers                             # the lowest layer the backward walks
        keep = model._keep(first, N * T, wave.device)
        feat = torch.empty((N * T, c.conv_dim[-1]), dtype=BF16, device=wave.device) if model.trainable_front else None
        final = torch.empty((N * T, c.hidden_size), dtype=BF16, device=wave.device) if model._ln_family else None
        pos_w = model._pos_weight()
        out = model._launches(wave, pos_w, keep, first, feat, reg, final)
        ctx.model, ctx.first, ctx.front, ctx.pos_w, ctx.reg = model, first, model.trainable_front, pos_w, reg
        ctx.feature_encoder = model.trainable_feature_encoder
        ctx.save_for_backward(wave, keep, *(t for t in (feat, final) if t is not None))
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        wave, keep, *rest = ctx.saved_tensors
        if any(ctx.needs_input_grad[3:]):
            feat = rest.pop(0) if ctx.front else None
            ctx.model._backward(wave, keep, feat, ctx.first, ctx.pos_w, dout.contiguous(), ctx.reg, ctx.feature_encoder,
                                rest[0] if rest else None)
        return (None,) * len(ctx.needs_input_grad)


class NativeWav2Vec2(FrozenBackbone):
    """HuggingFace ``Wav2Vec2Model`` (no attention mask), defaults = wav2vec2-base; ``feat_extract_norm="layer"``, ``conv_bias=True`` and
    ``do_stable_layer_norm=True`` together: the layer-norm family (``FAMILIES["large-lv60"]``).

    ``forward(input_values)`` -> ``.last_hidden_state`` (N, T, hidden) f32; ``input_values``: (N, L) f32 on the GPU.
    Frozen by default; after ``set_trainable_layers(k)``, ``k > 0``, a call in grad mode carries the top ``k`` layers' weight
    gradients (never a gradient with respect to ``input_values``).
    ``state_dict()`` has the keys, shapes and order of ``Wav2Vec2Model``; ``load_state_dict`` also takes the older weight-norm
    names (``weight_g`` / ``weight_v``).  Q/K/V are stored fused, the inner conv weights as ``(C_out, k, C_in)`` (the GEMM's
    operand), and split / permuted on the way.  ``masked_spec_embed`` is read only where SpecAugment's time mask is on
    (``set_regularisation``; the training-mode regularisers are off by default)."""

    def __init__(self, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, conv_dim: Sequence[int] = (512,) * 7,
                 conv_kernel: Sequence[int] = (10, 3, 3, 3, 3, 2, 2), conv_stride: Sequence[int] = (5, 2, 2, 2, 2, 2, 2),
                 conv_bias: bool = False, num_conv_pos_embeddings: int = 128, num_conv_pos_embedding_groups: int = 16,
                 layer_norm_eps: float = 1e-5, feat_extract_norm: str = "group", do_stable_layer_norm: bool = False,
                 in_channels: int = 1, chunk: int = DEFAULT_CHUNK, hidden_dropout: float = 0.0, attention_dropout: float = 0.0,
                 activation_dropout: float = 0.0, feat_proj_dropout: float = 0.0, layerdrop: float = 0.0, mask_time_prob: float = 0.0,
                 mask_time_length: int = 10, mask_time_min_masks: int = 2, mask_feature_prob: float = 0.0):
        d, H, I = int(hidden_size), int(num_attention_heads), int(intermediate_size)
        dims, ks, ss = tuple(int(v) for v in conv_dim), tuple(int(v) for v in conv_kernel), tuple(int(v) for v in conv_stride)
        pk, pg = int(num_conv_pos_embeddings), int(num_conv_pos_embedding_groups)
        who = "NativeWav2Vec2"
        if feat_extract_norm not in ("group", "layer"):
            raise ValueError(f"{who}: feat_extract_norm={feat_extract_norm!r}: 'group' (the base family) or 'layer'")
        switches = (feat_extract_norm == "layer", bool(do_stable_layer_norm), bool(conv_bias))
        if any(switches) != all(switches):
            raise ValueError(f"{who}: feat_extract_norm={feat_extract_norm!r}, do_stable_layer_norm={do_stable_layer_norm!r}, "
                             f"conv_bias={conv_bias!r}: the layer-norm family (large-lv60, XLS-R) sets all three ('layer', True, "
                             "True) and the base family none; no mixed setting is built (no released checkpoint has one)")
        ln_family = all(switches)
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
        if ln_family and any(c > 2048 or (c // 8) & (c // 8 - 1) for c in dims):
            raise ValueError(f"{who}: conv_dim {dims}: the layer-norm family's LayerNorm over channels takes 8 times a power of two, "
                             "8 .. 2048 channels")
        kp = (pk * cg + 31) // 32 * 32
        if cg not in POS_GROUP_WIDTHS or pk < 1 or (127 * cg + kp) * 2 > 65536:
            raise ValueError(f"{who}: positional convolution with group width {cg} (one of {POS_GROUP_WIDTHS}) and kernel {pk} has no "
                             "kernel form (its LDS image must fit 64 KiB)")
        if num_hidden_layers < 1 or chunk < 1:
            raise ValueError(f"{who}: layers and chunk at least 1")
        self.config = types.SimpleNamespace(
            hidden_size=d, num_hidden_layers=int(num_hidden_layers), num_attention_heads=H, intermediate_size=I, conv_dim=dims,
            conv_kernel=ks, conv_stride=ss, conv_bias=ln_family, num_conv_pos_embeddings=pk, num_conv_pos_embedding_groups=pg,
            layer_norm_eps=float(layer_norm_eps), feat_extract_norm="layer" if ln_family else "group", do_stable_layer_norm=ln_family, hidden_act="gelu",
            feat_extract_activation="gelu", num_feat_extract_layers=len(dims), model_type="wav2vec2")
        self.pos_cg, self.pos_kp = cg, kp
        self._ln_family = ln_family
        add = self._add
        add("masked_spec_embed", (d,), "masked_spec_embed", std=1.0)
        fe = "feature_extractor.conv_layers."
        add("conv0_w", (dims[0], 1, ks[0]), fe + "0.conv.weight", std=0.3)
        if ln_family:
            add("conv0_b", (dims[0],), fe + "0.conv.bias", std=0.0)
        add("conv0_gn_w", (dims[0],), fe + "0.layer_norm.weight", ones=True)       # (the layer-norm family's LayerNorm of layer 0 as well)
        add("conv0_gn_b", (dims[0],), fe + "0.layer_norm.bias", std=0.0)
        for i in range(1, len(dims)):
            add(f"conv{i}_w", (dims[i], ks[i], dims[i - 1]), f"{fe}{i}.conv.weight", std=(dims[i - 1] * ks[i]) ** -0.5, swapped=True)
            if ln_family:
                add(f"conv{i}_b", (dims[i],), f"{fe}{i}.conv.bias", std=0.0)
                add(f"conv{i}_ln_w", (dims[i],), f"{fe}{i}.layer_norm.weight", ones=True)
                add(f"conv{i}_ln_b", (dims[i],), f"{fe}{i}.layer_norm.bias", std=0.0)
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
        self._front = False                            # set_trainable_layers(L, front=True)
        self._feature_encoder = False                  # set_trainable_layers(L, front=True, feature_encoder=True)
        self.layerdrop_generator = torch.Generator()   # LayerDrop's host draws (CPU; seed it to fix the skip pattern)
        if mask_feature_prob != 0:
            raise ValueError(f"{who}: mask_feature_prob={mask_feature_prob!r}: masking along the feature axis is not built (no released "
                             "base checkpoint sets it)")
        self.config.mask_feature_prob = 0.0
        self.set_regularisation(hidden_dropout=hidden_dropout, attention_dropout=attention_dropout, activation_dropout=activation_dropout,
                                feat_proj_dropout=feat_proj_dropout, layerdrop=layerdrop, mask_time_prob=mask_time_prob,
                                mask_time_length=mask_time_length, mask_time_min_masks=mask_time_min_masks)

    # -- fine-tuning --------------------------------------------------------------------------------------
    _FRONT_PARAMS = ("fp_ln_w", "fp_ln_b", "fp_w", "fp_b", "pos_b", "pos_g", "pos_v", "enc_ln_w", "enc_ln_b")

    @property
    def trainable_front(self) -> bool:
        return self._front

    @property
    def trainable_feature_encoder(self) -> bool:
        return self._feature_encoder

    def _feature_params(self) -> list:
        """the feature extractor's parameters: layer 0's convolution and GroupNorm, then the inner convolutions"""
        return ["conv0_w", "conv0_gn_w", "conv0_gn_b"] + [f"conv{i}_w" for i in range(1, len(self.config.conv_dim))]

    def _trainable_names(self) -> list:
        """the parameters that require a gradient, in the order the differentiable forward takes them"""
        L, k = self.config.num_hidden_layers, self._trainable
        front = list(self._FRONT_PARAMS) + (["masked_spec_embed"] if self.config.mask_time_prob > 0.0 else []) if self._front else []
        layers = [n for i in range(L - k, L) for n in self._layer_params(i)]
        if self._ln_family:                    # encoder.layer_norm sits on top of the layers: it trains with the first of them
            top = ("enc_ln_w", "enc_ln_b")
            return [n for n in front if n not in top] + layers + (list(top) if k else [])
        return (self._feature_params() if self._feature_encoder else []) + front + layers

    # -- training-mode regularisers ------------------------------------------------------------------------
    def set_regularisation(self, **settings) -> None:
        """HuggingFace's training-mode regularisers, under its names (``REG_NAMES``; the ones not given keep their values, all 0 /
        off at construction): ``hidden_dropout`` (after ``encoder.layer_norm`` and on every layer's attention and MLP outputs),
        ``attention_dropout`` (the attention probabilities), ``activation_dropout`` (the GELU output), ``feat_proj_dropout`` (the
        feature projection's output), each a probability in [0, 1); ``layerdrop``, the probability in [0, 1) of skipping a layer;
        SpecAugment's time mask ``mask_time_prob`` in [0, 1] with ``mask_time_length`` >= 1 and ``mask_time_min_masks`` >= 0
        (``config.apply_spec_augment`` says whether it is on).  ``REG_960H`` holds wav2vec2-base-960h's values.  They act only in
        a call of the differentiable route (``trainable_layers > 0``, grad mode on) in ``train()`` mode; every other call is the plain
        launch list.  Masking along the feature axis (``mask_feature_prob``) is not built.  ``masked_spec_embed`` trains exactly
        when the front end does and ``mask_time_prob`` is above 0."""
        who, c = "NativeWav2Vec2.set_regularisation", self.config
        unknown = sorted(set(settings) - set(REG_NAMES))
        if "mask_feature_prob" in unknown and settings["mask_feature_prob"] == 0:
            unknown.remove("mask_feature_prob")
        if unknown:
            raise ValueError(f"{who}: {unknown} not built or not known (the settings are {', '.join(REG_NAMES)})")
        new = {n: settings.get(n, getattr(c, n, 10 if n == "mask_time_length" else 2 if n == "mask_time_min_masks" else 0.0)) for n in REG_NAMES}
        for n in REG_NAMES[:5]:
            _check_probability(who, n, new[n])
        _check_probability(who, "mask_time_prob", new["mask_time_prob"], closed=True)
        for n, low in (("mask_time_length", 1), ("mask_time_min_masks", 0)):
            v = new[n]
            if isinstance(v, bool) or not isinstance(v, int) or v < low:
                raise ValueError(f"{who}({n}={v!r}): an integer of at least {low}")
        on = [n for n in REG_NAMES[:6] if new[n] > 0.0]
        if self._ln_family and on:
            raise ValueError(f"{who}({', '.join(f'{n}={new[n]!r}' for n in on)}): the training-mode regularisers are not built for the "
                             "layer-norm family (feat_extract_norm='layer'); they stay at 0 there")
        for n in REG_NAMES:
            setattr(c, n, float(new[n]) if n not in ("mask_time_length", "mask_time_min_masks") else new[n])
        c.apply_spec_augment = c.mask_time_prob > 0.0
        self._require_grad(self._trainable_names())

    def _reg_of_call(self, N: int, T: int, dev) -> Optional[_Reg]:
        """the regularisers of the differentiable call that is about to run: None unless the module trains with a setting above 0.
        LayerDrop is HuggingFace's ``torch.rand([]) < layerdrop`` per layer, drawn on the host from
        ``layerdrop_generator``: no device synchronisation, but a graph capture would freeze the pattern, so it is refused there"""
        c = self.config
        if not self.training or not any(getattr(c, n) > 0.0 for n in REG_NAMES[:6]):
            return None
        if c.mask_time_prob > 0.0 and c.mask_time_length > T:             # (HuggingFace's _compute_mask_indices raises as well)
            raise ValueError(f"NativeWav2Vec2: mask_time_length {c.mask_time_length} is longer than the clip's {T} frames")
        L = c.num_hidden_layers
        skip = [False] * L
        if c.layerdrop > 0.0:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("NativeWav2Vec2: layerdrop > 0 draws its skip pattern on the host, which a graph capture would freeze "
                                   "into every replay; capture with layerdrop = 0 (the other regularisers draw new masks on every replay)")
            skip = [bool(torch.rand([], generator=self.layerdrop_generator).item() < c.layerdrop) for _ in range(L)]
        self._own_training_forward()
        return _Reg(c, N, T, dev, skip)

    def set_trainable_layers(self, k: int, front: bool = False, feature_encoder: bool = False) -> None:
        """The parameters of the top ``k`` layers (``L - k .. L - 1``) get ``requires_grad = True``, every other parameter
        ``False``; 0 freezes the backbone again.  ``front=True`` (with ``k == L`` only: the gradient reaches the front end through
        every layer) also trains ``feature_projection.layer_norm`` and ``.projection``, the positional convolution's ``bias`` and
        its weight norm's ``g`` / ``v`` (``parametrizations.weight.original0`` / ``original1``) and ``encoder.layer_norm``: the
        regime of HuggingFace's ``freeze_feature_encoder()``.  ``feature_encoder=True`` (with ``k == L`` and ``front`` only: the
        gradient reaches the convolutions through the front end) also trains the feature extractor, ``conv0_w``, layer 0's
        GroupNorm and every inner convolution: the regime of a ``Wav2Vec2Model`` nobody froze (the reference's).
        ``masked_spec_embed`` trains with the front end where the time mask is on
        (``mask_time_prob > 0``, ``set_regularisation``) and is frozen otherwise.  With grad mode on and ``k > 0``, ``forward``
        returns a result that carries a graph; its backward adds those parameters' gradients into their f32 ``.grad`` (the module's
        parameter arena) and stops below layer ``L - k``.  There is no gradient with respect to the waveform; SpecAugment's time
        mask, the backbone's dropout and LayerDrop are ``set_regularisation``'s (off by default); the fp32 parity mode is refused as
        everywhere in this class."""
        self._check_trainable(k, "front", front, "the front end trains", "its gradient comes through every layer")
        self._check_trainable(k, "feature_encoder", feature_encoder, "the feature encoder trains", "its gradient comes through every layer")
        if feature_encoder and not front:
            raise ValueError(f"NativeWav2Vec2: set_trainable_layers({k!r}, front={front!r}, feature_encoder={feature_encoder!r}): the "
                             "feature encoder trains with the front end only (its gradient comes through the front end)")
        if feature_encoder and self._ln_family:
            raise ValueError(f"NativeWav2Vec2: set_trainable_layers({k!r}, front={front!r}, feature_encoder=True): the layer-norm family's "
                             "feature encoder does not train (the backward of its LayerNorm over channels is not built); "
                             "HuggingFace's freeze_feature_encoder() regime, front=True, is")
        if feature_encoder != self._feature_encoder:
            self._gws = None                                              # the backward's table changes (``_grad_table``)
        self._trainable, self._front, self._feature_encoder = k, front, feature_encoder
        self._require_grad(self._trainable_names())

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
        table = [("win", win, BF16), ("raw", raw, BF16)] + self._token_table(T, T * c.intermediate_size)
        if self._ln_family:                    # layer 0 is one pass: no statistics
            return table
        return table + [("stats", 2 * c.conv_dim[0], torch.float32), ("partial", lib.W2V_STATS_SLOTS * 2 * c.conv_dim[0], torch.float32)]

    def workspace_bytes_per_clip(self, L: int) -> int:
        return self._bytes_per_item(self._ws_table(L))

    # -- weights ----------------------------------------------------------------------------------------
    def _pos_weight(self, transposed: bool = False) -> torch.Tensor:
        """The positional convolution's effective weight g v / ||v|| (norm over dims (0, 1) per tap, ``weight_norm(dim=2)``),
        folded in f32, repacked to (groups, cg, Kp) column (tap, channel) and rounded to bf16.  ``transposed``: the operand of the
        input gradient instead, taps reversed and co / ci swapped within each group: [g][ci][j * cg + co] = w[g cg + co][ci][k - 1 - j].
        Once per weight version while the front end is frozen; in every call while it trains (the optimiser writes the masters
        through raw pointers, which moves no version counter, so nothing derived from a trainable weight may be cached)"""
        def build():
            g, v = self._f("pos_g"), self._f("pos_v")
            w = g * v / v.norm(dim=(0, 1), keepdim=True)                                          # (C, cg, k)
            C, cg, k = w.shape
            packed = torch.zeros(C, self.pos_kp, dtype=BF16, device=w.device)
            if transposed:
                w = w.view(C // cg, cg, cg, k).flip(3).permute(0, 2, 3, 1)                        # (groups, ci, reversed tap, co)
            else:
                w = w.permute(0, 2, 1)
            packed[:, :k * cg] = w.reshape(C, k * cg).to(BF16)
            return packed
        if self._front:
            with torch.no_grad():
                return build()
        return self._derived("pos_wt16" if transposed else "pos_w16", ("pos_g", "pos_v"), build)

    # -- launches ---------------------------------------------------------------------------------------
    def _features(self, ws, wave: torch.Tensor, n: int, Ts: List[int], raws: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """the feature extractor: wave (n, L) f32 -> (n * T, conv_dim[-1]) bf16 after the last layer's GELU.  With ``raws`` (the
        backward's recompute; ``raws[i]``: (n T_i, conv_dim[i]) bf16) every layer's raw output goes to its own buffer and stays
        there: the last layer's GELU is not applied, and ``win`` is left holding the last layer's window form"""
        c = self.config
        dims, ks, ss = c.conv_dim, c.conv_kernel, c.conv_stride
        if self._ln_family:
            return self._features_ln(ws, wave, n, Ts)
        w0 = self._f("conv0_w")
        lib.w2v_conv0_stats(wave, w0, ws["stats"], ws["partial"], ks[0], ss[0])
        lib.w2v_conv0_norm_gelu(wave, w0, ws["stats"], self._f("conv0_gn_w"), self._f("conv0_gn_b"), ws["win"], ks[0], ss[0],
                                ks[1], ss[1], 1e-5)                                   # (nn.GroupNorm's own eps, not layer_norm_eps)
        last = len(dims) - 1
        for i in range(1, last + 1):
            rows, K = n * Ts[i], ks[i] * dims[i - 1]
            win, raw = self._rows(ws, "win", rows, K), self._rows(ws, "raw", rows, dims[i]) if raws is None else raws[i]
            ops.gemm(GEMM_NT, win, self._w(f"conv{i}_w").view(dims[i], K), raw)
            if i < last:
                lib.w2v_gelu_window(raw, ws["win"], n, Ts[i], dims[i], ks[i + 1], ss[i + 1])
            elif raws is None:
                lib.bias_gelu(raw)
        return raw

    def _features_ln(self, ws, wave: torch.Tensor, n: int, Ts: List[int]) -> torch.Tensor:
        """``_features`` of the layer-norm family: every layer is conv + bias -> LayerNorm over channels -> GELU (nn.LayerNorm's
        own eps, 1e-5, not layer_norm_eps).  Layer 0 in one pass, an inner layer's bias in its GEMM's epilogue and its LayerNorm
        and GELU on the way into the next window form; behind the last layer in place"""
        c = self.config
        dims, ks, ss, last = c.conv_dim, c.conv_kernel, c.conv_stride, len(c.conv_dim) - 1
        lib.w2v_conv0_ln_gelu(wave, self._f("conv0_w"), self._f("conv0_b"), self._f("conv0_gn_w"), self._f("conv0_gn_b"), ws["win"],
                              ks[0], ss[0], ks[1], ss[1], 1e-5)
        for i in range(1, last + 1):
            rows, K = n * Ts[i], ks[i] * dims[i - 1]
            win, raw = self._rows(ws, "win", rows, K), self._rows(ws, "raw", rows, dims[i])
            ops.gemm(GEMM_NT, win, self._w(f"conv{i}_w").view(dims[i], K), raw, bias=self._f(f"conv{i}_b"), epilogue=EPI_BIAS)
            k, s = (ks[i + 1], ss[i + 1]) if i < last else (0, 1)
            lib.w2v_ln_gelu_window(raw, self._f(f"conv{i}_ln_w"), self._f(f"conv{i}_ln_b"), ws["win"] if k else raw, n, Ts[i], dims[i], k, s, 1e-5)
        return raw

    def forward(self, input_values: torch.Tensor, attention_mask=None) -> BackboneOutput:
        if attention_mask is not None:
            raise NotImplementedError("NativeWav2Vec2: attention_mask is not implemented (the reference never passes one)")
        self._check_input(input_values, "input_values")
        if input_values.dim() != 2:
            raise ValueError(f"NativeWav2Vec2: input_values {tuple(input_values.shape)} is not (N, L)")
        if self.frames(input_values.shape[1]) < 1:
            raise ValueError(f"NativeWav2Vec2: {input_values.shape[1]} samples are shorter than the feature extractor's receptive field")
        wave = input_values.contiguous()
        _arena.ensure(self)
        if torch.is_grad_enabled() and self._trainable > 0:
            reg = self._reg_of_call(wave.shape[0], self.frames(wave.shape[1]), wave.device)
            return BackboneOutput(_Differentiable.apply(self, wave.detach(), reg, *(getattr(self, n) for n in self._trainable_names())))
        return BackboneOutput(self._launches(wave, self._pos_weight()))

    def _front_end(self, ws, feat: torch.Tensor, pos_w: torch.Tensor, n: int, T: int, st=None, reg: Optional[_Reg] = None,
                   n0: int = 0) -> None:
        """feat (n T, conv_dim[-1]) -> the feature LayerNorm (into ``win``; statistics into ``st``, None: the workspace's), the
        projection (``x``) and the positional convolution (``y``; the layer-norm family: the other way round).  With ``reg`` (``n0``: the chunk's first clip in the batch) the
        projection's output is dropped and the time mask's rows set to ``masked_spec_embed``, in place, in front of the convolution"""
        c, d, rows = self.config, self.config.hidden_size, n * T
        x, y, fln = self._rows(ws, "x", rows, d), self._rows(ws, "y", rows, d), self._rows(ws, "win", rows, feat.shape[1])
        if self._ln_family:                    # no LayerNorm behind the convolution: its output is layer 0's input, ``x``
            x, y = y, x
        self._ln(ws if st is None else st, feat, fln, "fp_ln_w", "fp_ln_b")
        ops.gemm(GEMM_NT, fln, self._w("fp_w"), x, bias=self._f("fp_b"), epilogue=EPI_BIAS)
        if reg is not None and reg.front:
            lib.w2v_mask_drop(x, x, n, T, reg.length, reg.feat_proj(n0), reg.spans(n0, n), self._f("masked_spec_embed"))
        lib.w2v_posconv(x, pos_w, self._f("pos_b"), y, n, T, d, c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings)

    def _hooks(self, i: int, ws, n: int, T: int, n0: int, reg: Optional[_Reg]) -> tuple:
        """layer ``i``'s (attend, join, join_bwd, act) for a chunk of ``n`` clips from clip ``n0`` under ``reg``: the attention with
        dropped probabilities, hidden dropout fused with the residual add and its gradient form, the GELU with activation dropout
        and its backward; None where the setting is 0 (the plain launch).  join / join_bwd: ``_hidden_joins``"""
        if reg is None:
            return None, None, None, None
        attend = act = None
        probs, drop = reg.probs(i, n0), reg.act(i, n0)
        if probs is not None:
            def attend(qkv: torch.Tensor, att: torch.Tensor) -> None:
                lib.attn_fwd_grouped_keyed([self._attn_problem(ws, qkv, att, n, T, T)], self.head_dim, self.head_dim ** -0.5, probs)
        join, join_bwd = self._hidden_joins(reg, reg.join_sites(i), n, n0)
        if drop is not None:
            act = (lambda h, b, g: lib.bias_gelu_drop_to(h, b, g, n, drop), lambda dg, h, b, dh: lib.bias_gelu_drop_bwd(dg, h, b, dh, n, drop))
        return attend, join, join_bwd, act

    def _launches(self, wave: torch.Tensor, pos_w: torch.Tensor, keep: Optional[torch.Tensor] = None, first: int = 0,
                  feat_keep: Optional[torch.Tensor] = None, reg: Optional[_Reg] = None, final: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the launch list on checked inputs -> (N, T, d) f32.  The differentiable call's: ``keep`` (layers - first, N T, d) bf16
        also takes a copy of the input of every layer from ``first`` up, ``feat_keep`` (N T, conv_dim[-1]) one of the feature
        LayerNorm's input; ``reg``: the call's regularisers (a layer LayerDrop skips launches nothing and keeps nothing); ``final``
        (N T, d), the layer-norm family: one of the input of ``encoder.layer_norm``, which sits behind the last layer there"""
        c = self.config
        N, L = wave.shape
        Ts = feat_lengths(L, c.conv_kernel, c.conv_stride)
        T, d = Ts[-1], c.hidden_size
        ws = self._workspace(wave.device, L)
        out = torch.empty((N, T, d), dtype=torch.float32, device=wave.device)
        for n0, n in self._chunks(N):
            rows = n * T
            feat = self._features(ws, wave[n0:n0 + n], n, Ts)
            if feat_keep is not None:
                feat_keep[n0 * T:n0 * T + rows].copy_(feat)
            x, y = self._rows(ws, "x", rows, d), self._rows(ws, "y", rows, d)
            self._front_end(ws, feat, pos_w, n, T, None, reg, n0)
            if not self._ln_family:
                self._ln(ws, y, x, "enc_ln_w", "enc_ln_b")
            if reg is not None and reg.p_h > 0.0:
                lib.hidden_dropout(x, x, n, reg.hidden(reg.enc, n0))
            for i in range(c.num_hidden_layers):
                if reg is not None and reg.skip[i]:
                    continue
                if keep is not None and i >= first:
                    keep[i - first, n0 * T:n0 * T + rows].copy_(x)
                if self._ln_family:
                    self._pre_ln_layer(i, ws, n, T)
                    continue
                attend, join, _, act = self._hooks(i, ws, n, T, n0, reg)
                self._post_ln_layer(i, ws, n, T, attend, join, act)
            if self._ln_family:
                if final is not None:
                    final[n0 * T:n0 * T + rows].copy_(x)
                self._ln(ws, x, y, "enc_ln_w", "enc_ln_b")
                x = y
            self._widen(x, out[n0:n0 + n])
        return out

    # -- the backward: the trainable layers' and the front end's weight gradients ---------------------------------------
    def _grad_table(self, L: int) -> WsTable:
        """what the backward holds beside the forward workspace, per clip of ``L`` samples: the layers' part (``_grad_rows``; the
        front end's dz takes ``dqkv``'s place) and the two conv_dim[-1]-wide gradients around the feature LayerNorm.  lse is the
        forward workspace's.  While the feature encoder trains, also every inner conv layer's raw output side by side (``raws``; a
        layer's gradient takes its raw output's place once that has been read), one window-form gradient (``dwin``) and layer
        0's two sums per channel (``bsums``)"""
        c = self.config
        T, cd = self.frames(L), c.conv_dim[-1]
        table = self._grad_rows(T, "ln2" if self._ln_family else "y2") + [("dfln", T * cd, BF16), ("dfeat", T * cd, BF16)]
        if self._feature_encoder:
            Ts = feat_lengths(L, c.conv_kernel, c.conv_stride)
            inner = range(1, len(Ts))
            table += [("raws", sum(Ts[i] * c.conv_dim[i] for i in inner), BF16),
                      ("dwin", max(Ts[i] * c.conv_kernel[i] * c.conv_dim[i - 1] for i in inner), BF16),
                      ("bsums", 2 * c.conv_dim[0], torch.float32)]
        return table

    def grad_workspace_bytes_per_clip(self, L: int) -> int:
        return self._bytes_per_item(self._grad_table(L))

    def _grad_scratch(self) -> Tuple[int, Dict[str, int]]:
        """the LayerNorm backward's scratch at the wider of its two widths; ``dpos``: the positional weight's f32 gradient in the
        packed layout, summed over a backward's chunks; ``junk`` also takes the column sums of the conv layers' weight-gradient
        launches (they have no bias), so it is as wide as the widest of them"""
        d, extra = super()._grad_scratch()
        return max(d, self.config.conv_dim[-1]), {**extra, "junk": max(d, *self.config.conv_dim), "dpos": d * self.pos_kp}

    def _pos_wgrad_slabs(self, n: int, T: int) -> int:
        """The slab count of ``mmf_w2v_posconv_wgrad`` on a chunk of ``n`` clips: its grid is (tap blocks, groups) workgroups of
        256 threads, two of which fit a CU; where that leaves CUs idle the (clip, time block) units are cut into as many runs as
        bring it to two rounds of the CUs, each at least 4 units long"""
        c = self.config
        cus = lib.load().mmf_device_cu_count()
        cus = cus if cus > 0 else 256
        wgs = c.num_conv_pos_embedding_groups * ((c.num_conv_pos_embeddings + POS_WGRAD_TAPS - 1) // POS_WGRAD_TAPS)
        units = n * ((T + POS_WGRAD_BLOCK - 1) // POS_WGRAD_BLOCK)
        return max(1, min(2 * cus // wgs, units // 4, lib.SUM_SLABS_MAX))

    def _layer_grad(self, i: int, ws, g, xin: torch.Tensor, n: int, T: int, below: bool, reg: Optional[_Reg] = None, n0: int = 0) -> None:
        """layer ``i`` again from its saved input ``xin``, then its backward with the weight, bias and LayerNorm gradients added
        into the parameters' ``.grad``: ``ga`` holds the gradient of the layer's output on entry and, with ``below``, of ``xin``
        on return.  ``reg`` / ``n0``: the forward's regularisers and the chunk's first clip; every mask is drawn again"""
        probs = reg.probs(i, n0) if reg is not None else None

        def attn_bwd(qkv: torch.Tensor, att: torch.Tensor, datt: torch.Tensor, dqkv: torch.Tensor) -> None:
            problem = [self._attn_problem(ws, qkv, att, n, T, T, datt, g["delta"], dqkv)]
            if probs is None:
                lib.attn_bwd_grouped_exact_delta(problem, self.head_dim, self.head_dim ** -0.5)
            else:
                lib.attn_bwd_grouped_exact_delta_keyed(problem, self.head_dim, self.head_dim ** -0.5, probs)
        attend, join, join_bwd, act = self._hooks(i, ws, n, T, n0, reg)
        self._post_ln_layer_grad(i, ws, g, xin, n, T, attend, attn_bwd, lambda dqkv, x: self._qkv_wgrad_roles(i, g["junk"], dqkv, x),
                                 below, self._slabs_for, join, join_bwd, act)

    def _ln_family_layer_grad(self, i: int, ws, g, xin: torch.Tensor, n: int, T: int) -> None:
        """the layer-norm family's ``_layer_grad``: ``_pre_ln_layer_grad`` (mmfusion/backbone.py) with this class's attention backward
        (the exact-delta route) and Q/K/V weight gradient (no column sum for the key bias).  ``ga`` holds the gradient of ``xin`` on
        return whatever lies below: a pre-LN layer's first LayerNorm is its own parameter and its backward takes that gradient in"""
        def attn_bwd(qkv: torch.Tensor, att: torch.Tensor, datt: torch.Tensor, dqkv: torch.Tensor) -> None:
            lib.attn_bwd_grouped_exact_delta([self._attn_problem(ws, qkv, att, n, T, T, datt, g["delta"], dqkv)], self.head_dim,
                                             self.head_dim ** -0.5)
        self._pre_ln_layer_grad(i, ws, g, xin, n, T, attn_bwd, lambda dqkv, ln1: self._qkv_wgrad_roles(i, g["junk"], dqkv, ln1),
                                self._slabs_for)

    def _front_grad(self, ws, g, feat: torch.Tensor, pos_w: torch.Tensor, pos_wt: torch.Tensor, n: int, T: int,
                    reg: Optional[_Reg] = None, n0: int = 0) -> None:
        """the front end again from the saved ``feat``, then its backward: ``ga`` holds the gradient of layer 0's input on entry.
        The gradients of the encoder LayerNorm, the positional bias, the projection and the feature LayerNorm are added into
        their ``.grad``; the positional weight's into ``g["dpos"]`` (f32, packed), which ``_backward`` finishes.  With ``reg``
        the front end is computed under the forward's masks again (``x0`` is the masked, dropped projection), the gradient first
        passes the encoder dropout, the rows of dx0 inside a span are summed into ``masked_spec_embed``'s gradient where it trains
        (per-slab partials, ``mmf_sum_slabs_f32``: a fixed order), and the projection's gradients take dproj = in_span ? 0 : dx0 keep c.
        The layer-norm family has no encoder LayerNorm here (it sits on top of the layers: ``_backward``); ``ga`` / ``gb`` swap roles"""
        c = self.config
        rows, d, cd, R = n * T, c.hidden_size, c.conv_dim[-1], self._rows
        G, k = c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings
        x0, y, fln = R(ws, "x", rows, d), R(ws, "y", rows, d), R(ws, "win", rows, cd)
        ga, gb, dz, dfln, dfeat = R(g, "ga", rows, d), R(g, "gb", rows, d), R(g, "dqkv", rows, d), R(g, "dfln", rows, cd), R(g, "dfeat", rows, cd)
        st1, st2 = self._stats(g, 1), self._stats(g, 2)
        self._front_end(ws, feat, pos_w, n, T, st1, reg, n0)
        if self._ln_family:                    # layer 0 reads the convolution's output itself: the gradient on entry is dy already
            x0, ga, gb = y, gb, ga
        else:
            self._ln(st2, y, R(ws, "ln", rows, d), "enc_ln_w", "enc_ln_b")           # for its statistics; the output is not read
            if reg is not None and reg.p_h > 0.0:
                lib.hidden_dropout(ga, ga, n, reg.hidden(reg.enc, n0))                 # through the dropout behind the encoder LayerNorm
            self._ln_bwd(st2, y, ga, gb, "enc_ln_w", (self.enc_ln_w.grad, self.enc_ln_b.grad))      # gb = dy
        lib.w2v_posconv_bwd_act(x0, pos_w, self._f("pos_b"), gb, dz, n, T, d, G, k)
        lib.colsum_grouped([lib.ColsumProblem(dz.data_ptr(), self.pos_b.grad.data_ptr(), rows, d, d)])
        S = self._pos_wgrad_slabs(n, T)
        if S > 1:
            partial = self._slab_buffer(S * g["dpos"].numel(), dz.device).view(S, -1)
            lib.w2v_posconv_wgrad(dz, x0, partial, n, T, d, G, k, slabs=S)
            lib.sum_slabs(partial, g["dpos"], True)
        else:
            lib.w2v_posconv_wgrad(dz, x0, g["dpos"], n, T, d, G, k, accumulate=True)
        lib.w2v_posconv_dgrad(dz, pos_wt, gb, ga, n, T, d, G, k)                     # ga = dx0: the convolution + the residual
        if reg is not None and reg.front:
            spans = reg.spans(n0, n)
            if spans is not None and self.masked_spec_embed.requires_grad:
                S = max(1, min(lib.SUM_SLABS_MAX, rows // 64))
                partial = self._slab_buffer(S * d, ga.device).view(S, d)
                lib.w2v_mask_embed_grad(ga, spans, partial, n, T, reg.length)
                lib.sum_slabs(partial, self.masked_spec_embed.grad, True)            # (a vector: zeroed with the biases, never lazily)
            lib.w2v_mask_drop(ga, ga, n, T, reg.length, reg.feat_proj(n0), spans)       # ga = dproj
        wg = self.fp_w.grad
        self._wgrad_launch([(ga, fln, wg, self.fp_b.grad)], self._first_touch(wg), self._slabs_for(rows, self._tiles(d, cd)))
        ops.gemm(GEMM_NN, ga, self._w("fp_w"), dfln)
        self._ln_bwd(st1, feat, dfln, dfeat, "fp_ln_w", (self.fp_ln_w.grad, self.fp_ln_b.grad))    # dfeat: what _conv_grad starts from where the conv stack trains

    def _conv_grad(self, ws, g, wave: torch.Tensor, n: int, Ts: List[int]) -> None:
        """the feature extractor's backward on a chunk of ``n`` clips: ``dfeat`` holds the gradient of the last layer's GELU output
        on entry.  The conv stack is computed again with every raw output kept (``_features`` with ``raws``), then walked top down:
        dr_i = the gradient of layer i's raw output, win_i rebuilt from the raw output below, dW_i (+)= dr_i^T win_i straight into
        the parameter's ``.grad`` (stored (C_out, k, C_in): the GEMM's (C_out, k C_in)), dwin_i = dr_i W_i, folded back to dr_{i-1}
        in the place of the raw output it is formed from; layer 0 takes dwin_1 itself (two passes, csrc/wav2vec2.hip)"""
        c = self.config
        dims, ks, ss, last = c.conv_dim, c.conv_kernel, c.conv_stride, len(c.conv_dim) - 1
        raws, at = [None], 0
        for i in range(1, last + 1):
            raws.append(g["raws"][at:at + n * Ts[i] * dims[i]].view(n * Ts[i], dims[i]))
            at += n * Ts[i] * dims[i]
        self._features(ws, wave, n, Ts, raws)
        w0, gn_w, gn_b = self._f("conv0_w"), self._f("conv0_gn_w"), self._f("conv0_gn_b")
        dr = self._rows(g, "dfeat", n * Ts[last], dims[last])
        lib.bias_gelu_bwd(dr, raws[last], None, dr)                                 # dr_last, in place
        for i in range(last, 0, -1):
            rows, K = n * Ts[i], ks[i] * dims[i - 1]
            win, dwin = self._rows(ws, "win", rows, K), self._rows(g, "dwin", rows, K)
            if i == 1:
                lib.w2v_conv0_norm_gelu(wave, w0, ws["stats"], gn_w, gn_b, ws["win"], ks[0], ss[0], ks[1], ss[1], 1e-5)
            elif i < last:                                                          # (the recompute left win_last in place)
                lib.w2v_gelu_window(raws[i - 1], ws["win"], n, Ts[i - 1], dims[i - 1], ks[i], ss[i])
            wg = getattr(self, f"conv{i}_w").grad.view(dims[i], K)
            self._wgrad_launch([(dr, win, wg, g["junk"][:dims[i]])], self._first_touch(wg),
                               self._slabs_for(rows, self._tiles(dims[i], K)))
            ops.gemm(GEMM_NN, dr, self._w(f"conv{i}_w").view(dims[i], K), dwin)
            if i > 1:
                dr = raws[i - 1]
                lib.w2v_window_fold_gelu_bwd(g["dwin"], dr, dr, n, Ts[i - 1], dims[i - 1], ks[i], ss[i])
        w0g = self.conv0_w.grad
        lib.w2v_conv0_bwd_stats(wave, w0, ws["stats"], gn_w, gn_b, g["dwin"], g["bsums"], ws["partial"], self.conv0_gn_w.grad,
                                self.conv0_gn_b.grad, ks[0], ss[0], ks[1], ss[1], 1e-5)     # (vectors: zeroed with the biases, never lazily)
        partial = self._slab_buffer(n * lib.W2V_STATS_SLOTS * dims[0] * ks[0], wave.device)
        lib.w2v_conv0_bwd_wgrad(wave, w0, ws["stats"], gn_w, gn_b, g["dwin"], g["bsums"], partial, w0g, ks[0], ss[0], ks[1], ss[1], 1e-5,
                                accumulate=not self._first_touch(w0g))

    def _backward(self, wave: torch.Tensor, keep: torch.Tensor, feat: Optional[torch.Tensor], first: int, pos_w: torch.Tensor,
                  dout: torch.Tensor, reg: Optional[_Reg] = None, feature_encoder: bool = False,
                  final: Optional[torch.Tensor] = None) -> None:
        """for the gradient ``dout`` (N, T, d) f32 of the result: the gradients of layers ``first`` .. L - 1 and, with ``feat`` (the
        saved input of the feature LayerNorm: the front end trains), of the front end, added into their ``.grad``.  ``keep``: the
        saved inputs of the layers from ``first`` up, ``pos_w``: the positional weight the forward used, ``reg``: its regularisers
        (a layer LayerDrop skipped is the identity: ``ga`` passes through and its parameters receive nothing); ``feature_encoder``:
        the conv stack trains too (``_conv_grad`` takes each chunk's ``dfeat`` from ``_front_grad``); ``final``, the layer-norm
        family: the saved input of ``encoder.layer_norm``, whose backward comes first there"""
        c, d, dev = self.config, self.config.hidden_size, wave.device
        self._refuse_fp32()
        N, Lw = wave.shape
        T, L, front = self.frames(Lw), c.num_hidden_layers, feat is not None
        ws, g = self._workspace(dev, Lw), self._grad_workspace(dev, Lw)
        if front:
            pos_wt = self._pos_weight(transposed=True)
            g["dpos"].zero_()
        for n0, n in self._chunks(N):
            rows = slice(n0 * T, (n0 + n) * T)
            ga = self._rows(g, "ga", n * T, d)
            if final is None:
                self._narrow(dout[n0:n0 + n], ga)
            else:
                gb, st = self._rows(g, "gb", n * T, d), self._stats(g, 1)
                self._narrow(dout[n0:n0 + n], gb)
                self._ln(st, final[rows], self._rows(ws, "ln", n * T, d), "enc_ln_w", "enc_ln_b")     # for its statistics; the output is not read
                self._ln_bwd(st, final[rows], gb, ga, "enc_ln_w", (self.enc_ln_w.grad, self.enc_ln_b.grad))
            for i in reversed(range(first, L)):
                if self._ln_family:
                    self._ln_family_layer_grad(i, ws, g, keep[i - first, rows], n, T)
                elif reg is None or not reg.skip[i]:
                    self._layer_grad(i, ws, g, keep[i - first, rows], n, T, front or i > first, reg, n0)
            if front:
                self._front_grad(ws, g, feat[rows], pos_w, pos_wt, n, T, reg, n0)
            if feature_encoder:
                self._conv_grad(ws, g, wave[n0:n0 + n], n, feat_lengths(Lw, c.conv_kernel, c.conv_stride))
        if front:
            lib.w2v_weightnorm_bwd(g["dpos"], self._f("pos_g"), self._f("pos_v"), self.pos_g.grad, self.pos_v.grad,
                                   self._first_touch(self.pos_v.grad))
