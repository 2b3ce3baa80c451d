"""WavLM backbone on the HIP kernels: waveforms -> frame states, frozen.

``NativeWavLM`` is HuggingFace's ``WavLMModel`` (wavlm-base, wavlm-base-plus; no attention mask) rebuilt from its sizes alone, with
HuggingFace's ``state_dict`` surface.  It is ``NativeWav2Vec2``'s base family with one difference: every layer's attention adds a
gated relative position bias to its scores,

    score[b, h, i, j] = (q_i . k_j) / sqrt(dh) + g[b, h, i] * bias[h, bucket(j - i)]

``bias`` is layer 0's ``rel_attn_embed`` (num_buckets x H), shared by all layers, through log-spaced buckets of the signed
distance; ``g`` comes from the layer's INPUT row (not from q): the 8-output ``gru_rel_pos_linear`` all heads share, on the head's
slice, then ``g = sigmoid(a) (sigmoid(b) gru_rel_pos_const[h] - 1) + 2`` with a / b the sums of outputs 0..3 / 4..7.  The feature
extractor, the feature projection, the positional convolution, the workspace, the chunking and the post-LN layer block are
inherited (mmfusion/wav2vec2.py, mmfusion/backbone.py); per layer the launch list has two launches of this model's own in the
place of the plain attention (``_post_ln_layer``'s ``attend``):

      gate                          mmf_wavlm_gate                       x (the layer input) -> gate (n, H, T) f32
      attention                     mmf_attn_fwd_relbias                 qkv, gate, table -> att (lse is written too)

The bias depends on j - i only, so no (T, T) tensor exists anywhere: per (T, weight version) ``_table`` makes one f32 row of
2T - 1 entries per head, ``table[h][j - i + T - 1]``, and the kernel reads its runs of it (csrc/wavlm.hip).  The bucket of every
distance is computed on the host with HuggingFace's own float32 expression (log, divide, multiply, truncate, clamp), so distances
on a bucket boundary land where HuggingFace puts them (a device ``log`` may differ in the last bit), and kept per T; the gather from
``rel_attn_embed`` runs on the device.  The first call at a new T therefore copies an index to the device: capture a graph after a
call at that T.

Frozen forward only.  Refused, each with an error that names ``NativeWavLM``: ``set_trainable_layers(k > 0)`` and every regulariser
above 0 (no backward of the biased attention is built), ``attention_mask``, the fp32 parity mode, CPU tensors, and the wavlm-large
combination (``feat_extract_norm="layer"``, ``do_stable_layer_norm=True``, ``conv_bias``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from . import arena as _arena
from . import lib
from .backbone import BackboneOutput, WsTable
from .wav2vec2 import DEFAULT_CHUNK, REG_NAMES, NativeWav2Vec2

_BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
# constructor kwargs of the released families (wavlm-base and wavlm-base-plus differ in their training data only)
FAMILIES = {"base": dict(_BASE), "base-plus": dict(_BASE)}


def relative_buckets(distances: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """HuggingFace's ``WavLMAttention._relative_positions_bucket`` on int64 ``distances`` (memory - context), operation for
    operation in float32 on the host"""
    nb = num_buckets // 2
    rel = distances.to(torch.long).cpu()
    out = (rel > 0).to(torch.long) * nb
    rel = torch.abs(rel)
    max_exact = nb // 2
    small = rel < max_exact
    large = torch.log(rel.float() / max_exact)
    large = large / math.log(max_distance / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(small, rel, large)


class NativeWavLM(NativeWav2Vec2):
    """HuggingFace ``WavLMModel`` (no attention mask), defaults = wavlm-base / wavlm-base-plus (``FAMILIES``).

    ``forward(input_values)`` -> ``.last_hidden_state`` (N, T, hidden) f32; ``input_values``: (N, L) f32 on the GPU.  Frozen.
    ``state_dict()`` has the keys, shapes and order of ``WavLMModel``; ``load_state_dict`` also takes the older weight-norm names."""

    def __init__(self, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, conv_dim: Sequence[int] = (512,) * 7,
                 conv_kernel: Sequence[int] = (10, 3, 3, 3, 3, 2, 2), conv_stride: Sequence[int] = (5, 2, 2, 2, 2, 2, 2),
                 conv_bias: bool = False, num_conv_pos_embeddings: int = 128, num_conv_pos_embedding_groups: int = 16,
                 layer_norm_eps: float = 1e-5, feat_extract_norm: str = "group", do_stable_layer_norm: bool = False,
                 num_buckets: int = 320, max_bucket_distance: int = 800, chunk: int = DEFAULT_CHUNK, **regularisers):
        who = "NativeWavLM"
        if feat_extract_norm != "group" or do_stable_layer_norm or conv_bias:
            raise ValueError(f"{who}: feat_extract_norm={feat_extract_norm!r}, do_stable_layer_norm={do_stable_layer_norm!r}, "
                             f"conv_bias={conv_bias!r}: only the wavlm-base family ('group', False, False) is built; wavlm-large's "
                             "layer-norm feature extractor with pre-LN layers is not")
        nb, md = int(num_buckets), int(max_bucket_distance)
        if nb < 4 or nb % 4 or md <= nb // 4:
            raise ValueError(f"{who}: num_buckets={num_buckets!r} must be a multiple of 4 (half per sign, half of those exact) and "
                             f"max_bucket_distance={max_bucket_distance!r} above num_buckets / 4")
        unknown = sorted(set(regularisers) - set(REG_NAMES) - {"mask_feature_prob"})
        if unknown:
            raise TypeError(f"{who}: unexpected arguments {unknown}")
        super().__init__(hidden_size, num_hidden_layers, num_attention_heads, intermediate_size, conv_dim, conv_kernel, conv_stride,
                         False, num_conv_pos_embeddings, num_conv_pos_embedding_groups, layer_norm_eps, "group", False,
                         chunk=chunk, **regularisers)
        c, H, dh = self.config, self.config.num_attention_heads, self.head_dim
        c.model_type, c.num_buckets, c.max_bucket_distance = "wavlm", nb, md
        for i in range(c.num_hidden_layers):
            a = f"encoder.layers.{i}.attention."
            self._add(f"l{i}_gate_c", (1, H, 1, 1), a + "gru_rel_pos_const", ones=True)
            self._add(f"l{i}_gate_w", (8, dh), a + "gru_rel_pos_linear.weight", std=dh ** -0.5)
            self._add(f"l{i}_gate_b", (8,), a + "gru_rel_pos_linear.bias", std=0.0)
        self._add("rel_embed", (nb, H), "encoder.layers.0.attention.rel_attn_embed.weight", std=1.0)
        self._hf = {k: self._hf[k] for k in self._hf_order()}
        self._bucket_index: Dict[int, torch.Tensor] = {}       # T -> the bucket of every distance -(T - 1) .. T - 1, on the device

    def _hf_order(self) -> list:
        """``WavLMModel.state_dict()``'s key order: Wav2Vec2's, with an attention's own parameter (``gru_rel_pos_const``) ahead of
        its projections and ``gru_rel_pos_linear`` / ``rel_attn_embed`` behind ``out_proj``"""
        keys = []
        for k in self._hf:
            if ".attention.gru_rel_pos" in k or ".attention.rel_attn_embed" in k:
                continue
            a = k[:k.index("attention.") + len("attention.")] if ".attention.k_proj.weight" in k else None
            if a is not None:
                keys.append(a + "gru_rel_pos_const")
            keys.append(k)
            if k.endswith(".attention.out_proj.bias"):
                a = k[:-len("out_proj.bias")]
                keys += [a + "gru_rel_pos_linear.weight", a + "gru_rel_pos_linear.bias"]
                if a + "rel_attn_embed.weight" in self._hf:
                    keys.append(a + "rel_attn_embed.weight")
        assert sorted(keys) == sorted(self._hf), "every key once"
        return keys

    # -- frozen only ------------------------------------------------------------------------------------------
    def set_trainable_layers(self, k: int, front: bool = False, feature_encoder: bool = False) -> None:
        """0 only: ``NativeWavLM`` is a frozen backbone (the backward of the biased attention is not built)"""
        if isinstance(k, bool) or k != 0 or front or feature_encoder:
            raise ValueError(f"NativeWavLM: set_trainable_layers({k!r}, front={front!r}, feature_encoder={feature_encoder!r}): the "
                             "backbone is frozen; no backward of the gated relative-bias attention is built yet")
        super().set_trainable_layers(0)

    def set_regularisation(self, **settings) -> None:
        """every setting must stay 0: the regularisers act in a differentiable training call, which this frozen model has none of"""
        on = sorted(n for n in REG_NAMES[:6] if n in settings and not isinstance(settings[n], bool) and settings[n] != 0)
        if on:
            raise ValueError(f"NativeWavLM: set_regularisation({', '.join(f'{n}={settings[n]!r}' for n in on)}): the training-mode "
                             "regularisers are not built for this frozen backbone; they stay at 0")
        super().set_regularisation(**settings)

    # -- workspace / derived ------------------------------------------------------------------------------------
    def _ws_table(self, L: int) -> WsTable:
        return super()._ws_table(L) + [("gate", self.config.num_attention_heads * self.frames(L), torch.float32)]

    def _table(self, T: int, dev) -> torch.Tensor:
        """(H, 2T - 1) f32, ``table[h][j - i + T - 1] = rel_attn_embed[bucket(j - i)][h]``: once per (T, weight version)"""
        c = self.config
        idx = self._bucket_index.get(T)
        if idx is None or idx.device != dev:
            idx = relative_buckets(torch.arange(-(T - 1), T), c.num_buckets, c.max_bucket_distance).to(dev)
            self._bucket_index[T] = idx
        return self._derived(f"rel_table_{T}", ("rel_embed",), lambda: self._f("rel_embed").index_select(0, idx).t().contiguous())

    # -- launches -----------------------------------------------------------------------------------------------
    def _hooks(self, i: int, ws, n: int, T: int, n0: int, reg) -> tuple:
        """layer ``i``'s attention: the gate from the layer input (``x``, still whole when ``attend`` runs), then the fused forward
        with the bias.  No join / activation hooks: nothing trains"""
        c, dh = self.config, self.head_dim
        H, rows = c.num_attention_heads, n * T
        x, gate = self._rows(ws, "x", rows, c.hidden_size), ws["gate"][:n * H * T]
        table = self._table(T, x.device)

        def attend(qkv: torch.Tensor, att: torch.Tensor) -> None:
            lib.wavlm_gate(x, self._f(f"l{i}_gate_w"), self._f(f"l{i}_gate_b"), self._f(f"l{i}_gate_c").view(H), gate, n, T, H, dh)
            lib.attn_fwd_relbias(self._attn_problem(ws, qkv, att, n, T, T), dh, dh ** -0.5, gate, table)
        return attend, None, None, None

    def forward(self, input_values: torch.Tensor, attention_mask=None) -> BackboneOutput:
        who = "NativeWavLM"
        if attention_mask is not None:
            raise NotImplementedError(f"{who}: attention_mask is not implemented (the reference never passes one)")
        self._check_input(input_values, "input_values")
        if input_values.dim() != 2:
            raise ValueError(f"{who}: input_values {tuple(input_values.shape)} is not (N, L)")
        if self.frames(input_values.shape[1]) < 1:
            raise ValueError(f"{who}: {input_values.shape[1]} samples are shorter than the feature extractor's receptive field")
        _arena.ensure(self)
        with torch.no_grad():
            return BackboneOutput(self._launches(input_values.contiguous(), self._pos_weight()))
