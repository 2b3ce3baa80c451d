"""Frozen DeBERTa-v3 backbone on the HIP kernels: token ids (or input embeddings) + attention mask -> token states, forward only.

The reference pushes every batch of token ids through HuggingFace's ``AutoModel`` for ``microsoft/deberta-v3-base`` (reference
models/encoders.py:20,49-71).  ``NativeDeberta`` is ``DebertaV2Model`` rebuilt from its sizes alone (nothing is fetched), with
HuggingFace's ``state_dict`` surface, so published checkpoints and the reference's ``.pth`` files load.  Only the v3 family
is built: relative attention with shared keys, ``pos_att_type = "p2c|c2p"``, layer-normed relative embeddings, no absolute
position or token-type embeddings, no convolution, exact GELU, post-LN layers.

What a DeBERTa layer has and the other backbones' layers do not is the disentangled attention: the scores carry a
content-to-position and a position-to-content term gathered through log-bucketed relative distances,

    s[i, j] = (Q_i . K_j + Q_i . posK[idx(i - j)] + K_j . posQ[idx(i - j)]) / sqrt(3 head_dim)
    idx(delta) = clamp(bucket(delta) + S, 0, 2 S - 1),  S = position_buckets

and a padding mask.  ``mmf_deberta_attn_fwd`` (csrc/deberta.hip) fuses all of it; ``idx`` is a (2 T - 1) int32 table built on
the host by HuggingFace's own float32 operations (``bucket_index``) and cached per (T, S, max position).  ``bucket`` is odd in
delta, so both gathers use the one table (tests/test_deberta_cpu.py holds that to HuggingFace's tables).

Launch list for a chunk of ``n`` items of ``T`` tokens (the layer's blocks: mmfusion/backbone.py):

    gather + LayerNorm + mask       mmf_deberta_embed                    ids | inputs_embeds -> x (n T, hidden)
    per post-LN layer:
      fused Q/K/V linear + bias     mmf_gemm_grouped NT, BIAS            x   -> qkv
      disentangled attention        mmf_deberta_attn_fwd                 qkv, posQ_i, posK_i, idx, mask -> att
      out-projection + bias + x     mmf_gemm_grouped NT, BIAS | ADD_AUX  att -> y
      LayerNorm                                                          y   -> ln
      _ffn(ln, + ln)                                                     ln  -> h -> y
      LayerNorm                                                          y   -> x
    widening cast                   mmf_cast_bf16_to_f32                 x   -> result

``LayerNorm(rel_embeddings)`` and every layer's ``posQ | posK`` (that layer's own q / k projection of it, biases included)
depend on the frozen weights only: they are computed once per weight version (one mmf_deberta_embed launch on the relative
table, one GEMM per layer) and kept as bf16; ``load_state_dict`` moves the parameters' version counters, which rebuilds them.

Items are processed in chunks of ``chunk`` through one workspace sized by the chunk and the longest sequence seen so far.
Forward only, frozen, bf16 storage only, nothing synchronises with the host (mmfusion/backbone.py).
"""
from __future__ import annotations

import math
import types
from typing import Dict, Optional, Tuple

import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BF16, BackboneOutput, FrozenBackbone, WsTable
from .lib import EPI_BIAS, GEMM_NT

# items per pass through the workspace.  NOT chosen by measurement yet: 16 items of 512 tokens give the layer GEMMs 8192 rows
# at 0.14 GB of workspace; tools/deberta_bench.py --chunks is the sweep that should decide it
DEFAULT_CHUNK = 16
MAX_TOKENS = 1024                          # mmf_deberta_attn_fwd's longest sequence
# keys a published checkpoint carries and HuggingFace's DebertaV2Model ignores on load
_IGNORED = ("embeddings.position_ids", "embeddings.position_embeddings.", "mask_predictions.", "lm_predictions.")


def log_bucket(delta: torch.Tensor, bucket_size: int, max_position: int) -> torch.Tensor:
    """HuggingFace's ``make_log_bucket_position`` on an int64 tensor: the same float32 operations (true division, ``log``,
    ``ceil``, ``where``) in the same order, so the buckets agree with HuggingFace's entry for entry"""
    sign = torch.sign(delta)
    mid = bucket_size // 2
    abs_pos = torch.where((delta < mid) & (delta > -mid), torch.tensor(mid - 1).type_as(delta), torch.abs(delta))
    log_pos = torch.ceil(torch.log(abs_pos / mid) / torch.log(torch.tensor((max_position - 1) / mid)) * (mid - 1)) + mid
    return torch.where(abs_pos <= mid, delta.type_as(log_pos), log_pos * sign).to(torch.long)


def bucket_index(T: int, S: int, max_position: int) -> torch.Tensor:
    """int32 (2T - 1,) on the CPU: entry ``delta + T - 1`` = clamp(bucket(delta) + S, 0, 2S - 1), delta = i - j"""
    delta = torch.arange(-(T - 1), T, dtype=torch.long)
    return torch.clamp(log_bucket(delta, S, max_position) + S, 0, 2 * S - 1).to(torch.int32)


class _WordEmbeddings:
    """``model.embeddings.word_embeddings``: ids -> f32 embeddings without autograd (``TextEncoder``'s prompt route calls it
    and hands the result back as ``inputs_embeds``).  Not an ``nn.Module``: the table is the backbone's own parameter."""

    def __init__(self, owner: "NativeDeberta"):
        self._owner = [owner]                          # (a list: the backbone must not become a submodule of its own attribute)

    @property
    def weight(self) -> torch.Tensor:
        return self._owner[0].word_emb.detach()

    def __call__(self, input_ids: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            return torch.nn.functional.embedding(input_ids, self.weight)


class NativeDeberta(FrozenBackbone):
    """HuggingFace ``DebertaV2Model`` (inference), the v3 family, defaults = deberta-v3-base.

    ``forward(input_ids=None, attention_mask=None, inputs_embeds=None)`` -> ``.last_hidden_state`` (N, T, hidden) f32.
    ``input_ids`` (N, T) int64 or ``inputs_embeds`` (N, T, hidden) f32, on the GPU, exactly one of them; ``attention_mask``
    (N, T) of any integer / bool / float dtype, or None for all ones.  Masked keys get probability exactly 0; a masked query
    row attends uniformly over all T keys, so padded rows of the result are HuggingFace's too.
    ``state_dict()`` has the keys, shapes and order of ``DebertaV2Model``; Q/K/V are stored fused and split on the way."""

    def __init__(self, vocab_size: int = 128100, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, max_position_embeddings: int = 512, position_buckets: int = 256,
                 layer_norm_eps: float = 1e-7, relative_attention: bool = True, share_att_key: bool = True,
                 pos_att_type=("p2c", "c2p"), norm_rel_ebd: str = "layer_norm", position_biased_input: bool = False,
                 type_vocab_size: int = 0, conv_kernel_size: int = 0, max_relative_positions: int = -1, hidden_act: str = "gelu",
                 embedding_size: Optional[int] = None, chunk: int = DEFAULT_CHUNK):
        d, H, I, S = int(hidden_size), int(num_attention_heads), int(intermediate_size), int(position_buckets)
        who = "NativeDeberta"
        pos = sorted(p.strip() for p in (pos_att_type.split("|") if isinstance(pos_att_type, str) else (pos_att_type or ())))
        if not relative_attention:
            raise ValueError(f"{who}: relative_attention=False is not built (the v3 family attends through relative positions)")
        if not share_att_key:
            raise ValueError(f"{who}: share_att_key=False (separate pos_key_proj / pos_query_proj) is not built")
        if pos != ["c2p", "p2c"]:
            raise ValueError(f"{who}: pos_att_type={pos_att_type!r}: only 'p2c|c2p' is built")
        if [p.strip() for p in str(norm_rel_ebd).lower().split("|")] != ["layer_norm"]:
            raise ValueError(f"{who}: norm_rel_ebd={norm_rel_ebd!r}: only 'layer_norm' is built")
        if position_biased_input:
            raise ValueError(f"{who}: position_biased_input=True (absolute position embeddings) is not built")
        if type_vocab_size:
            raise ValueError(f"{who}: type_vocab_size={type_vocab_size}: token-type embeddings are not built")
        if conv_kernel_size:
            raise ValueError(f"{who}: conv_kernel_size={conv_kernel_size}: the convolution layer (v2 xlarge) is not built")
        if max_relative_positions >= 1 and max_relative_positions != max_position_embeddings:
            raise ValueError(f"{who}: max_relative_positions={max_relative_positions}: only -1 (max_position_embeddings) is built")
        if hidden_act != "gelu":
            raise ValueError(f"{who}: hidden_act={hidden_act!r}: only the exact 'gelu' is built")
        if embedding_size is not None and int(embedding_size) != d:
            raise ValueError(f"{who}: embedding_size={embedding_size} differs from hidden_size {d}: embed_proj is not built")
        super().__init__(d, H, chunk, head_dims=(64,))         # (the disentangled attention kernel's only form; every published v3 size has it)
        if not 1 <= S <= 256:
            raise ValueError(f"{who}: position_buckets {S} must be in 1 .. 256 (the attention kernel takes up to 512 relative rows)")
        if max_position_embeddings < 2 or vocab_size < 1 or I % 8 or I < 8:
            raise ValueError(f"{who}: max_position_embeddings {max_position_embeddings} (at least 2), vocab_size {vocab_size} (at least 1), "
                             f"intermediate_size {I} (a multiple of 8)")
        if num_hidden_layers < 1 or chunk < 1:
            raise ValueError(f"{who}: layers and chunk at least 1")
        self.config = types.SimpleNamespace(
            vocab_size=int(vocab_size), hidden_size=d, num_hidden_layers=int(num_hidden_layers), num_attention_heads=H,
            intermediate_size=I, max_position_embeddings=int(max_position_embeddings), position_buckets=S,
            layer_norm_eps=float(layer_norm_eps), relative_attention=True, share_att_key=True, pos_att_type=["p2c", "c2p"],
            norm_rel_ebd="layer_norm", position_biased_input=False, type_vocab_size=0, max_relative_positions=-1,
            hidden_act="gelu", model_type="deberta-v2")
        add = self._add
        add("word_emb", (vocab_size, d), "embeddings.word_embeddings.weight")
        add("emb_ln_w", (d,), "embeddings.LayerNorm.weight", ones=True)
        add("emb_ln_b", (d,), "embeddings.LayerNorm.bias", std=0.0)
        for i in range(num_hidden_layers):
            a, att = f"encoder.layer.{i}.", f"encoder.layer.{i}.attention."
            self._add_layer(i, d, I, {"q": att + "self.query_proj", "k": att + "self.key_proj", "v": att + "self.value_proj",
                                      "o": att + "output.dense", "ln1": att + "output.LayerNorm", "fc1": a + "intermediate.dense",
                                      "fc2": a + "output.dense", "ln2": a + "output.LayerNorm"})
        add("rel_emb", (2 * S, d), "encoder.rel_embeddings.weight")
        add("enc_ln_w", (d,), "encoder.LayerNorm.weight", ones=True)
        add("enc_ln_b", (d,), "encoder.LayerNorm.bias", std=0.0)
        self.embeddings = types.SimpleNamespace(word_embeddings=_WordEmbeddings(self))
        self._idx: Dict[Tuple, torch.Tensor] = {}      # (T, S, max position, device) -> the int32 table on that device

    # -- HuggingFace state_dict surface ----------------------------------------------------------------
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        kept = {k: v for k, v in state_dict.items() if not (k.startswith(prefix) and k[len(prefix):].startswith(_IGNORED))}
        super()._load_from_state_dict(kept, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    # -- shapes / workspace -----------------------------------------------------------------------------
    def _ws_table(self, T: int) -> WsTable:
        """per item of ``T`` tokens"""
        return self._token_table(T, T * self.config.intermediate_size)

    def workspace_bytes_per_item(self, T: int) -> int:
        return self._bytes_per_item(self._ws_table(T))

    def _index(self, T: int, dev) -> torch.Tensor:
        c = self.config
        key = (T, c.position_buckets, c.max_position_embeddings, dev)
        t = self._idx.get(key)
        if t is None:
            host = bucket_index(T, c.position_buckets, c.max_position_embeddings)
            step = host[1:] - host[:-1]
            if T > 1 and (int(step.min()) < 0 or int(step.max()) > 1):
                raise ValueError(f"NativeDeberta: position_buckets {c.position_buckets} with max_position_embeddings "
                                 f"{c.max_position_embeddings} makes buckets that skip rows between neighbouring distances: the attention "
                                 "kernel has no form for that")
            t = self._idx[key] = host.to(dev)
        return t

    # -- weights ----------------------------------------------------------------------------------------
    def _pos_tables(self, dev) -> list:
        """per layer (posQ, posK) = the layer's q / k projection (bias included) of LayerNorm(rel_embeddings): bf16 (2S, d) views
        of one (2S, 2d) GEMM output, computed on the HIP kernels once per weight version"""
        c = self.config
        d, rows = c.hidden_size, 2 * c.position_buckets

        def build():
            rel = torch.empty((rows, d), dtype=BF16, device=dev)
            lib.deberta_embed(rel, None, self._f("enc_ln_w"), self._f("enc_ln_b"), c.layer_norm_eps, embeds=self._f("rel_emb"))
            pos = []
            for i in range(c.num_hidden_layers):
                qk = torch.empty((rows, 2 * d), dtype=BF16, device=dev)
                ops.gemm(GEMM_NT, rel, self._w(f"l{i}_qkv_w")[:2 * d], qk, bias=self._f(f"l{i}_qkv_b")[:2 * d], epilogue=EPI_BIAS)
                pos.append((qk[:, :d], qk[:, d:]))
            return pos
        names = ["rel_emb", "enc_ln_w", "enc_ln_b"] + [f"l{i}_qkv_{s}" for i in range(c.num_hidden_layers) for s in "wb"]
        return self._derived("pos", names, build)

    # -- launches ---------------------------------------------------------------------------------------
    def _layer(self, i: int, ws, n: int, T: int, pos, idx: torch.Tensor, mask: Optional[torch.Tensor]) -> None:
        """a post-LN layer around the disentangled attention: ``pos`` = this layer's (posQ, posK), ``idx`` the index table,
        ``mask`` the chunk's (n, T) mask or None"""
        c, scale = self.config, math.sqrt(3.0 * self.head_dim)

        def attend(qkv: torch.Tensor, att: torch.Tensor) -> None:
            lib.deberta_attn_fwd(qkv, pos[0], pos[1], idx, mask, att, n, c.num_attention_heads, T, c.position_buckets, scale, self.head_dim)
        self._post_ln_layer(i, ws, n, T, attend)

    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None) -> BackboneOutput:
        c, who = self.config, "NativeDeberta"
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError(f"{who}: exactly one of input_ids / inputs_embeds")
        d = c.hidden_size
        if input_ids is not None:
            self._check_input(input_ids, "input_ids", torch.int64, ndim=2)
            src = input_ids.contiguous()
        else:
            self._check_input(inputs_embeds, "inputs_embeds")
            if inputs_embeds.dim() != 3 or inputs_embeds.shape[2] != d:
                raise ValueError(f"{who}: inputs_embeds {tuple(inputs_embeds.shape)} is not (N, T, {d})")
            src = inputs_embeds.contiguous()
        N, T = src.shape[:2]
        if not 1 <= T <= MAX_TOKENS:
            raise ValueError(f"{who}: {T} tokens: the attention kernel takes 1 .. {MAX_TOKENS}")
        dev = src.device
        mask = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (N, T) or attention_mask.device != dev:
                raise ValueError(f"{who}: attention_mask {tuple(attention_mask.shape)} is not (N, T) = ({N}, {T}) on the inputs' device")
            mask = attention_mask if attention_mask.dtype in (torch.float32, torch.uint8, torch.bool) else attention_mask.to(torch.float32)
            mask = mask.contiguous()
        _arena.ensure(self)
        pos, idx = self._pos_tables(dev), self._index(T, dev)
        ws = self._workspace(dev, T)
        out = torch.empty((N, T, d), dtype=torch.float32, device=dev)
        table, gamma, beta = self._f("word_emb"), self._f("emb_ln_w"), self._f("emb_ln_b")
        for n0 in range(0, N, self.chunk):
            n = min(self.chunk, N - n0)
            x = self._rows(ws, "x", n * T, d)
            part, m = src[n0:n0 + n], None if mask is None else mask[n0:n0 + n]
            if input_ids is not None:
                lib.deberta_embed(x, table, gamma, beta, c.layer_norm_eps, ids=part.reshape(-1), mask=m)
            else:
                lib.deberta_embed(x, None, gamma, beta, c.layer_norm_eps, embeds=part, mask=m)
            for i in range(c.num_hidden_layers):
                self._layer(i, ws, n, T, pos[i], idx, m)
            self._widen(x, out[n0:n0 + n])
        return BackboneOutput(out)
