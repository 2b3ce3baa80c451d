"""DeBERTa-v3 backbone on the HIP kernels: token ids (or input embeddings) + attention mask -> token states, with the gradient
with respect to the input embeddings (prompt tuning) and, for the top layers marked trainable, to their weights (fine-tuning);
frozen by default.

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
Frozen, bf16 storage only, nothing synchronises with the host (mmfusion/backbone.py).

The input gradient.  ``forward(inputs_embeds=...)`` with embeddings that require a gradient, grad mode on, is one
``torch.autograd.Function`` around the whole call; every other call is the launch list above and returns a tensor without a
graph.  Prompt tuning needs no weight gradient, and posQ | posK depend on the frozen weights only, so the backward is the
input-gradient pass through the frozen layers.  The differentiable forward is the launch list above plus one copy per layer:
it keeps the bf16 input ``x`` of every layer (L N T d 2 bytes) and the backward, per chunk and per layer in reverse, runs the
layer's forward again from that ``x`` and then its backward, the post-LN layer's (``_post_ln_layer_grad``, mmfusion/backbone.py
has its rows; the frozen walk: no weight gradient) with

      the attention again           mmf_deberta_attn_fwd_lse             qkv -> att, lse
      attention backward            mmf_deberta_attn_bwd (3 launches)    datt -> dqkv
    embedding backward              mmf_deberta_embed_bwd                gx  -> d inputs_embeds (f32)

Gradients are stored as bf16 exactly where the forward stores the activation they belong to (a residual join is summed in f32
in the GEMM epilogue and rounded once); the incoming gradient of ``last_hidden_state`` is rounded to bf16 once, the outgoing
one is f32.  The recomputation reuses the forward workspace; what the backward holds beside it (the second pre-LN sum, the GELU
output beside ``h``, both LayerNorms' statistics, lse, the gradient buffers and scratch) is a table of its own
(``_grad_table``), allocated on the first differentiable call.

The top-K weight gradients.  ``set_trainable_layers(k)`` marks the parameters of layers ``L - k .. L - 1`` trainable; with grad
mode on every call is then the differentiable one (the trainable parameters are inputs of the ``autograd.Function``, so the ids
route carries a graph too), it keeps the inputs of the layers the backward will walk only (``>= L - k``, all when the
embeddings need a gradient as well), and the backward of a trainable layer adds, in stream order where the operands stand,

      dW_fc2 += dy2^T gel   dW_fc1 += dh^T ln   dW_o += dy1^T att   dW_qkv += dqkv^T x     mmf_gemm_grouped TN, COLSUM_A (the biases)
      both LayerNorms' dgamma / dbeta                                                     mmf_layernorm_bwd_grouped, into .grad
      d(posQ | posK) += ...                                                               mmf_deberta_attn_bwd_pos (4 launches)

into the parameters' f32 ``.grad`` (the arena's lazy-zero protocol as ``ops.queue_wgrad`` keeps it), and stops after the lowest
trainable layer's weight gradients when the embeddings need none.  The layer's q / k weights are used twice, on the tokens and on
LayerNorm(rel_embeddings): the f32 (2S, 2d) gradient of posQ | posK is summed over the chunks, rounded to bf16 once (where the
forward stores the tables) and two TN GEMMs against ``rel`` add ``dW_qkv[:2d] += dpos^T rel`` and ``db_q += colsum(dposQ)``
(``colsum(dposK)`` is zero in exact arithmetic, the rows of dS summing to zero, so ``db_k`` takes none).
A trainable layer's tables are computed in every call (the optimiser writes weights through raw pointers: no version counter
moves).  ``rel_embeddings``, the encoder LayerNorm, the word embeddings and the embedding LayerNorm stay frozen in this mode.

All weights.  ``set_trainable_layers(L, embeddings=True)`` trains those four as well (six tensors): every layer already runs the
position path, and the walk goes down to layer 0 with its input gradient.  Per chunk, after layer 0,

      ids route     mmf_deberta_embed_bwd_params (ids, table)    gx -> the gathered rows' f32 gradient; emb LN dgamma / dbeta += ...
                    mmf_embedding_scatter_add_f32                those rows -> word_emb.grad (masked tokens skipped)
      embeds route  mmf_deberta_embed_bwd_params (embeds)        gx -> d inputs_embeds (mmf_deberta_embed_bwd's bits); dgamma / dbeta

and after the last chunk the position path continues below posQ | posK: d rel = sum over the layers of bf16(dpos_i) W_qk,i, one NN
GEMM per layer adding into one f32 (2S, d) buffer in stream order; rounded to bf16 once (``rel`` is stored as bf16), then
``mmf_deberta_embed_bwd_params`` on the relative table adds into ``rel_emb.grad`` and the encoder LayerNorm's gradients.  Neither
kernel uses atomics: the column sums go through per-workgroup partials added in a fixed order, and the scatter's first occurrence
of a table row owns it.  ``rel`` is then computed in every call too (nothing derived from a trainable tensor is cached).  The table
gradients are plain accumulating regions of the arena (never first-touch managed: a scatter cannot overwrite the rows it does not
visit), so ``zero_grad`` clears them by memset.  On the prompt route ``embeddings.word_embeddings(input_ids)`` carries a graph in
this mode and its backward scatters the gradient of ``inputs_embeds`` into the table.

Dropout.  HuggingFace's model in ``train()`` drops at five sites, and the reference trains it that way; here they are opt-in
(``hidden_dropout_prob`` / ``attention_probs_dropout_prob``, both 0 by default, or ``set_dropout``) and act only in a call that has
``self.training``, a probability above 0 and the differentiable route; every other call is the launch lists above, bit for bit.

    1  embeddings                 mmf_hidden_dropout (in place)        x = dropout(LayerNorm(..) * mask)
    2  relative embeddings        mmf_hidden_dropout, once per layer   rel_i = dropout_i(rel); posQ_i | posK_i from rel_i, every call
    3  attention probabilities    mmf_deberta_attn_fwd_drop            softmax -> dropout -> @ V, inside the kernel
    4  attention output           NT, BIAS; mmf_hidden_dropout         y = bf16(fma(dense + bias, keep c, x))
    5  MLP output                 NT, BIAS; mmf_hidden_dropout         y = bf16(fma(dense + bias, keep c, ln))

Sites 1, 2, 4, 5 take ``hidden_dropout_prob``, site 3 ``attention_probs_dropout_prob``; a probability of 0 leaves its sites' launches
as they are without dropout.  A call takes 1 + 4 L sites from ``ops.next_site()`` in that order (``_Drop``) and keeps them for its
backward; the keying, and why no result depends on ``chunk``, is mmfusion/backbone.py's ("Training-mode dropout"; ``rel_i`` is one
item, sub-stream 0).  The backward draws every mask again: the recomputed layer regenerates sites 3 - 5, the attention
backward is ``mmf_deberta_attn_bwd_drop`` / ``_pos_drop``, ``dW_qkv[:2d] += bf16(dpos_i)^T rel_i`` with ``rel_i`` drawn again, and
d rel = sum_i keep_i c (bf16(dpos_i) W_qk,i): one NN GEMM per layer into its own f32 slab, masked there, then ``mmf_sum_slabs_f32``.
"""
from __future__ import annotations

import math
import types
from typing import Dict, Optional, Tuple

import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BF16, BackboneOutput, FrozenBackbone, WsTable, _CallDropout, _check_probability
from .lib import EPI_ACCUM, EPI_BIAS, EPI_COLSUM_A, GEMM_NN, GEMM_NT, GEMM_TN

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


class _Gather(torch.autograd.Function):
    """``word_emb[ids]`` with the table as an input, so that the result carries a graph; the table's gradient is not returned
    but added into its f32 ``.grad`` by ``mmf_embedding_scatter_add_f32`` (no mask: the reference's embedding has none)"""

    @staticmethod
    def forward(ctx, model: "NativeDeberta", ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
        _arena.ensure(model)
        ctx.model = model
        ctx.save_for_backward(ids)
        return torch.nn.functional.embedding(ids, table.detach())

    @staticmethod
    def backward(ctx, grad: torch.Tensor):
        (ids,) = ctx.saved_tensors
        lib.embedding_scatter_add(ids.reshape(-1).contiguous(), grad.contiguous().view(-1, grad.shape[-1]), ctx.model.word_emb.grad)
        return None, None, None


class _WordEmbeddings:
    """``model.embeddings.word_embeddings``: ids -> f32 embeddings (``TextEncoder``'s prompt route calls it and hands the result
    back as ``inputs_embeds``); without autograd unless the table trains (``set_trainable_layers(L, embeddings=True)``) and grad
    mode is on: then the result carries a graph whose backward adds into ``word_emb.grad``.  Not an ``nn.Module``: the table is
    the backbone's own parameter."""

    def __init__(self, owner: "NativeDeberta"):
        self._owner = [owner]                          # (a list: the backbone must not become a submodule of its own attribute)

    @property
    def weight(self) -> torch.Tensor:
        return self._owner[0].word_emb.detach()

    def __call__(self, input_ids: torch.Tensor) -> torch.Tensor:
        owner = self._owner[0]
        if torch.is_grad_enabled() and owner.word_emb.requires_grad:
            if not input_ids.is_cuda or input_ids.dtype != torch.int64:
                raise TypeError("NativeDeberta: the trainable word embeddings take int64 ids on the GPU (no CPU fallback)")
            return _Gather.apply(owner, input_ids, owner.word_emb)
        with torch.no_grad():
            return torch.nn.functional.embedding(input_ids, self.weight)


class _Drop(_CallDropout):
    """The dropout of one differentiable training call (mmfusion/backbone.py), its 1 + 4 L sites in HuggingFace's order: the
    embeddings, then per layer the relative embeddings, the attention probabilities, the attention output, the MLP output."""
    REL, PROBS, OUT, MLP = range(4)

    def __init__(self, p_h: float, p_a: float, layers: int):
        super().__init__(p_h, p_a, 1, layers)
        (self.emb,) = self.lead

    def probs(self, i: int, item0: int) -> Optional[tuple]:
        """the attention's (p, state, site, item base): the kernel forms the stream id (item0 + item) H + head itself"""
        return self.key(self.p_a, self.layers[i][self.PROBS], item0) if self.p_a > 0.0 else None


class _Differentiable(torch.autograd.Function):
    """``NativeDeberta._run``, differentiable with respect to ``inputs_embeds`` and to the parameters of the trainable layers
    and, with them all, the embedding-side parameters.  ``params`` are those parameters: they are inputs so that the result
    carries a graph on the ids route too; their gradients are not returned but added into their f32 ``.grad`` by the backward's
    own launches, as ``ops.queue_wgrad``'s are."""

    @staticmethod
    def forward(ctx, model: "NativeDeberta", src: torch.Tensor, mask: Optional[torch.Tensor], by_ids: bool, drop: Optional[_Drop],
                *params) -> torch.Tensor:
        N, T = src.shape[:2]
        L = model.config.num_hidden_layers
        need_in = not by_ids and ctx.needs_input_grad[1]
        emb = model.trainable_embeddings
        first = 0 if need_in or emb else L - model.trainable_layers   # the lowest layer the backward walks
        keep = model._keep(first, N * T, src.device)
        _arena.ensure(model)
        rel, pos = model._pos_state(src.device, drop)
        out = model._run(src, mask, by_ids, keep, first, pos, drop)
        ctx.model, ctx.mask, ctx.by_ids, ctx.first, ctx.pos, ctx.k = model, mask, by_ids, first, pos, model.trainable_layers
        ctx.rel, ctx.emb, ctx.drop = rel, emb, drop
        ctx.save_for_backward(src, keep)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        src, keep = ctx.saved_tensors
        need_in = not ctx.by_ids and ctx.needs_input_grad[1]
        k = ctx.k if any(ctx.needs_input_grad[5:]) else 0         # (torch.autograd.grad for the embeddings alone: no weight gradients)
        grad = None
        if need_in or k:
            grad = ctx.model._backward(src, ctx.by_ids, ctx.mask, keep, ctx.first, ctx.pos, ctx.rel, dout.contiguous(), need_in, k,
                                       ctx.emb and k > 0, ctx.drop)
        return (None, grad, None, None, None) + (None,) * (len(ctx.needs_input_grad) - 5)


class NativeDeberta(FrozenBackbone):
    """HuggingFace ``DebertaV2Model`` (inference), the v3 family, defaults = deberta-v3-base.

    ``forward(input_ids=None, attention_mask=None, inputs_embeds=None)`` -> ``.last_hidden_state`` (N, T, hidden) f32.
    ``input_ids`` (N, T) int64 or ``inputs_embeds`` (N, T, hidden) f32, on the GPU, exactly one of them; ``attention_mask``
    (N, T) of any integer / bool / float dtype, or None for all ones.  Masked keys get probability exactly 0; a masked query
    row attends uniformly over all T keys, so padded rows of the result are HuggingFace's too.  With grad mode on and
    ``inputs_embeds.requires_grad`` the result carries the gradient with respect to ``inputs_embeds``; after
    ``set_trainable_layers(k)``, ``k > 0``, every call in grad mode carries the top ``k`` layers' weight gradients.
    ``state_dict()`` has the keys, shapes and order of ``DebertaV2Model``; Q/K/V are stored fused and split on the way."""

    def __init__(self, vocab_size: int = 128100, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, max_position_embeddings: int = 512, position_buckets: int = 256,
                 layer_norm_eps: float = 1e-7, relative_attention: bool = True, share_att_key: bool = True,
                 pos_att_type=("p2c", "c2p"), norm_rel_ebd: str = "layer_norm", position_biased_input: bool = False,
                 type_vocab_size: int = 0, conv_kernel_size: int = 0, max_relative_positions: int = -1, hidden_act: str = "gelu",
                 embedding_size: Optional[int] = None, chunk: int = DEFAULT_CHUNK, hidden_dropout_prob: float = 0.0,
                 attention_probs_dropout_prob: float = 0.0):
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
            hidden_act="gelu", model_type="deberta-v2", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        self.set_dropout(hidden_dropout_prob, attention_probs_dropout_prob)
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
        self._embeddings = False                       # set_trainable_layers(L, embeddings=True)

    # -- dropout -------------------------------------------------------------------------------------------
    def set_dropout(self, hidden: float = 0.0, attention: float = 0.0) -> None:
        """``config.hidden_dropout_prob`` (the embeddings, every layer's relative embeddings, attention output and MLP output) and
        ``config.attention_probs_dropout_prob`` (the attention probabilities), each in [0, 1); HuggingFace's deberta-v3-base has 0.1
        for both, the default here is 0 for both: off.  They act in training mode, on the differentiable route only (grad mode on
        and something to train: ``set_trainable_layers`` or ``inputs_embeds.requires_grad``); ``eval()`` and ``no_grad`` calls are
        the inference launches whatever the values."""
        for name, p in (("hidden", hidden), ("attention", attention)):
            _check_probability("NativeDeberta: set_dropout", name, p)
        self.config.hidden_dropout_prob, self.config.attention_probs_dropout_prob = float(hidden), float(attention)

    def _drop_of_call(self) -> Optional[_Drop]:
        """the dropout of the differentiable call that is about to run: None unless the module trains with a probability above 0"""
        c = self.config
        if not self.training or (c.hidden_dropout_prob <= 0.0 and c.attention_probs_dropout_prob <= 0.0):
            return None
        self._own_training_forward()
        return _Drop(c.hidden_dropout_prob, c.attention_probs_dropout_prob, c.num_hidden_layers)

    # -- fine-tuning -------------------------------------------------------------------------------------
    _EMBEDDING_PARAMS = ("word_emb", "emb_ln_w", "emb_ln_b", "rel_emb", "enc_ln_w", "enc_ln_b")

    @property
    def trainable_embeddings(self) -> bool:
        return self._embeddings

    def set_trainable_layers(self, k: int, embeddings: bool = False) -> None:
        """The parameters of the top ``k`` layers (``L - k .. L - 1``) get ``requires_grad = True``, every other parameter
        ``False``; 0 freezes the backbone again.  ``embeddings=True`` (with ``k == L`` only: their gradient comes through every
        layer, the relative embeddings' through every layer's position path) also trains the word embeddings, the embedding
        LayerNorm, ``rel_embeddings`` and the encoder LayerNorm: every parameter, as the reference's optimiser trains the model.
        With grad mode on and ``k > 0`` a call returns a result that carries a graph, and its backward adds those parameters'
        gradients into their f32 ``.grad`` (the module's parameter arena) and stops below layer ``L - k`` unless ``inputs_embeds``
        or the embeddings need a gradient too.  Without ``embeddings`` the six embedding-side tensors stay frozen whatever ``k``.
        Dropout is ``set_dropout``'s; the fp32 parity mode is refused as everywhere in this class."""
        L = self.config.num_hidden_layers
        self._check_trainable(k, "embeddings", embeddings, "the embeddings train", "their gradient comes through every layer")
        if self._embeddings and not embeddings:        # (steps taken while ``rel_embeddings`` trained moved no version counter)
            self._cache.pop("pos", None)
        self._trainable, self._embeddings = k, embeddings
        self._require_grad([n for i in range(L - k, L) for n in self._layer_params(i)] + list(self._EMBEDDING_PARAMS if embeddings else ()))

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

    def _grad_table(self, T: int) -> WsTable:
        """what the backward holds beside the forward workspace, per item of ``T`` tokens: the layers' part (``_grad_rows``) and
        the lse of the attention it runs again (the forward workspace's is not written by ``mmf_deberta_attn_fwd``)"""
        return self._grad_rows(T) + [("lse", self.config.num_attention_heads * T, torch.float32)]

    def grad_workspace_bytes_per_item(self, T: int) -> int:
        return self._bytes_per_item(self._grad_table(T))

    def _grad_scratch(self) -> Tuple[int, Dict[str, int]]:
        return self.config.hidden_size, {}             # (every bias takes its column sum here: nothing goes to ``junk``)

    def _pos_workspace(self, g: dict, n: int, T: int) -> torch.Tensor:
        """``mmf_deberta_attn_bwd_pos``'s workspace for chunks of up to ``n`` items of ``T`` tokens, kept beside the backward's
        buffers and grown on demand"""
        c = self.config
        need = lib.deberta_attn_bwd_pos_workspace_bytes(n, c.num_attention_heads, T, c.position_buckets) // 4
        w = g.get("pos_ws")
        if w is None or w.numel() < need:
            w = g["pos_ws"] = torch.empty(need, dtype=torch.float32, device=g["dev"])
        return w

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
    def _pos_cache(self, dev) -> tuple:
        """(LayerNorm(rel_embeddings) as bf16 (2S, d), [(posQ, posK) of every FROZEN layer]): what depends on frozen weights only,
        one mmf_deberta_embed launch on the relative table and one GEMM per frozen layer, once per weight version.  With the
        embeddings trainable ``rel`` itself is computed in every call and no layer is frozen: the rule ``_pos_tables`` states"""
        c = self.config
        frozen = c.num_hidden_layers - self._trainable

        def build():
            rel = torch.empty((2 * c.position_buckets, c.hidden_size), dtype=BF16, device=dev)
            lib.deberta_embed(rel, None, self._f("enc_ln_w"), self._f("enc_ln_b"), c.layer_norm_eps, embeds=self._f("rel_emb"))
            return rel, [self._pos_of(i, rel) for i in range(frozen)]
        if self._embeddings:
            with torch.no_grad():
                return build()
        names = ["rel_emb", "enc_ln_w", "enc_ln_b"] + [f"l{i}_qkv_{s}" for i in range(frozen) for s in "wb"]
        return self._derived("pos", names, build)

    def _pos_of(self, i: int, rel: torch.Tensor) -> tuple:
        d = self.config.hidden_size
        qk = torch.empty((rel.shape[0], 2 * d), dtype=BF16, device=rel.device)
        ops.gemm(GEMM_NT, rel, self._w(f"l{i}_qkv_w")[:2 * d], qk, bias=self._f(f"l{i}_qkv_b")[:2 * d], epilogue=EPI_BIAS)
        return qk[:, :d], qk[:, d:]

    def _pos_tables(self, dev) -> list:
        """per layer (posQ, posK) = the layer's q / k projection (bias included) of LayerNorm(rel_embeddings): bf16 (2S, d) views
        of one (2S, 2d) GEMM output.  A frozen layer's are computed once per weight version.  A trainable layer's are computed in
        every call, from ``rel`` (cached while ``rel_embeddings`` and the encoder LayerNorm are frozen): the optimiser writes
        masters and shadows through raw pointers, which moves no version counter, so nothing derived from a trainable weight
        may be cached"""
        return self._pos_state(dev)[1]

    def _pos_state(self, dev, drop: Optional[_Drop] = None) -> tuple:
        """(``rel`` = LayerNorm(rel_embeddings) as bf16 (2S, d), ``_pos_tables``' list computed from it).  With hidden dropout
        every layer's tables come from its own ``rel_i`` = dropout_i(rel) and are computed in this call, a frozen layer's too
        (the mask is the call's); ``rel`` itself is the cached one while frozen"""
        rel, pos = self._pos_cache(dev)
        if drop is not None and drop.p_h > 0.0:
            return rel, [self._pos_of(i, self._rel_of(i, rel, drop)) for i in range(self.config.num_hidden_layers)]
        return rel, list(pos) + [self._pos_of(i, rel) for i in range(len(pos), self.config.num_hidden_layers)]

    @staticmethod
    def _rel_of(i: int, rel: torch.Tensor, drop: _Drop) -> torch.Tensor:
        """layer ``i``'s dropped relative embeddings (one item: sub-stream 0, index row * d + column), rounded once"""
        rel_i = torch.empty_like(rel)
        lib.hidden_dropout(rel, rel_i, 1, drop.hidden(drop.layers[i][_Drop.REL], 0))
        return rel_i

    # -- launches ---------------------------------------------------------------------------------------
    def _layer(self, i: int, ws, n: int, T: int, pos, idx: torch.Tensor, mask: Optional[torch.Tensor], drop: Optional[_Drop] = None,
               n0: int = 0) -> None:
        """a post-LN layer around the disentangled attention: ``pos`` = this layer's (posQ, posK), ``idx`` the index table,
        ``mask`` the chunk's (n, T) mask or None; ``drop``: the call's dropout, ``n0`` the chunk's first item in the batch"""
        c, scale = self.config, math.sqrt(3.0 * self.head_dim)
        probs = drop.probs(i, n0) if drop is not None else None

        def attend(qkv: torch.Tensor, att: torch.Tensor) -> None:
            lib.deberta_attn_fwd(qkv, pos[0], pos[1], idx, mask, att, n, c.num_attention_heads, T, c.position_buckets, scale, self.head_dim,
                                 drop=probs)
        self._post_ln_layer(i, ws, n, T, attend, self._hidden_joins(drop, drop and drop.join_sites(i), n, n0)[0])

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
        if torch.is_grad_enabled() and (self._trainable > 0 or (inputs_embeds is not None and inputs_embeds.requires_grad)):
            L = c.num_hidden_layers
            params = [getattr(self, n) for i in range(L - self._trainable, L) for n in self._layer_params(i)]
            if self._embeddings:
                params += [getattr(self, n) for n in self._EMBEDDING_PARAMS]
            return BackboneOutput(_Differentiable.apply(self, src, mask, input_ids is not None, self._drop_of_call(), *params))
        return BackboneOutput(self._run(src, mask, input_ids is not None))

    def _run(self, src: torch.Tensor, mask: Optional[torch.Tensor], by_ids: bool, keep: Optional[torch.Tensor] = None,
             first: int = 0, pos: Optional[list] = None, drop: Optional[_Drop] = None) -> torch.Tensor:
        """the launch list on checked inputs -> (N, T, d) f32; ``keep`` (layers - first, N T, d) bf16: also copy the input of every
        layer from ``first`` up there; ``pos``: the layers' position tables where the caller has them already; ``drop``: the
        call's dropout (``pos`` is then ``_pos_state(dev, drop)``'s)"""
        c, d, dev = self.config, self.config.hidden_size, src.device
        N, T = src.shape[:2]
        _arena.ensure(self)
        pos, idx = self._pos_tables(dev) if pos is None else pos, self._index(T, dev)
        ws = self._workspace(dev, T)
        out = torch.empty((N, T, d), dtype=torch.float32, device=dev)
        table, gamma, beta = self._f("word_emb"), self._f("emb_ln_w"), self._f("emb_ln_b")
        for n0, n in self._chunks(N):
            x = self._rows(ws, "x", n * T, d)
            part, m = src[n0:n0 + n], None if mask is None else mask[n0:n0 + n]
            if by_ids:
                lib.deberta_embed(x, table, gamma, beta, c.layer_norm_eps, ids=part.reshape(-1), mask=m)
            else:
                lib.deberta_embed(x, None, gamma, beta, c.layer_norm_eps, embeds=part, mask=m)
            if drop is not None and drop.p_h > 0.0:
                lib.hidden_dropout(x, x, n, drop.hidden(drop.emb, n0))
            for i in range(c.num_hidden_layers):
                if keep is not None and i >= first:
                    keep[i - first, n0 * T:(n0 + n) * T].copy_(x)
                self._layer(i, ws, n, T, pos[i], idx, m, drop, n0)
            self._widen(x, out[n0:n0 + n])
        return out

    # -- the backward: input gradient and the trainable layers' weight gradients -------------------------------------
    def _layer_grad(self, i: int, ws, g, xin: torch.Tensor, n: int, T: int, pos, idx: torch.Tensor, mask: Optional[torch.Tensor],
                    dpos: Optional[torch.Tensor] = None, below: bool = True, drop: Optional[_Drop] = None, n0: int = 0) -> None:
        """layer ``i`` again from its saved input ``xin``, then its backward: ``ga`` holds the gradient of the layer's output on
        entry and, with ``below``, of ``xin`` on return.  ``dpos`` (2S, 2d) f32, for a trainable layer: the layer's weight, bias
        and LayerNorm gradients are added into the parameters' ``.grad`` and the gradient of posQ | posK into ``dpos``.  ``drop``,
        ``n0`` as in ``_layer``: the layer runs again under the forward's masks and its backward draws them once more"""
        c, d = self.config, self.config.hidden_size
        dims = (n, c.num_attention_heads, T, c.position_buckets, math.sqrt(3.0 * self.head_dim), self.head_dim)
        train = dpos is not None
        probs = drop.probs(i, n0) if drop is not None else None

        def attend(qkv: torch.Tensor, att: torch.Tensor) -> None:
            lib.deberta_attn_fwd(qkv, pos[0], pos[1], idx, mask, att, *dims, lse=g["lse"], drop=probs)

        def attn_bwd(qkv: torch.Tensor, att: torch.Tensor, datt: torch.Tensor, dqkv: torch.Tensor) -> None:
            if train:
                lib.deberta_attn_bwd_pos(qkv, pos[0], pos[1], idx, mask, att, g["lse"], datt, g["delta"], dqkv, dpos[:, :d], dpos[:, d:],
                                         self._pos_workspace(g, n, T), *dims, drop=probs)
            else:
                lib.deberta_attn_bwd(qkv, pos[0], pos[1], idx, mask, att, g["lse"], datt, g["delta"], dqkv, *dims, drop=probs)
        join, join_bwd = self._hidden_joins(drop, drop and drop.join_sites(i), n, n0)
        # the plain Q/K/V weight gradient, the key bias's column sum included: db_k has a real position-to-content term here
        self._post_ln_layer_grad(i, ws, g, xin, n, T, attend, attn_bwd, (lambda dqkv, x: self._wgrad(dqkv, x, f"l{i}_qkv")) if train else None,
                                 below, join=join, join_bwd=join_bwd)

    def _embed_workspace(self, g: dict, rows: int, d_rows: bool) -> tuple:
        """(``mmf_deberta_embed_bwd_params``' workspace for up to ``rows`` rows, with ``d_rows`` an f32 (rows, d) buffer for the
        rows' gradient where the caller has none), kept beside the backward's buffers and grown on demand"""
        d = self.config.hidden_size
        need = lib.deberta_embed_bwd_params_workspace_bytes(rows, d) // 4
        w, r = g.get("emb_ws"), g.get("d_rows")
        if w is None or w.numel() < need:
            w = g["emb_ws"] = torch.empty(need, dtype=torch.float32, device=g["dev"])
        if d_rows and (r is None or r.numel() < rows * d):
            r = g["d_rows"] = torch.empty(rows * d, dtype=torch.float32, device=g["dev"])
        return w, r[:rows * d].view(rows, d) if d_rows else None

    def _backward(self, src: torch.Tensor, by_ids: bool, mask: Optional[torch.Tensor], keep: torch.Tensor, first: int, pos: list,
                  rel: torch.Tensor, dout: torch.Tensor, need_in: bool, k: int, emb: bool = False,
                  drop: Optional[_Drop] = None) -> Optional[torch.Tensor]:
        """for the gradient ``dout`` (N, T, d) f32 of the result: with ``need_in``, -> d ``inputs_embeds`` (N, T, d) f32; with
        ``k > 0``, the gradients of the top ``k`` layers' parameters, added into their ``.grad``; with ``emb`` (``k == L``), also
        those of the six embedding-side parameters.  ``keep``: the saved inputs of the layers from ``first`` up, ``pos`` / ``rel``:
        the position tables the forward used and the normalised relative embeddings they were made from.  Without ``need_in``
        and ``emb`` the walk ends with layer ``first``'s weight gradients.  ``drop``: the forward's dropout, every mask drawn again"""
        c, d, dev = self.config, self.config.hidden_size, src.device
        N, T = src.shape[:2]
        L, S2 = c.num_hidden_layers, 2 * c.position_buckets
        hidden = drop is not None and drop.p_h > 0.0
        self._refuse_fp32()
        idx = self._index(T, dev)
        ws, g = self._workspace(dev, T), self._grad_workspace(dev, T)
        grad = torch.empty((N, T, d), dtype=torch.float32, device=dev) if need_in else None
        # the gradient of posQ | posK of each trainable layer, summed over the chunks in f32
        dpos = torch.zeros((k, S2, 2 * d), dtype=torch.float32, device=dev) if k else None
        for n0, n in self._chunks(N):
            rows = slice(n0 * T, (n0 + n) * T)
            m = None if mask is None else mask[n0:n0 + n]
            ga = self._rows(g, "ga", n * T, d)
            self._narrow(dout[n0:n0 + n], ga)
            for i in reversed(range(first, L)):
                self._layer_grad(i, ws, g, keep[i - first, rows], n, T, pos[i], idx, m, dpos[i - (L - k)] if i >= L - k else None,
                                 need_in or emb or i > first, drop, n0)
            if hidden and (need_in or emb):
                lib.hidden_dropout(ga, ga, n, drop.hidden(drop.emb, n0))      # through the embedding output's dropout
            if emb:
                # the embedding LayerNorm's parameters, and the word embeddings: the gathered rows' gradient (a buffer of the
                # backward's), scattered into the table's; on the embeds route the rows' gradient is d inputs_embeds itself
                gamma, into = self._f("emb_ln_w"), (self.emb_ln_w.grad, self.emb_ln_b.grad)
                wsp, d_rows = self._embed_workspace(g, n * T, by_ids or not need_in)
                if by_ids:
                    ids = src[n0:n0 + n].reshape(-1)
                    lib.deberta_embed_bwd_params(gamma, c.layer_norm_eps, m, ga, d_rows, *into, wsp, ids=ids, table=self._f("word_emb"))
                    lib.embedding_scatter_add(ids, d_rows, self.word_emb.grad, mask=m)
                else:
                    lib.deberta_embed_bwd_params(gamma, c.layer_norm_eps, m, ga, grad[n0:n0 + n].view(n * T, d) if need_in else d_rows,
                                                 *into, wsp, embeds=src[n0:n0 + n])
            elif need_in:
                lib.deberta_embed_bwd(src[n0:n0 + n], self._f("emb_ln_w"), c.layer_norm_eps, m, ga, grad[n0:n0 + n])
        if k:
            # the position path: posQ | posK = rel W_qk^T + b_qk is stored as bf16, so its gradient is rounded to bf16 there, once
            dp16 = ops.cast_to_bf16(dpos.view(k * S2, 2 * d)).view(k, S2, 2 * d)
            # db_q += colsum(dposQ); db_k takes no column sum: sum_r dposK[r] = sum_i (sum_j dS_ij) Q_i, and a softmax backward's
            # dS rows sum to zero, so the exact term is 0 and what the kernel's dposK sums to is rounding residue alone (delta
            # comes from the bf16 O: each row of dS sums to dO_i . (O_i - bf16(O_i)), the residue colsum(dK) carries once already)
            for i in range(L - k, L):
                w, b, dp = getattr(self, f"l{i}_qkv_w").grad, getattr(self, f"l{i}_qkv_b").grad, dp16[i - (L - k)]
                rel_i = self._rel_of(i, rel, drop) if hidden else rel              # what the layer's tables were projected from
                ops.gemm_group(GEMM_TN, [(dp[:, :d], rel_i, w[:d], b[:d], None)], EPI_ACCUM | EPI_COLSUM_A)
                ops.gemm_group(GEMM_TN, [(dp[:, d:], rel_i, w[d:2 * d], None, None)], EPI_ACCUM)
            if emb:
                # ... continued below posQ | posK: d rel = sum over the layers of dpos_i (2S, 2d) W_qk,i (2d, d), one NN launch per
                # layer adding into one f32 (2S, d) buffer in stream order (layer 0 writes it).  In-stream accumulation keeps the sum
                # in f32 in a fixed order with no partial buffer; a grouped launch into per-layer partials would hold L (2S, d) f32
                # slabs and need the slab sum behind it, for products of 2S rows that fill a fraction of the CUs either way.
                # rel is stored as bf16: d rel is rounded to bf16 there, once, and the relative table's LayerNorm backward adds
                # straight into rel_emb.grad and the encoder LayerNorm's gradients
                # With hidden dropout each layer's term is the gradient of its own rel_i and goes through that layer's mask before
                # the sum: one slab per layer, masked where it lies, then the slabs' sum in layer order
                drel = torch.empty((S2, d), dtype=torch.float32, device=dev)
                if hidden:
                    slabs = torch.empty((L, S2 * d), dtype=torch.float32, device=dev)
                    for i in range(L):
                        ops.gemm(GEMM_NN, dp16[i], self._w(f"l{i}_qkv_w")[:2 * d], slabs[i].view(S2, d))
                        lib.hidden_dropout(slabs[i], slabs[i], 1, drop.hidden(drop.layers[i][_Drop.REL], 0))
                    for s0 in range(0, L, lib.SUM_SLABS_MAX):
                        lib.sum_slabs(slabs[s0:s0 + lib.SUM_SLABS_MAX], drel, s0 > 0)
                else:
                    for i in range(L):
                        ops.gemm(GEMM_NN, dp16[i], self._w(f"l{i}_qkv_w")[:2 * d], drel, epilogue=EPI_ACCUM if i else 0)
                wsp, _ = self._embed_workspace(g, S2, False)
                lib.deberta_embed_bwd_params(self._f("enc_ln_w"), c.layer_norm_eps, None, ops.cast_to_bf16(drel), self.rel_emb.grad,
                                             self.enc_ln_w.grad, self.enc_ln_b.grad, wsp, embeds=self._f("rel_emb"), accumulate=True)
        return grad
