"""BERT / RoBERTa backbones on the HIP kernels: token ids (or input embeddings) -> hidden states, frozen.

``NativeBert`` is HuggingFace's ``BertModel`` and ``NativeRoberta`` its ``RobertaModel`` (encoder only, absolute position
embeddings) rebuilt from their sizes alone, with HuggingFace's ``state_dict`` surface.  The layer is the post-LN block the other
backbones share (mmfusion/backbone.py); what is this family's own is the embedding row and an attention that honours a key
padding mask.  The launch list of a chunk of ``n`` items of ``T`` tokens:

      embeddings                    mmf_bert_embed                       ids | embeds, token types -> x (bf16)
      (once per call, all items)    mmf_mask_pack                        attention_mask -> packed (bits, last valid key, count)
      per layer                     FrozenBackbone._post_ln_layer with
        attention                   mmf_attn_fwd_keymask                 qkv, packed -> att (lse is written too)
      result                        mmf_cast_bf16_to_f32                 x -> last_hidden_state

``mmf_bert_embed`` is word + token-type + position rows and the LayerNorm in one pass.  BERT's position of a token is its place;
RoBERTa's is HuggingFace's ``create_position_ids_from_input_ids``, ``pad + (ids != pad among the item's tokens up to this one)``
for a non-pad id and ``pad`` for a pad, which the kernel counts itself from the ids (never from ``attention_mask``); on the
``inputs_embeds`` route it is ``pad + 1 + place``.  The attention masks KEYS only: a masked key has probability exactly 0, every
query row is computed (padded rows of the result are HuggingFace's eager rows too), and an item without a valid key attends
uniformly over all its keys.  The kernel skips 32-key blocks without a valid key and never reads tiles behind an item's last valid
key, so a padded batch costs what its tokens cost; no (T, T) tensor exists anywhere.  Nothing synchronises with the host and the
mask is packed on the device, so a captured graph replays with other ids and another mask.

``pooler.dense`` is held for the ``state_dict`` surface (``add_pooling_layer=True``, what ``AutoModel`` builds) and never computed:
``pooler_output`` is None.

Frozen forward only.  Refused, each with an error that names the class: ``set_trainable_layers(k > 0)``, ``set_dropout`` above 0,
``inputs_embeds.requires_grad`` in grad mode (no backward is built: prompt tuning would silently get no gradient),
``position_embedding_type`` other than "absolute", ``hidden_act`` other than "gelu", ``is_decoder`` / cross-attention, more tokens
than the position table holds, the fp32 parity mode, CPU tensors.
"""
from __future__ import annotations

import types
from typing import Optional

import torch

from . import arena as _arena
from . import lib
from .backbone import BackboneOutput, FrozenBackbone, WsTable, _check_probability
from .deberta import _WordEmbeddings

DEFAULT_CHUNK = 16

# constructor kwargs of the released families for both classes, over each class's defaults (bert-base-uncased / roberta-base; the
# large models differ from them in these four sizes only)
FAMILIES = {"base": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072),
            "large": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)}


class NativeBert(FrozenBackbone):
    """HuggingFace ``BertModel`` (inference, absolute positions), defaults = bert-base-uncased.

    ``forward(input_ids=None, attention_mask=None, inputs_embeds=None, token_type_ids=None)`` -> ``.last_hidden_state`` (N, T,
    hidden) f32.  ``input_ids`` (N, T) int64 or ``inputs_embeds`` (N, T, hidden) f32, on the GPU, exactly one of them;
    ``attention_mask`` (N, T) of any integer / bool / float dtype, or None for all ones; ``token_type_ids`` (N, T) int64 or None for
    type 0.  ``state_dict()`` has the keys, shapes and order of ``BertModel``; Q/K/V are stored fused and split on the way."""

    MODEL_TYPE, RULE = "bert", "bert"
    # HuggingFace's order of the embedding keys
    _EMB_ORDER = ("word_embeddings", "position_embeddings", "token_type_embeddings", "LayerNorm")

    def __init__(self, vocab_size: int = 30522, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, max_position_embeddings: int = 512, type_vocab_size: int = 2,
                 layer_norm_eps: float = 1e-12, pad_token_id: int = 0, hidden_act: str = "gelu",
                 position_embedding_type: str = "absolute", is_decoder: bool = False, add_cross_attention: bool = False,
                 add_pooling_layer: bool = True, chunk: int = DEFAULT_CHUNK, hidden_dropout_prob: float = 0.0,
                 attention_probs_dropout_prob: float = 0.0):
        who = type(self).__name__
        d, H, I = int(hidden_size), int(num_attention_heads), int(intermediate_size)
        if position_embedding_type != "absolute":
            raise ValueError(f"{who}: position_embedding_type={position_embedding_type!r}: only 'absolute' is built")
        if hidden_act != "gelu":
            raise ValueError(f"{who}: hidden_act={hidden_act!r}: only the exact 'gelu' is built")
        if is_decoder or add_cross_attention:
            raise ValueError(f"{who}: is_decoder={is_decoder!r}, add_cross_attention={add_cross_attention!r}: the encoder alone is "
                             "built (no causal mask, no cross-attention)")
        super().__init__(d, H, chunk)
        if vocab_size < 1 or type_vocab_size < 1 or max_position_embeddings < 1 or I % 8 or I < 8:
            raise ValueError(f"{who}: vocab_size {vocab_size}, type_vocab_size {type_vocab_size} and max_position_embeddings "
                             f"{max_position_embeddings} at least 1, intermediate_size {I} a multiple of 8")
        if not 0 <= pad_token_id < vocab_size:
            raise ValueError(f"{who}: pad_token_id {pad_token_id} is outside the vocabulary of {vocab_size}")
        if num_hidden_layers < 1 or chunk < 1:
            raise ValueError(f"{who}: layers and chunk at least 1")
        self.config = types.SimpleNamespace(
            vocab_size=int(vocab_size), hidden_size=d, num_hidden_layers=int(num_hidden_layers), num_attention_heads=H,
            intermediate_size=I, max_position_embeddings=int(max_position_embeddings), type_vocab_size=int(type_vocab_size),
            layer_norm_eps=float(layer_norm_eps), pad_token_id=int(pad_token_id), hidden_act="gelu",
            position_embedding_type="absolute", is_decoder=False, add_cross_attention=False, model_type=self.MODEL_TYPE,
            hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        self.set_dropout(hidden_dropout_prob, attention_probs_dropout_prob)
        emb = {"word_embeddings": lambda k: self._add("word_emb", (vocab_size, d), k + ".weight"),
               "position_embeddings": lambda k: self._add("pos_emb", (max_position_embeddings, d), k + ".weight"),
               "token_type_embeddings": lambda k: self._add("type_emb", (type_vocab_size, d), k + ".weight"),
               "LayerNorm": lambda k: (self._add("emb_ln_w", (d,), k + ".weight", ones=True), self._add("emb_ln_b", (d,), k + ".bias", std=0.0))}
        for name in self._EMB_ORDER:
            emb[name]("embeddings." + name)
        for i in range(num_hidden_layers):
            a, att = f"encoder.layer.{i}.", f"encoder.layer.{i}.attention."
            self._add_layer(i, d, I, {"q": att + "self.query", "k": att + "self.key", "v": att + "self.value",
                                      "o": att + "output.dense", "ln1": att + "output.LayerNorm", "fc1": a + "intermediate.dense",
                                      "fc2": a + "output.dense", "ln2": a + "output.LayerNorm"})
        if add_pooling_layer:                                  # held, never computed
            self._add("pooler_w", (d, d), "pooler.dense.weight")
            self._add("pooler_b", (d,), "pooler.dense.bias", std=0.0)
        self.embeddings = types.SimpleNamespace(word_embeddings=_WordEmbeddings(self))

    # -- frozen only ------------------------------------------------------------------------------------------
    def set_trainable_layers(self, k: int, embeddings: bool = False) -> None:
        """0 only: a frozen backbone (no backward of the key-masked attention or of the embedding row is built)"""
        if isinstance(k, bool) or k != 0 or embeddings:
            raise ValueError(f"{type(self).__name__}: set_trainable_layers({k!r}, embeddings={embeddings!r}): the backbone is frozen; "
                             "no backward of the key-masked attention is built yet")
        self._trainable = 0
        self._require_grad(())

    def set_dropout(self, hidden: float = 0.0, attention: float = 0.0) -> None:
        """both must stay 0: dropout acts in a differentiable training call, which this frozen model has none of"""
        who = f"{type(self).__name__}: set_dropout"
        for name, p in (("hidden", hidden), ("attention", attention)):
            _check_probability(who, name, p)
            if p != 0:
                raise ValueError(f"{who}({name}={p!r}): training-mode dropout is not built for this frozen backbone; it stays at 0")

    # -- shapes / workspace -----------------------------------------------------------------------------
    def _ws_table(self, T: int) -> WsTable:
        """per item of ``T`` tokens"""
        return self._token_table(T, T * self.config.intermediate_size)

    def workspace_bytes_per_item(self, T: int) -> int:
        return self._bytes_per_item(self._ws_table(T))

    def _first_position(self) -> int:
        """the position-table row of an item's first token when nothing is a pad"""
        return 0

    # -- launches ---------------------------------------------------------------------------------------
    def _embed(self, x: torch.Tensor, T: int, ids, embeds, types_) -> None:
        c = self.config
        lib.bert_embed(x, self._f("word_emb"), self._f("pos_emb"), self._f("type_emb"), self._f("emb_ln_w"), self._f("emb_ln_b"),
                       c.layer_norm_eps, T, self.RULE, c.pad_token_id, ids=ids, embeds=embeds, token_type_ids=types_)

    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None, token_type_ids=None) -> BackboneOutput:
        c, who = self.config, type(self).__name__
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
            if torch.is_grad_enabled() and inputs_embeds.requires_grad:
                raise RuntimeError(f"{who}: inputs_embeds requires a gradient, and no backward is built for this frozen backbone "
                                   "(prompt tuning would get no gradient); call it under no_grad or detach the embeddings")
            src = inputs_embeds.detach().contiguous()
        N, T = src.shape[:2]
        room = c.max_position_embeddings - self._first_position()
        if N < 1 or not 1 <= T <= room:
            raise ValueError(f"{who}: {N} items of {T} tokens: at least one item, and 1 .. {room} tokens (max_position_embeddings "
                             f"{c.max_position_embeddings}, the first token at position {self._first_position()})")
        dev = src.device
        mask = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (N, T) or attention_mask.device != dev:
                raise ValueError(f"{who}: attention_mask {tuple(attention_mask.shape)} is not (N, T) = ({N}, {T}) on the inputs' device")
            mask = attention_mask if attention_mask.dtype in (torch.float32, torch.uint8, torch.bool) else attention_mask.to(torch.float32)
            mask = mask.contiguous()
        if token_type_ids is not None:
            if tuple(token_type_ids.shape) != (N, T) or token_type_ids.device != dev or token_type_ids.dtype != torch.int64:
                raise ValueError(f"{who}: token_type_ids must be int64 (N, T) = ({N}, {T}) on the inputs' device")
            token_type_ids = token_type_ids.contiguous()
        with torch.no_grad():
            return BackboneOutput(self._run(src, mask, token_type_ids, input_ids is not None))

    def _run(self, src: torch.Tensor, mask: Optional[torch.Tensor], types_: Optional[torch.Tensor], by_ids: bool) -> torch.Tensor:
        """the launch list on checked inputs -> (N, T, d) f32"""
        c, d, dh, dev = self.config, self.config.hidden_size, self.head_dim, src.device
        N, T = src.shape[:2]
        _arena.ensure(self)
        ws = self._workspace(dev, T)
        out = torch.empty((N, T, d), dtype=torch.float32, device=dev)
        words = lib.mask_pack_words(T)
        packed = torch.empty(N * words, dtype=torch.int32, device=dev)
        lib.mask_pack(mask, packed, N, T)                      # once per call, every layer of every chunk reads it
        for n0, n in self._chunks(N):
            x = self._rows(ws, "x", n * T, d)
            part, tt = src[n0:n0 + n], None if types_ is None else types_[n0:n0 + n].reshape(-1)
            self._embed(x, T, part.reshape(-1) if by_ids else None, None if by_ids else part, tt)
            rows = packed[n0 * words:(n0 + n) * words]

            def attend(qkv: torch.Tensor, att: torch.Tensor) -> None:
                lib.attn_fwd_keymask(self._attn_problem(ws, qkv, att, n, T, T), dh, dh ** -0.5, rows)
            for i in range(c.num_hidden_layers):
                self._post_ln_layer(i, ws, n, T, attend)
            self._widen(x, out[n0:n0 + n])
        return out


class NativeRoberta(NativeBert):
    """HuggingFace ``RobertaModel`` (inference, absolute positions), defaults = roberta-base: ``NativeBert`` with RoBERTa's
    position ids (from the ids and ``pad_token_id``, counted on the device), one token type and eps 1e-5.  ``state_dict()`` has the
    keys, shapes and order of ``RobertaModel``."""

    MODEL_TYPE, RULE = "roberta", "roberta"
    _EMB_ORDER = ("word_embeddings", "token_type_embeddings", "LayerNorm", "position_embeddings")

    def __init__(self, vocab_size: int = 50265, hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
                 intermediate_size: int = 3072, max_position_embeddings: int = 514, type_vocab_size: int = 1,
                 layer_norm_eps: float = 1e-5, pad_token_id: int = 1, **kw):
        super().__init__(vocab_size, hidden_size, num_hidden_layers, num_attention_heads, intermediate_size, max_position_embeddings,
                         type_vocab_size, layer_norm_eps, pad_token_id, **kw)

    def _first_position(self) -> int:
        return self.config.pad_token_id + 1
