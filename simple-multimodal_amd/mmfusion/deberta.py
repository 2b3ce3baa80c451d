"""Frozen DeBERTa-v3 backbone on the HIP kernels: token ids (or input embeddings) + attention mask -> token states, with the
gradient with respect to the input embeddings (prompt tuning); the weights never train.

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
layer's forward again from that ``x`` and then its backward:

      the layer's forward again, with                                     x -> qkv, att, lse, y1, ln1 (mean1, rstd1), h, g, y2
        mmf_deberta_attn_fwd_lse for the attention, mmf_bias_gelu_bf16_to for the GELU (h kept),
        and the second LayerNorm for its statistics                       y2 -> (mean2, rstd2)
      LayerNorm backward            mmf_layernorm_bwd_grouped            gx, y2 -> dy2
      fc2 dgrad                     mmf_gemm_grouped NN                  dy2 -> dg
      GELU backward                 mmf_bias_gelu_bwd_bf16 (in place)    dg, h -> dh
      fc1 dgrad + dy2               mmf_gemm_grouped NN, ADD_AUX         dh  -> dln1
      LayerNorm backward            mmf_layernorm_bwd_grouped            dln1, y1 -> dy1
      out-projection dgrad          mmf_gemm_grouped NN                  dy1 -> datt
      attention backward            mmf_deberta_attn_bwd (3 launches)    datt -> dqkv
      Q/K/V dgrad + dy1             mmf_gemm_grouped NN, ADD_AUX         dqkv -> gx of the layer below
    embedding backward              mmf_deberta_embed_bwd                gx  -> d inputs_embeds (f32)

Gradients are stored as bf16 exactly where the forward stores the activation they belong to (a residual join is summed in f32
in the GEMM epilogue and rounded once); the incoming gradient of ``last_hidden_state`` is rounded to bf16 once, the outgoing
one is f32.  The recomputation reuses the forward workspace; what the backward holds beside it (the second pre-LN sum, the GELU
output beside ``h``, both LayerNorms' statistics, lse, the gradient buffers and scratch) is a table of its own
(``_grad_table``), allocated on the first differentiable call.
"""
from __future__ import annotations

import math
import types
from typing import Dict, Optional, Tuple

import torch

from . import arena as _arena
from . import lib, ops
from .backbone import BF16, BackboneOutput, FrozenBackbone, WsTable
from .lib import EPI_ADD_AUX, EPI_BIAS, GEMM_NN, GEMM_NT

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


class _InputGrad(torch.autograd.Function):
    """``NativeDeberta._run`` on input embeddings, differentiable with respect to them"""

    @staticmethod
    def forward(ctx, model: "NativeDeberta", embeds: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
        N, T, d = embeds.shape
        keep = torch.empty((model.config.num_hidden_layers, N * T, d), dtype=BF16, device=embeds.device)
        out = model._run(embeds, mask, False, keep)
        ctx.model, ctx.mask = model, mask
        ctx.save_for_backward(embeds, keep)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        embeds, keep = ctx.saved_tensors
        return None, ctx.model._input_grad(embeds, ctx.mask, keep, dout.contiguous()), None


class NativeDeberta(FrozenBackbone):
    """HuggingFace ``DebertaV2Model`` (inference), the v3 family, defaults = deberta-v3-base.

    ``forward(input_ids=None, attention_mask=None, inputs_embeds=None)`` -> ``.last_hidden_state`` (N, T, hidden) f32.
    ``input_ids`` (N, T) int64 or ``inputs_embeds`` (N, T, hidden) f32, on the GPU, exactly one of them; ``attention_mask``
    (N, T) of any integer / bool / float dtype, or None for all ones.  Masked keys get probability exactly 0; a masked query
    row attends uniformly over all T keys, so padded rows of the result are HuggingFace's too.  With grad mode on and
    ``inputs_embeds.requires_grad`` the result carries the gradient with respect to ``inputs_embeds``.
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
        self._gws: Optional[dict] = None               # the backward's workspace (_grad_table), from the first differentiable call

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
        """what the backward holds beside the forward workspace, per item of ``T`` tokens: the second pre-LN sum, the GELU output
        (``h`` keeps the raw fc1 output), both LayerNorms' statistics, lse and delta, and the gradient buffers (``ga`` / ``gb``
        alternate as the d-wide gradients, ``dh`` is dg then dh)"""
        c = self.config
        d, H, I, f32 = c.hidden_size, c.num_attention_heads, c.intermediate_size, torch.float32
        return [("y2", T * d, BF16), ("g", T * I, BF16), ("ga", T * d, BF16), ("gb", T * d, BF16), ("dh", T * I, BF16),
                ("dqkv", T * 3 * d, BF16), ("mean1", T, f32), ("rstd1", T, f32), ("mean2", T, f32), ("rstd2", T, f32),
                ("lse", H * T, f32), ("delta", H * T, f32)]

    def grad_workspace_bytes_per_item(self, T: int) -> int:
        return self._bytes_per_item(self._grad_table(T))

    def _grad_workspace(self, dev, T: int) -> dict:
        g = self._gws
        if g is not None and g["dev"] == dev and g["chunk"] == self.chunk and g["size"] >= T:
            return g
        d = self.config.hidden_size
        g = {"dev": dev, "chunk": self.chunk, "size": T, "dgb": torch.empty(2 * d, dtype=torch.float32, device=dev),
             "ln_ws": torch.empty(lib.load().mmf_layernorm_bwd_workspace_bytes(d) // 4, dtype=torch.float32, device=dev)}
        for name, numel, dtype in self._grad_table(T):
            g[name] = torch.empty(self.chunk * numel, dtype=dtype, device=dev)
        self._gws = g
        return g

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
        if inputs_embeds is not None and torch.is_grad_enabled() and inputs_embeds.requires_grad:
            return BackboneOutput(_InputGrad.apply(self, src, mask))
        return BackboneOutput(self._run(src, mask, input_ids is not None))

    def _run(self, src: torch.Tensor, mask: Optional[torch.Tensor], by_ids: bool, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the launch list on checked inputs -> (N, T, d) f32; ``keep`` (layers, N T, d) bf16: also copy every layer's input there"""
        c, d, dev = self.config, self.config.hidden_size, src.device
        N, T = src.shape[:2]
        _arena.ensure(self)
        pos, idx = self._pos_tables(dev), self._index(T, dev)
        ws = self._workspace(dev, T)
        out = torch.empty((N, T, d), dtype=torch.float32, device=dev)
        table, gamma, beta = self._f("word_emb"), self._f("emb_ln_w"), self._f("emb_ln_b")
        for n0 in range(0, N, self.chunk):
            n = min(self.chunk, N - n0)
            x = self._rows(ws, "x", n * T, d)
            part, m = src[n0:n0 + n], None if mask is None else mask[n0:n0 + n]
            if by_ids:
                lib.deberta_embed(x, table, gamma, beta, c.layer_norm_eps, ids=part.reshape(-1), mask=m)
            else:
                lib.deberta_embed(x, None, gamma, beta, c.layer_norm_eps, embeds=part, mask=m)
            for i in range(c.num_hidden_layers):
                if keep is not None:
                    keep[i, n0 * T:(n0 + n) * T].copy_(x)
                self._layer(i, ws, n, T, pos[i], idx, m)
            self._widen(x, out[n0:n0 + n])
        return out

    # -- the input gradient ---------------------------------------------------------------------------------
    def _layer_grad(self, i: int, ws, g, xin: torch.Tensor, n: int, T: int, pos, idx: torch.Tensor, mask: Optional[torch.Tensor]) -> None:
        """layer ``i`` again from its saved input ``xin``, then its backward: ``ga`` holds the gradient of the layer's output on
        entry and of ``xin`` on return"""
        c, scale = self.config, math.sqrt(3.0 * self.head_dim)
        rows, d, H, S, I = n * T, c.hidden_size, c.num_attention_heads, c.position_buckets, c.intermediate_size
        R = self._rows
        ga, gb, dh, dqkv, y2, gel = R(g, "ga", rows, d), R(g, "gb", rows, d), R(g, "dh", rows, I), R(g, "dqkv", rows, 3 * d), R(g, "y2", rows, d), R(g, "g", rows, I)
        ln, h, qkv, att = R(ws, "ln", rows, d), R(ws, "h", rows, I), R(ws, "qkv", rows, 3 * d), R(ws, "att", rows, d)
        st1 = {"mean": g["mean1"], "rstd": g["rstd1"], "dgb": g["dgb"], "ln_ws": g["ln_ws"]}
        st2 = {"mean": g["mean2"], "rstd": g["rstd2"], "dgb": g["dgb"], "ln_ws": g["ln_ws"]}

        def attend(qkv_: torch.Tensor, att_: torch.Tensor) -> None:
            lib.deberta_attn_fwd(qkv_, pos[0], pos[1], idx, mask, att_, n, H, T, S, scale, self.head_dim, lse=g["lse"])
        y1 = self._attention(i, ws, xin, xin, n, T, attend)
        self._ln(st1, y1, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        ops.gemm(GEMM_NT, ln, self._w(f"l{i}_fc1_w"), h)
        lib.bias_gelu_to(h, self._f(f"l{i}_fc1_b"), gel)
        ops.gemm(GEMM_NT, gel, self._w(f"l{i}_fc2_w"), y2, bias=self._f(f"l{i}_fc2_b"), aux=ln, epilogue=EPI_BIAS | EPI_ADD_AUX)
        self._ln(st2, y2, R(ws, "x", rows, d), f"l{i}_ln2_w", f"l{i}_ln2_b")          # for its statistics; the output is not read

        self._ln_bwd(st2, y2, ga, gb, f"l{i}_ln2_w")                                  # gb = dy2
        ops.gemm(GEMM_NN, gb, self._w(f"l{i}_fc2_w"), dh)                             # dg
        lib.bias_gelu_bwd(dh, h, self._f(f"l{i}_fc1_b"), dh)
        ops.gemm(GEMM_NN, dh, self._w(f"l{i}_fc1_w"), ga, aux=gb, epilogue=EPI_ADD_AUX)          # ga = dln1: the MLP branch + the residual
        self._ln_bwd(st1, y1, ga, gb, f"l{i}_ln1_w")                                  # gb = dy1
        ops.gemm(GEMM_NN, gb, self._w(f"l{i}_o_w"), ga)                               # ga = datt
        lib.deberta_attn_bwd(qkv, pos[0], pos[1], idx, mask, att, g["lse"], ga, g["delta"], dqkv, n, H, T, S, scale, self.head_dim)
        ops.gemm(GEMM_NN, dqkv, self._w(f"l{i}_qkv_w"), ga, aux=gb, epilogue=EPI_ADD_AUX)        # ga = dx: the attention branch + the residual

    def _input_grad(self, embeds: torch.Tensor, mask: Optional[torch.Tensor], keep: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
        """d ``inputs_embeds`` (N, T, d) f32 for the gradient ``dout`` (N, T, d) f32 of the result; ``keep``: the layers' saved inputs"""
        c, d, dev = self.config, self.config.hidden_size, embeds.device
        N, T = embeds.shape[:2]
        if ops.fp32_mode():
            raise RuntimeError("NativeDeberta runs with bf16 storage only: it has no form for the fp32 parity mode (and no eager fallback)")
        pos, idx = self._pos_tables(dev), self._index(T, dev)
        ws, g = self._workspace(dev, T), self._grad_workspace(dev, T)
        grad = torch.empty((N, T, d), dtype=torch.float32, device=dev)
        for n0 in range(0, N, self.chunk):
            n = min(self.chunk, N - n0)
            rows = slice(n0 * T, (n0 + n) * T)
            m = None if mask is None else mask[n0:n0 + n]
            ga = self._rows(g, "ga", n * T, d)
            self._narrow(dout[n0:n0 + n], ga)
            for i in reversed(range(c.num_hidden_layers)):
                self._layer_grad(i, ws, g, keep[i, rows], n, T, pos[i], idx, m)
            lib.deberta_embed_bwd(embeds[n0:n0 + n], self._f("emb_ln_w"), c.layer_norm_eps, m, ga, grad[n0:n0 + n])
        return grad
