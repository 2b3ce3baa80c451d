"""The DeBERTa-v3 forward (HuggingFace ``DebertaV2Model`` in inference up to ``last_hidden_state``; the v3 family only:
relative attention with shared keys, ``pos_att_type = "p2c|c2p"``, layer-normed relative embeddings, no absolute positions,
no token types, no convolution, post-LN layers) restated as explicit tensor math, written from the architecture:

    x   = LayerNorm(word_embeddings[ids]) * mask
    rel = LayerNorm(rel_embeddings)                                    (2S, d), S = position_buckets
    per layer:  q, k, v = x Wq + bq, ...;  posQ = rel Wq + bq;  posK = rel Wk + bk   (the layer's own q / k projections)
        s[i, j] = (q_i . k_j + q_i . posK[idx(i - j)] + k_j . posQ[idx(i - j)]) / sqrt(3 head_dim)       per head
        s[i, j] = finfo.min where mask[i] mask[j] == 0;  p = softmax_j(s);  ctx = p v
        y = LayerNorm(x + ctx Wo + bo);  x = LayerNorm(y + gelu(y W1 + b1) W2 + b2)

``idx(delta) = clamp(bucket(delta) + S, 0, 2S - 1)`` with HuggingFace's log bucketing.  ``bucket`` is odd in delta, so the
content-to-position gather (index ``bucket(i - j) + S``) and the position-to-content gather (index ``-bucket(j - i) + S``,
transposed) use the same index; tests/test_deberta_cpu.py holds that to HuggingFace's own tables.  A fully masked query row
has every score at finfo.min and so attends uniformly over all T keys, exactly as HuggingFace's does.

It imports neither transformers nor the code under test.  Weights are a ``state_dict`` in ``DebertaV2Model``'s key naming.

``bf16_storage=True`` models the storage format of the HIP path, not its kernels: values are rounded to bf16 exactly where
that path writes bf16 to memory, and everything between two stores is computed in ``dtype``.  The rounding points:
  * the embedding kernel's output (after LayerNorm and mask);
  * the GEMM weights (read from the bf16 shadow); biases and norm parameters stay f32;
  * LayerNorm(rel_embeddings) (the embedding kernel's output on the relative table) and each layer's posQ / posK;
  * the fused q / k / v rows; the attention output; out-projection + bias + residual; each LayerNorm output;
  * the MLP's fc1 output before its bias (the GELU kernel adds the bias in f32) and the GELU output; fc2 + bias + residual.
Scores, bias terms and probabilities are never stored, so they are not rounded.
"""
import math
import types

import torch

from backbone_ref import _r, config_kwargs, gelu_erf, layer_norm  # noqa: F401  (the tests read them from here)


def tiny_config():
    return types.SimpleNamespace(vocab_size=300, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                 max_position_embeddings=32, position_buckets=8, layer_norm_eps=1e-7)


def base_config():
    return types.SimpleNamespace(vocab_size=128100, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                                 intermediate_size=3072, max_position_embeddings=512, position_buckets=256, layer_norm_eps=1e-7)


def hf_config_kwargs(cfg):
    """the keyword arguments of HuggingFace's ``DebertaV2Config`` for this family (tools/capture_deberta_golden.py and the tests
    that build a live ``DebertaV2Model``)"""
    return dict(vars(cfg), relative_attention=True, share_att_key=True, pos_att_type=["p2c", "c2p"], norm_rel_ebd="layer_norm",
                position_biased_input=False, type_vocab_size=0, max_relative_positions=-1, hidden_act="gelu",
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pad_token_id=0)


def hf_keys(cfg):
    """the ``DebertaV2Model`` state_dict: key -> shape, in HuggingFace's order"""
    d, I = cfg.hidden_size, cfg.intermediate_size
    out = {"embeddings.word_embeddings.weight": (cfg.vocab_size, d), "embeddings.LayerNorm.weight": (d,), "embeddings.LayerNorm.bias": (d,)}
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layer.{i}."
        for n in ("query_proj", "key_proj", "value_proj"):
            out[f"{a}attention.self.{n}.weight"], out[f"{a}attention.self.{n}.bias"] = (d, d), (d,)
        out[a + "attention.output.dense.weight"], out[a + "attention.output.dense.bias"] = (d, d), (d,)
        out[a + "attention.output.LayerNorm.weight"], out[a + "attention.output.LayerNorm.bias"] = (d,), (d,)
        out[a + "intermediate.dense.weight"], out[a + "intermediate.dense.bias"] = (I, d), (I,)
        out[a + "output.dense.weight"], out[a + "output.dense.bias"] = (d, I), (d,)
        out[a + "output.LayerNorm.weight"], out[a + "output.LayerNorm.bias"] = (d,), (d,)
    out["encoder.rel_embeddings.weight"] = (2 * cfg.position_buckets, d)
    out["encoder.LayerNorm.weight"], out["encoder.LayerNorm.bias"] = (d,), (d,)
    return out


def seeded_weights(cfg, seed: int = 0):
    """Weights with spread enough that the forward exercises everything: 1/sqrt(fan_in)-scaled matrices, the q / k projections
    1.5 times that (tests/w2v_ref.py's choice) so the softmax rows are far from uniform; unit-variance embeddings (word and
    relative); non-trivial biases and norm parameters."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in hf_keys(cfg).items():
        t = torch.randn(shape, generator=g)
        if k.endswith("LayerNorm.weight"):
            t = 1.0 + 0.2 * t
        elif k.endswith(".bias"):
            t = 0.1 * t
        elif "embeddings" in k:
            pass
        else:
            t = t / math.sqrt(shape[1]) * (1.5 if ("query_proj" in k or "key_proj" in k) else 1.0)
        sd[k] = t
    return sd


def log_bucket(delta: torch.Tensor, bucket_size: int, max_position: int) -> torch.Tensor:
    """HuggingFace's ``make_log_bucket_position`` on an int64 tensor of relative positions: its float32 operations (the true
    division, ``log``, ``ceil``, ``where``) in its order -> int64 buckets"""
    sign = torch.sign(delta)
    mid = bucket_size // 2
    abs_pos = torch.where((delta < mid) & (delta > -mid), torch.tensor(mid - 1).type_as(delta), torch.abs(delta))
    log_pos = torch.ceil(torch.log(abs_pos / mid) / torch.log(torch.tensor((max_position - 1) / mid)) * (mid - 1)) + mid
    return torch.where(abs_pos <= mid, delta.type_as(log_pos), log_pos * sign).to(torch.long)


def bucket_index(T: int, S: int, max_position: int) -> torch.Tensor:
    """int32 (2T - 1,): entry ``delta + T - 1`` = clamp(bucket(delta) + S, 0, 2S - 1) for delta = i - j in -(T-1) .. T-1"""
    delta = torch.arange(-(T - 1), T, dtype=torch.long)
    return torch.clamp(log_bucket(delta, S, max_position) + S, 0, 2 * S - 1).to(torch.int32)


def disentangled_attention(q, k, v, posq, posk, idx, mask, scale):
    """q, k, v (n, H, T, dh); posq, posk (H, 2S, dh); idx (2T - 1,) integer; mask (n, T) or None -> (n, H, T, dh).
    Forms the (T, T) bias explicitly: this is the definition, not the kernel."""
    n, H, T, dh = q.shape
    ar = torch.arange(T, device=q.device)
    ix = idx.to(q.device).long()[(ar[:, None] - ar[None, :]) + T - 1]                               # (T, T): idx(i - j)
    c2p = torch.gather(q @ posk.transpose(-1, -2), -1, ix.expand(n, H, T, T))                        # [i, j] = q_i . posK[idx(i-j)]
    p2c = torch.gather(k @ posq.transpose(-1, -2), -1, ix.t().expand(n, H, T, T)).transpose(-1, -2)  # [i, j] = k_j . posQ[idx(i-j)]
    s = (q @ k.transpose(-1, -2) + c2p + p2c) / scale
    if mask is not None:
        m = mask.to(q.device) != 0
        keep = (m[:, :, None] & m[:, None, :])[:, None]
        s = s.masked_fill(~keep, torch.finfo(s.dtype).min)
    return torch.softmax(s, dim=-1) @ v


def deberta_forward(sd, ids_or_embeds, mask, cfg, bf16_storage: bool = False, dtype=torch.float64):
    """-> last_hidden_state (N, T, d) in ``dtype``.  ``ids_or_embeds``: int64 ids (N, T) or float inputs_embeds (N, T, d);
    ``mask`` (N, T) of any dtype or None for all ones."""
    on, dev = bf16_storage, ids_or_embeds.device
    W = lambda key: _r(sd[key].to(dev, dtype), on, dtype)           # GEMM weights are read from the bf16 shadow
    F = lambda key: sd[key].to(dev, dtype)                          # biases, norm parameters and embedding tables stay f32 masters
    d, H, eps, S = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.position_buckets
    dh = d // H
    if ids_or_embeds.dtype in (torch.int64, torch.int32):
        emb = F("embeddings.word_embeddings.weight")[ids_or_embeds.long()]
    else:
        emb = ids_or_embeds.to(dtype)
    N, T = emb.shape[:2]
    m = None if mask is None else mask.to(dev)
    x = layer_norm(emb, F("embeddings.LayerNorm.weight"), F("embeddings.LayerNorm.bias"), eps)
    if m is not None:
        x = x * m.to(dtype).unsqueeze(-1)
    x = _r(x, on, dtype)
    rel = _r(layer_norm(F("encoder.rel_embeddings.weight"), F("encoder.LayerNorm.weight"), F("encoder.LayerNorm.bias"), eps), on, dtype)
    idx = bucket_index(T, S, cfg.max_position_embeddings)
    heads = lambda t: t.reshape(N, T, H, dh).transpose(1, 2)
    pos_heads = lambda t: t.reshape(2 * S, H, dh).transpose(0, 1)
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layer.{i}."
        s = a + "attention.self."
        lin = lambda t, name: t @ W(name + ".weight").T + F(name + ".bias")
        q, k, v = (_r(lin(x, s + n), on, dtype) for n in ("query_proj", "key_proj", "value_proj"))
        posq, posk = _r(lin(rel, s + "query_proj"), on, dtype), _r(lin(rel, s + "key_proj"), on, dtype)
        ctx = disentangled_attention(heads(q), heads(k), heads(v), pos_heads(posq), pos_heads(posk), idx, m, math.sqrt(3.0 * dh))
        ctx = _r(ctx.transpose(1, 2).reshape(N, T, d), on, dtype)
        y = _r(lin(ctx, a + "attention.output.dense") + x, on, dtype)
        y = _r(layer_norm(y, F(a + "attention.output.LayerNorm.weight"), F(a + "attention.output.LayerNorm.bias"), eps), on, dtype)
        f1 = _r(y @ W(a + "intermediate.dense.weight").T, on, dtype)                                  # GELU input as stored (the bias is added in f32)
        g = _r(gelu_erf(f1 + F(a + "intermediate.dense.bias")), on, dtype)
        z = _r(lin(g, a + "output.dense") + y, on, dtype)
        x = _r(layer_norm(z, F(a + "output.LayerNorm.weight"), F(a + "output.LayerNorm.bias"), eps), on, dtype)
    return x


class RefDeberta(torch.nn.Module):
    """``deberta_forward`` behind the ``backbone=`` protocol of ``TextEncoder`` (``.config``, ``.embeddings.word_embeddings``,
    ``input_ids`` / ``inputs_embeds`` / ``attention_mask`` keywords)"""

    def __init__(self, sd, cfg, dtype=torch.float32, bf16_storage: bool = False):
        super().__init__()
        self.sd, self.dtype, self.bf16_storage = sd, dtype, bf16_storage
        self.config = types.SimpleNamespace(**vars(cfg), model_type="deberta-v2")
        table = sd["embeddings.word_embeddings.weight"]
        self.embeddings = types.SimpleNamespace(word_embeddings=lambda ids: table.to(ids.device)[ids])

    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None):
        with torch.no_grad():
            x = input_ids if input_ids is not None else inputs_embeds
            out = deberta_forward(self.sd, x, attention_mask, self.config, bf16_storage=self.bf16_storage, dtype=self.dtype).float()
        return types.SimpleNamespace(last_hidden_state=out)
