"""The DeBERTa-v3 forward in training mode (HuggingFace ``DebertaV2Model`` in ``train()``): tests/deberta_ref.py's
``deberta_forward`` with the five dropout masks as explicit inputs, the closed-form backward of the attention with dropped
probabilities, and the host restatement of the keep-mask each site of the HIP path draws.  It imports neither transformers nor the
code under test.

The five sites, in ``DebertaV2Model``'s call order (``Sites``: 1 + 4 per layer, numbered from ``first``):

    emb        x     = dropout(LayerNorm(word_embeddings[ids]) * mask)
    rel[i]     rel_i = dropout_i(LayerNorm(rel_embeddings)); layer i's posQ | posK are its q / k projections of rel_i
    probs[i]   ctx   = dropout(softmax(s)) v
    out[i]     y     = LayerNorm(dropout(ctx Wo + bo) + x)
    mlp[i]     x     = LayerNorm(dropout(gelu(..) W2 + b2) + y)

A mask is a bool tensor (True = kept) and the kept values are multiplied by ``c`` = 1 / (1 - p) as the kernels form it in f32
(``attn_ref.inv_keep_of``).  ``bf16_storage`` adds these rounding points to ``deberta_ref``'s: dense + bias is rounded before its
dropout, dropout + residual is rounded once, the dropped embedding output and every ``rel_i`` are rounded once more; probabilities
are never stored.

Keying (csrc/deberta.hip, csrc/elementwise.hip).  Every mask is ``mmf_keep(mmf_rng_key(state, site, sub), index, thresh)`` of tests/attn_ref.py:
  hidden sites    sub = the item's index in the whole batch, index = t * d + column      (``hidden_keep``)
  rel[i]          one item: sub = 0, index = row * d + column
  probs[i]        sub = item * H + head, index = i * T + j for query i and key j         (``probs_keep``)
so a mask is a function of the element and not of how the batch is cut into chunks."""
import math
import types

import numpy as np
import torch

import attn_ref
import deberta_grad_ref as G
import deberta_ref
from backbone_ref import _r, gelu_erf, layer_norm


def sites(layers: int, first: int = 1):
    """the call's sites in order -> namespace(emb, rel[i], probs[i], out[i], mlp[i])"""
    s = iter(range(first, first + 1 + 4 * layers))
    ns = types.SimpleNamespace(emb=next(s), rel=[], probs=[], out=[], mlp=[])
    for _ in range(layers):
        ns.rel.append(next(s)), ns.probs.append(next(s)), ns.out.append(next(s)), ns.mlp.append(next(s))
    return ns


def hidden_keep(state, site, item0, items, per_item, thresh):
    """(items, per_item) bool: element e of item g from sub-stream item0 + g, index e"""
    key = attn_ref.mmf_rng_key(state, site, np.arange(item0, item0 + items, dtype=np.uint64))
    keep = attn_ref.mmf_keep(key[:, None], np.arange(per_item, dtype=np.uint64)[None, :], thresh)
    return torch.from_numpy(keep)


def probs_keep(state, site, item0, items, H, T, thresh):
    """(items, H, T, T) bool: pair (query i, key j) of head h of item g from sub-stream (item0 + g) H + h, index i T + j"""
    sub = (np.arange(item0, item0 + items, dtype=np.uint64)[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :]).reshape(-1)
    key = attn_ref.mmf_rng_key(state, site, sub)
    keep = attn_ref.mmf_keep(key[:, None], np.arange(T * T, dtype=np.uint64)[None, :], thresh)
    return torch.from_numpy(keep.reshape(items, H, T, T))


def call_masks(state, st, cfg, N, T, p_h, p_a):
    """every mask of one call of N items of T tokens under ``state`` (the value of the device state when the call's launches read
    it) -> namespace(emb (N, T, d), rel[i] (2S, d), probs[i] (N, H, T, T), out[i], mlp[i] (N, T, d), c_h, c_a); a probability
    whose threshold is 0 gives None masks and c = 1"""
    d, H, S2 = cfg.hidden_size, cfg.num_attention_heads, 2 * cfg.position_buckets
    th, ta = attn_ref.mmf_drop_thresh(p_h), attn_ref.mmf_drop_thresh(p_a)
    hid = (lambda site: hidden_keep(state, site, 0, N, T * d, th).reshape(N, T, d)) if th else (lambda site: None)
    return types.SimpleNamespace(
        emb=hid(st.emb), out=[hid(s) for s in st.out], mlp=[hid(s) for s in st.mlp],
        rel=[hidden_keep(state, s, 0, 1, S2 * d, th).reshape(S2, d) if th else None for s in st.rel],
        probs=[probs_keep(state, s, 0, N, H, T, ta) if ta else None for s in st.probs],
        c_h=attn_ref.inv_keep_of(th), c_a=attn_ref.inv_keep_of(ta))


def ones_masks(cfg, N, T):
    d, H, S2, L = cfg.hidden_size, cfg.num_attention_heads, 2 * cfg.position_buckets, cfg.num_hidden_layers
    one = lambda *shape: torch.ones(shape, dtype=torch.bool)
    return types.SimpleNamespace(emb=one(N, T, d), out=[one(N, T, d) for _ in range(L)], mlp=[one(N, T, d) for _ in range(L)],
                                 rel=[one(S2, d) for _ in range(L)], probs=[one(N, H, T, T) for _ in range(L)], c_h=1.0, c_a=1.0)


def _drop(t, keep, c):
    return t if keep is None else t * (keep.to(t.device).to(t.dtype) * c)


def disentangled_attention(q, k, v, posq, posk, idx, mask, scale, keep=None, c=1.0):
    """``deberta_ref.disentangled_attention`` with the probabilities dropped in front of the product with v"""
    s, _ = G.scores(q, k, posq, posk, idx, scale)
    if mask is not None:
        m = mask.to(q.device) != 0
        s = s.masked_fill(~(m[:, :, None] & m[:, None, :])[:, None], torch.finfo(s.dtype).min)
    return _drop(torch.softmax(s, dim=-1), keep, c) @ v


def deberta_forward(sd, ids_or_embeds, mask, cfg, masks, bf16_storage: bool = False, dtype=torch.float64):
    """``deberta_ref.deberta_forward`` in training mode under ``masks`` (``call_masks`` / ``ones_masks``)"""
    on, dev = bf16_storage, ids_or_embeds.device
    W = lambda key: _r(sd[key].to(dev, dtype), on, dtype)
    F = lambda key: sd[key].to(dev, dtype)
    d, H, eps, S = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.position_buckets
    dh, c_h = d // H, masks.c_h
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
    if masks.emb is not None:
        x = _r(_drop(x, masks.emb, c_h), on, dtype)
    rel = _r(layer_norm(F("encoder.rel_embeddings.weight"), F("encoder.LayerNorm.weight"), F("encoder.LayerNorm.bias"), eps), on, dtype)
    idx = deberta_ref.bucket_index(T, S, cfg.max_position_embeddings)
    heads = lambda t: t.reshape(N, T, H, dh).transpose(1, 2)
    pos_heads = lambda t: t.reshape(2 * S, H, dh).transpose(0, 1)

    def join(dense, keep, resid):                       # dense + bias as stored, dropped, + residual, stored
        if keep is None:
            return _r(dense + resid, on, dtype)
        return _r(_drop(_r(dense, on, dtype), keep, c_h) + resid, on, dtype)
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layer.{i}."
        s = a + "attention.self."
        lin = lambda t, name: t @ W(name + ".weight").T + F(name + ".bias")
        q, k, v = (_r(lin(x, s + n), on, dtype) for n in ("query_proj", "key_proj", "value_proj"))
        rel_i = rel if masks.rel[i] is None else _r(_drop(rel, masks.rel[i], c_h), on, dtype)
        posq, posk = _r(lin(rel_i, s + "query_proj"), on, dtype), _r(lin(rel_i, s + "key_proj"), on, dtype)
        ctx = disentangled_attention(heads(q), heads(k), heads(v), pos_heads(posq), pos_heads(posk), idx, m, math.sqrt(3.0 * dh),
                                     masks.probs[i], masks.c_a)
        ctx = _r(ctx.transpose(1, 2).reshape(N, T, d), on, dtype)
        y = join(lin(ctx, a + "attention.output.dense"), masks.out[i], x)
        y = _r(layer_norm(y, F(a + "attention.output.LayerNorm.weight"), F(a + "attention.output.LayerNorm.bias"), eps), on, dtype)
        f1 = _r(y @ W(a + "intermediate.dense.weight").T, on, dtype)
        g = _r(gelu_erf(f1 + F(a + "intermediate.dense.bias")), on, dtype)
        z = join(lin(g, a + "output.dense"), masks.mlp[i], y)
        x = _r(layer_norm(z, F(a + "output.LayerNorm.weight"), F(a + "output.LayerNorm.bias"), eps), on, dtype)
    return x


# ---- the attention with dropped probabilities: forward statistics and the closed-form backward -------------------------------
def attention_stats(q, k, v, posq, posk, idx, mask, scale, w):
    """-> (O (n, H, T, dh) = (w * softmax(s)) v, lse (n, H, T) of the UNDROPPED masked scores); ``w`` (n, H, T, T) = keep * c"""
    s, _ = G.scores(q, k, posq, posk, idx, scale)
    if mask is not None:
        m = mask != 0
        s = s.masked_fill(~(m[:, :, None] & m[:, None, :])[:, None], torch.finfo(s.dtype).min)
    return (torch.softmax(s, dim=-1) * w) @ v, torch.logsumexp(s, dim=-1)


def attention_backward(q, k, v, posq, posk, idx, mask, scale, dO, w, O, lse, f32_tol):
    """``deberta_grad_ref.attention_backward`` / ``deberta_wgrad_ref.table_gradients`` with dropped probabilities, w = keep * c:
        dP_ij = w_ij dO_i.V_j,  dS_ij = P_ij (dP_ij - delta_i) / scale on unmasked pairs,  dV_j = sum_i w_ij P_ij dO_i
    and dQ, dK, dposQ, dposK from that dS as without dropout.  ``O`` / ``lse``: what the kernel is handed (delta from O, P =
    exp(s - lse)).  -> (dq, dk, dv, dposq, dposk), (noise of each: the f32 summation noise of dP - delta, ``f32_tol`` per sum)"""
    n, H, T, dh = q.shape
    R = posq.shape[1]
    s, ix = G.scores(q, k, posq, posk, idx, scale)
    m = torch.ones(n, T, dtype=torch.bool) if mask is None else mask != 0
    keep = (m[:, :, None] & m[:, None, :])[:, None].expand(n, H, T, T)
    q_on = m[:, None, :, None].expand(n, H, T, T)
    zero = torch.zeros((), dtype=s.dtype)
    lse_safe = torch.where(m[:, None, :], lse, zero)
    P = torch.where(keep, torch.exp(s - lse_safe[..., None]), zero)
    P = torch.where(q_on, P, torch.full((), 1.0 / T, dtype=s.dtype))
    delta = (dO * O).sum(-1, keepdim=True)
    dS = torch.where(keep, P * ((dO @ v.transpose(-1, -2)) * w - delta), zero) / scale
    dv = (P * w).transpose(-1, -2) @ dO

    def sums(t):
        a = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.expand(n, H, T, T), t)
        b = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.t().expand(n, H, T, T), t.transpose(-1, -2))
        return a, b
    A, B = sums(dS)
    dq, dk = dS @ k + A @ posk, dS.transpose(-1, -2) @ q + B @ posq
    dposk, dposq = torch.einsum("nhir,nhid->hrd", A, q), torch.einsum("nhjr,nhjd->hrd", B, k)
    nS = torch.where(keep, P * ((dO.abs() @ v.abs().transpose(-1, -2)) * w + (dO * O).abs().sum(-1, keepdim=True)), zero) * (f32_tol / scale)
    nA, nB = sums(nS)
    noise = (nS @ k.abs() + nA @ posk.abs(), nS.transpose(-1, -2) @ q.abs() + nB @ posq.abs(), torch.zeros_like(dv),
             torch.einsum("nhjr,nhjd->hrd", nB, k.abs()), torch.einsum("nhir,nhid->hrd", nA, q.abs()))
    return (dq, dk, dv, dposq, dposk), noise
