"""The Wav2Vec2 forward in training mode (HuggingFace ``Wav2Vec2Model`` in ``train()``): tests/w2v_ref.py's ``w2v_forward`` with every
regulariser's mask as an explicit input, and the host restatement of what each site of the HIP path draws.  It imports neither
transformers nor the code under test.

The sites, in ``Wav2Vec2Model``'s call order (``sites``: 3 + 4 per layer, numbered from ``first``):

    fp         x0   = dropout(projection(LayerNorm(features)))
    spans      x0[rows inside a span] = masked_spec_embed               (SpecAugment along time; dropout does not touch these rows)
    enc        h    = dropout(LayerNorm(x0 + gelu(pos_conv(x0))))
    probs[i]   ctx  = dropout(softmax(s)) v
    out[i]     y    = LayerNorm(dropout(ctx Wo + bo) + h)
    act[i]     g    = dropout(gelu(y W1 + b1))
    mlp[i]     h    = LayerNorm(dropout(g W2 + b2) + y)

and ``skip[i]`` (LayerDrop) makes layer i the identity; it still owns its four sites.  A mask is a bool tensor (True = kept) and kept
values are multiplied by ``c`` = 1 / (1 - p) as the kernels form it in f32 (``attn_ref.inv_keep_of``).  ``bf16_storage`` adds these
rounding points to ``w2v_ref``'s: the dropped projection is rounded once (a masked row is bf16(masked_spec_embed)); dense + bias is
rounded before its dropout and dropout + residual once, as in tests/deberta_dropout_ref.py; the dropped GELU output is rounded once;
the dropped encoder LayerNorm output once more; probabilities are never stored.

Keying (csrc/wav2vec2.hip, csrc/vit.hip, csrc/attention2.hip, csrc/elementwise.hip).  Every mask is ``mmf_keep(mmf_rng_key(state, site, sub), index, thresh)``:
  hidden-type sites   sub = the clip's index in the whole batch, index = t * width + column, width d (I at act[i])
  probs[i]            sub = clip * H + head, index = i * T + j
and the span draw of clip c uses draws n = 0, 1, .. of ``mmf_mix32(key + n * 0x9E3779B9)``, key = mmf_rng_key(state, site, c): draw 0
decides the count, the following ones the starts (``span_starts`` has the rule)."""
import math
import types

import numpy as np
import torch

import attn_ref
import w2v_ref
from backbone_ref import _r, gelu_erf, layer_norm
from deberta_dropout_ref import hidden_keep, probs_keep  # noqa: F401  (the same keying)

MASK_TRIES = 64
SETTINGS_960H = dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, layerdrop=0.1,
                     mask_time_prob=0.05, mask_time_length=10, mask_time_min_masks=2)


def sites(layers: int, first: int = 1):
    s = iter(range(first, first + 3 + 4 * layers))
    ns = types.SimpleNamespace(fp=next(s), spans=next(s), enc=next(s), probs=[], out=[], act=[], mlp=[])
    for _ in range(layers):
        ns.probs.append(next(s)), ns.out.append(next(s)), ns.act.append(next(s)), ns.mlp.append(next(s))
    return ns


# ---- the span draw ---------------------------------------------------------------------------------------------------------
def span_count(num, T, length, min_masks):
    """HuggingFace's ``compute_num_masked_span`` + the two caps of ``_compute_mask_indices`` for a drawn count"""
    num = max(num, min_masks)
    if num * length > T:
        num = T // length
    return max(min(num, T - (length - 1)), 0)


def span_starts(state, site, clip, T, prob, length, min_masks):
    """the starts of clip ``clip`` (its index in the whole batch), in draw order.  count = int(e + u) with e = prob T / length and
    u = draw 0 / 2^32, in integers: floor(e) + (draw 0 >= ceil((1 - frac(e)) 2^32)), then ``span_count``.  Each start is
    (draw * (T - length + 1)) >> 32; one that is taken already is drawn again, ``MASK_TRIES`` draws at most per start, after which the
    start is the next free value above the last draw, cyclically"""
    key = int(attn_ref.mmf_rng_key(state, site, np.uint64(clip)))
    n = [0]

    def draw():
        v = int(attn_ref.mmf_mix32(np.uint64((key + n[0] * 0x9E3779B9) & 0xFFFFFFFF)))
        n[0] += 1
        return v
    e = prob * T / length
    n0 = int(e)
    up = math.ceil((1.0 - (e - n0)) * 4294967296.0)
    num = span_count(min(n0, T) + (1 if draw() >= up else 0), T, length, min_masks)
    rng, starts = T - length + 1, []
    for _ in range(num):
        cand, free = 0, False
        for _ in range(MASK_TRIES):
            cand = (draw() * rng) >> 32
            free = cand not in starts
            if free:
                break
        while not free:
            cand = 0 if cand + 1 == rng else cand + 1
            free = cand not in starts
        starts.append(cand)
    return starts


def span_table(state, site, item0, items, T, prob, length, min_masks, slots):
    """(items, slots) int32 as ``mmf_w2v_mask_spans`` writes it: -1 in the unused slots"""
    out = -torch.ones(items, slots, dtype=torch.int32)
    for g in range(items):
        s = span_starts(state, site, item0 + g, T, prob, length, min_masks)
        out[g, :len(s)] = torch.tensor(s, dtype=torch.int32)
    return out


def rows_of(table, T, length):
    """(items, T) bool: the frames inside a span of the table"""
    m = torch.zeros(table.shape[0], T, dtype=torch.bool)
    for g in range(table.shape[0]):
        for s in table[g].tolist():
            if s >= 0:
                m[g, s:s + length] = True
    return m


# ---- every mask of a call ---------------------------------------------------------------------------------------------------
def call_masks(state, st, cfg, N, T, settings):
    """every mask of one call of N clips of T frames under ``state`` (the device state's value when the launches read it) and
    ``settings`` (HuggingFace's names) -> namespace(fp, enc, out[i], mlp[i] (N, T, d); act[i] (N, T, I); probs[i] (N, H, T, T); spans
    (N, T) bool, True inside a span; c_h, c_a, c_act, c_fp); a probability whose threshold is 0 gives None masks and c = 1"""
    d, H, I, L = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.num_hidden_layers
    t = {k: attn_ref.mmf_drop_thresh(settings.get(k, 0.0)) for k in ("hidden_dropout", "attention_dropout", "activation_dropout", "feat_proj_dropout")}
    th, ta, tg, tf = t["hidden_dropout"], t["attention_dropout"], t["activation_dropout"], t["feat_proj_dropout"]
    hid = lambda site, thr, w: hidden_keep(state, site, 0, N, T * w, thr).reshape(N, T, w) if thr else None
    spans = None
    if settings.get("mask_time_prob", 0.0) > 0.0:
        length, mn = settings.get("mask_time_length", 10), settings.get("mask_time_min_masks", 2)
        slots = max(1, span_count(int(settings["mask_time_prob"] * T / length) + 1, T, length, mn))
        spans = rows_of(span_table(state, st.spans, 0, N, T, settings["mask_time_prob"], length, mn, slots), T, length)
    return types.SimpleNamespace(
        fp=hid(st.fp, tf, d), spans=spans, enc=hid(st.enc, th, d), out=[hid(s, th, d) for s in st.out], mlp=[hid(s, th, d) for s in st.mlp],
        act=[hid(s, tg, I) for s in st.act], probs=[probs_keep(state, s, 0, N, H, T, ta) if ta else None for s in st.probs],
        c_h=attn_ref.inv_keep_of(th), c_a=attn_ref.inv_keep_of(ta), c_act=attn_ref.inv_keep_of(tg), c_fp=attn_ref.inv_keep_of(tf))


def ones_masks(cfg, N, T):
    d, H, I, L = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.num_hidden_layers
    one = lambda *shape: torch.ones(shape, dtype=torch.bool)
    return types.SimpleNamespace(fp=one(N, T, d), spans=torch.zeros(N, T, dtype=torch.bool), enc=one(N, T, d), out=[one(N, T, d) for _ in range(L)],
                                 mlp=[one(N, T, d) for _ in range(L)], act=[one(N, T, I) for _ in range(L)],
                                 probs=[one(N, H, T, T) for _ in range(L)], c_h=1.0, c_a=1.0, c_act=1.0, c_fp=1.0)


def _drop(t, keep, c):
    return t if keep is None else t * (keep.to(t.device).to(t.dtype) * c)


def w2v_forward(sd, x, cfg, masks, skip=None, dtype=torch.float64, bf16_storage: bool = False):
    """``w2v_ref.w2v_forward`` in training mode under ``masks`` (``call_masks`` / ``ones_masks``) and LayerDrop's ``skip`` (a bool per
    layer; None: no layer skipped) -> last_hidden_state (N, T, d)"""
    on, dev = bf16_storage, x.device
    W = lambda k: _r(sd[k].to(dev, dtype), on, dtype)
    F = lambda k: sd[k].to(dev, dtype)
    d, H, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    dh, ks, ss = d // H, cfg.conv_kernel, cfg.conv_stride
    fe = "feature_extractor.conv_layers."
    N = x.shape[0]
    h = w2v_ref.conv0_raw(x.to(dtype), F(fe + "0.conv.weight"), ss[0])
    mean, var = w2v_ref.conv0_stats(h)
    h = (h - mean) / torch.sqrt(var + w2v_ref.GN_EPS) * F(fe + "0.layer_norm.weight") + F(fe + "0.layer_norm.bias")
    h = _r(gelu_erf(h), on, dtype)
    for i in range(1, len(ks)):
        w = W(f"{fe}{i}.conv.weight")
        raw = _r(w2v_ref.window(h, ks[i], ss[i]) @ w.permute(0, 2, 1).reshape(w.shape[0], -1).T, on, dtype)
        h = _r(gelu_erf(raw), on, dtype)
    h = _r(layer_norm(h, F("feature_projection.layer_norm.weight"), F("feature_projection.layer_norm.bias"), eps), on, dtype)
    h = _r(h @ W("feature_projection.projection.weight").T + F("feature_projection.projection.bias"), on, dtype)
    if masks.fp is not None:
        h = _r(_drop(h, masks.fp, masks.c_fp), on, dtype)                          # the dropped projection, rounded once
    if masks.spans is not None:
        h = torch.where(masks.spans.to(dev)[..., None], _r(F("masked_spec_embed"), on, dtype), h)
    pw = _r(w2v_ref.pos_weight(sd, dtype, dev), on, dtype)
    h = _r(h + gelu_erf(w2v_ref.pos_conv(h, pw, F(w2v_ref.WN + "bias"), cfg.num_conv_pos_embedding_groups)), on, dtype)
    h = _r(layer_norm(h, F("encoder.layer_norm.weight"), F("encoder.layer_norm.bias"), eps), on, dtype)
    if masks.enc is not None:
        h = _r(_drop(h, masks.enc, masks.c_h), on, dtype)

    def join(dense, keep, resid):                       # dense + bias as stored, dropped, + residual, stored
        if keep is None:
            return _r(dense + resid, on, dtype)
        return _r(_drop(_r(dense, on, dtype), keep, masks.c_h) + resid, on, dtype)
    for i in range(cfg.num_hidden_layers):
        if skip is not None and skip[i]:
            continue
        a = f"encoder.layers.{i}."
        q = _r(h @ W(a + "attention.q_proj.weight").T + F(a + "attention.q_proj.bias"), on, dtype)
        k = _r(h @ W(a + "attention.k_proj.weight").T + F(a + "attention.k_proj.bias"), on, dtype)
        v = _r(h @ W(a + "attention.v_proj.weight").T + F(a + "attention.v_proj.bias"), on, dtype)
        q, k, v = (t.reshape(N, -1, H, dh).transpose(1, 2) for t in (q, k, v))
        att = _drop(torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh), dim=-1), masks.probs[i], masks.c_a) @ v
        att = _r(att.transpose(1, 2).reshape(N, -1, d), on, dtype)
        y = join(att @ W(a + "attention.out_proj.weight").T + F(a + "attention.out_proj.bias"), masks.out[i], h)
        ln = _r(layer_norm(y, F(a + "layer_norm.weight"), F(a + "layer_norm.bias"), eps), on, dtype)
        f1 = _r(ln @ W(a + "feed_forward.intermediate_dense.weight").T, on, dtype)
        g = _r(_drop(gelu_erf(f1 + F(a + "feed_forward.intermediate_dense.bias")), masks.act[i], masks.c_act), on, dtype)   # one rounding
        y = join(g @ W(a + "feed_forward.output_dense.weight").T + F(a + "feed_forward.output_dense.bias"), masks.mlp[i], ln)
        h = _r(layer_norm(y, F(a + "final_layer_norm.weight"), F(a + "final_layer_norm.bias"), eps), on, dtype)
    return h
