"""The BERT / RoBERTa forward (HuggingFace ``BertModel`` / ``RobertaModel`` up to ``last_hidden_state``, eager attention, absolute
positions) restated as explicit tensor math.  It imports neither transformers nor the code under test.

    x = LayerNorm(word[ids] + type[token types] + pos[p])          p: BERT the token's place; RoBERTa from the ids (``position_ids``)
    per layer (post-LN): a = softmax(q k^T / sqrt(dh) over the VALID keys) v;  x = LN(x + o(a));  x = LN(x + fc2(gelu(fc1(x))))

Only keys are masked: every query row is computed.  An item without a valid key attends uniformly over all its keys (what
``score + finfo.min`` gives in float32).  ``bf16_storage`` rounds where the HIP path stores bf16 (the embedding row, the GEMM outputs
and weights, the attention output, the LayerNorm outputs).  ``mutant`` names one deliberate mistake (``MUTANTS``); the CPU test shows
each leaves the bound the true restatement meets.  ``keymask_staged`` (tests/attn_ref.py's staged forward with the key mask),
``position_ids``, ``embed_ref`` and ``pack_ref`` are what the GPU kernel tests compare against.
"""
import math
import types

import torch

from backbone_ref import _r, config_kwargs, gelu_erf, layer_norm  # noqa: F401

MUTANTS = ("mask_ignored", "mask_on_queries", "positions_from_mask", "position_offset_missing", "token_type_dropped", "pre_ln",
           "empty_item_plain_softmax")
# what a mutant needs in order to show: a model family, or an item without a valid key
ROBERTA_ONLY = ("positions_from_mask", "position_offset_missing")
NEEDS_EMPTY_ITEM = ("empty_item_plain_softmax",)


def tiny_config(family: str = "bert", **over):
    base = dict(vocab_size=64, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512)
    if family == "bert":
        base.update(max_position_embeddings=40, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0)
    else:
        base.update(max_position_embeddings=42, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1)
    return types.SimpleNamespace(**{**base, **over})


def base_config(family: str = "bert"):
    base = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    if family == "bert":
        base.update(vocab_size=30522, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0)
    else:
        base.update(vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1)
    return types.SimpleNamespace(**base)


def hf_config_kwargs(cfg):
    """the keyword arguments of HuggingFace's ``BertConfig`` / ``RobertaConfig`` for this restatement"""
    return dict(vars(cfg), hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                position_embedding_type="absolute", attn_implementation="eager")


def hf_keys(cfg, family: str = "bert", pooler: bool = True):
    """the ``BertModel`` / ``RobertaModel`` state_dict: key -> shape, in HuggingFace's order (RoBERTa's embeddings register their
    position table last)"""
    d, I, e = cfg.hidden_size, cfg.intermediate_size, "embeddings."
    emb = {"word_embeddings.weight": (cfg.vocab_size, d), "position_embeddings.weight": (cfg.max_position_embeddings, d),
           "token_type_embeddings.weight": (cfg.type_vocab_size, d), "LayerNorm.weight": (d,), "LayerNorm.bias": (d,)}
    order = list(emb) if family == "bert" else ["word_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight",
                                                "LayerNorm.bias", "position_embeddings.weight"]
    out = {e + k: emb[k] for k in order}
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            out[f"{a}attention.self.{n}.weight"], out[f"{a}attention.self.{n}.bias"] = (d, d), (d,)
        out[a + "attention.output.dense.weight"], out[a + "attention.output.dense.bias"] = (d, d), (d,)
        out[a + "attention.output.LayerNorm.weight"], out[a + "attention.output.LayerNorm.bias"] = (d,), (d,)
        out[a + "intermediate.dense.weight"], out[a + "intermediate.dense.bias"] = (I, d), (I,)
        out[a + "output.dense.weight"], out[a + "output.dense.bias"] = (d, I), (d,)
        out[a + "output.LayerNorm.weight"], out[a + "output.LayerNorm.bias"] = (d,), (d,)
    if pooler:
        out["pooler.dense.weight"], out["pooler.dense.bias"] = (d, d), (d,)
    return out


def seeded_weights(cfg, family: str = "bert", seed: int = 0):
    """Weights with spread enough that the forward exercises everything: 1/sqrt(fan_in)-scaled matrices, the q / k projections
    1.5 times that (tests/w2v_ref.py's choice) so the softmax rows are far from uniform; word, position and type embeddings of
    comparable size, so that a wrong position or a dropped type shows; non-trivial biases and norm parameters."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in hf_keys(cfg, family).items():
        t = torch.randn(shape, generator=g)
        if k.endswith("LayerNorm.weight"):
            t = 1.0 + 0.2 * t
        elif k.endswith(".bias"):
            t = 0.1 * t
        elif "embeddings" in k:
            t = t * (1.0 if "word" in k else 0.7)
        else:
            t = t * ((1.5 if ".query." in k or ".key." in k else 1.0) / math.sqrt(shape[1]))
        sd[k] = t
    return sd


# ---- the pieces the kernels are compared against -------------------------------------------------------------------------
def position_ids(ids, family: str, pad: int, mutant=None, mask=None):
    """(N, T) int64 position ids from (N, T) ids: BERT the place; RoBERTa HuggingFace's ``create_position_ids_from_input_ids``"""
    N, T = ids.shape
    place = torch.arange(T, device=ids.device).expand(N, T)
    if family == "bert":
        return place
    ne = (ids != pad).to(torch.int64)
    if mutant == "positions_from_mask":
        ne = (mask != 0).to(torch.int64) if mask is not None else torch.ones_like(ne)
    p = torch.cumsum(ne, dim=1) * ne
    return p if mutant == "position_offset_missing" else p + pad


def embeds_position_ids(N: int, T: int, family: str, pad: int, device=None):
    """the ``inputs_embeds`` route: BERT the place; RoBERTa pad + 1 + place"""
    place = torch.arange(T, device=device).expand(N, T)
    return place if family == "bert" else place + pad + 1


def clamp_ids(ids, n: int):
    return ids.clamp(0, n - 1)


def embed_ref(rows, pos_rows, type_rows, gamma, beta, eps):
    """LayerNorm((rows + type_rows) + pos_rows) in the operands' dtype: the three gathered rows, HuggingFace's order of the sum"""
    return layer_norm((rows + type_rows) + pos_rows, gamma, beta, eps)


def pack_words(T: int) -> int:
    return 2 + 2 * ((T + 63) // 64)


def pack_ref(mask, n: int, T: int):
    """``mmf_mask_pack``'s output restated on the host: (n, 2 + 2 ceil(T / 64)) int64 holding uint32 values: one past the last
    valid key, the count, then bit k of word w = key 32 w + k is valid.  ``mask`` (n, T) of any dtype (non-zero: valid) or None"""
    valid = torch.ones(n, T, dtype=torch.bool) if mask is None else (mask.reshape(n, T).cpu() != 0)
    out = torch.zeros(n, pack_words(T), dtype=torch.int64)
    for b in range(n):
        keys = valid[b].nonzero().reshape(-1).tolist()
        out[b, 0], out[b, 1] = (keys[-1] + 1 if keys else 0), len(keys)
        for k in keys:
            out[b, 2 + k // 32] |= 1 << (k % 32)
    return out


def masked_attention_ref(q, k, v, valid, scale, mutant=None):
    """q, k, v (B, H, T, dh), valid (B, T) bool -> (O (B, H, T, dh), LSE (B, H, T)): the exact softmax over the valid keys; an item
    without one takes all scores 0 (the uniform row)"""
    s = (q @ k.transpose(-1, -2)) * scale
    empty = ~valid.any(dim=1)
    keep = valid | empty[:, None]
    if mutant != "empty_item_plain_softmax":
        s = torch.where(empty[:, None, None, None], torch.zeros_like(s), s)
    s = s.masked_fill(~keep[:, None, None, :], -math.inf)
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1)


def keymask_staged(q, k, v, H, scale, valid, perturb=0.0, seed=0):
    """The forward of tests/attn_ref.py's ``staged()`` with a key mask: operands (B, T, H*dh) float64 holding bf16 values,
    ``valid`` (B, T) bool, ``scale`` the f32 value the kernel is handed.  The kernel's rounding points and only those (P relative to
    the deferred running maximum of 32-key blocks rounded to bf16 before P.V, the row sum from the unrounded P), with masked keys
    DROPPED (their K and V rows never enter: the score is -inf and 0 * v is formed with v replaced by 0), 32-key blocks without a
    valid key skipped (they raise no maximum), and the empty-item rule: all scores 0 over all T keys.  ``perturb`` as in
    ``staged()``, on the raw scores.  -> dict(o (B, T, H*dh), lse (B, H, T))"""
    import attn_ref as R
    qh, kh, vh = R.heads(q, H), R.heads(k, H), R.heads(v, H)
    B, _, T, dh = qh.shape
    empty = ~valid.any(dim=1)
    keep = valid | empty[:, None]                                              # (B, T)
    kh = torch.where(keep[:, None, :, None], kh, torch.zeros_like(kh))         # dropped: whatever the masked rows hold
    vh = torch.where(keep[:, None, :, None], vh, torch.zeros_like(vh))
    s = qh @ kh.transpose(-1, -2)
    if perturb:
        g = torch.Generator().manual_seed(seed)
        s = s * (1.0 + perturb * (2.0 * torch.rand(s.shape, generator=g, dtype=torch.float64) - 1.0))
    s = torch.where(empty[:, None, None, None], torch.zeros_like(s), s)
    s = s.masked_fill(~keep[:, None, None, :], -math.inf)
    c = scale * R.LOG2E
    m = torch.full((B, H, T), R.NEG_BIG, dtype=torch.float64)
    l = torch.zeros((B, H, T), dtype=torch.float64)
    o = torch.zeros((B, H, T, dh), dtype=torch.float64)
    qblk = torch.arange(T) // 32
    for k0 in range(0, T, 32):
        live = keep[:, k0:k0 + 32].any(dim=1)                                   # (B,): a block without a valid key is skipped
        sb = s[..., k0:k0 + 32]
        mx = sb.max(-1).values * c
        over = (mx > m + R.DEFER) & live[:, None, None]
        raise_blk = torch.nn.functional.pad(over, (0, -T % 32)).reshape(B, H, -1, 32).any(-1)
        mnew = torch.where(raise_blk[..., qblk], torch.maximum(m, mx), m)
        alpha = torch.exp2(m - mnew)
        m, l, o = mnew, l * alpha, o * alpha[..., None]
        p = torch.exp2(sb * c - m[..., None])                                  # exactly 0 at a masked key
        l = l + p.sum(-1)
        o = o + R.bf16r(p) @ vh[:, :, k0:k0 + 32]
    return dict(o=R.merge(o / l[..., None]), lse=m * R.LN2 + torch.log(l))


# ---- the model ---------------------------------------------------------------------------------------------------------------
def bert_forward(sd, x, mask, cfg, family: str = "bert", dtype=torch.float64, bf16_storage: bool = False, mutant=None,
                 token_type_ids=None):
    """``x``: (N, T) int64 ids or (N, T, d) input embeddings; ``mask`` (N, T) of any dtype or None -> last_hidden_state (N, T, d)
    in ``dtype``"""
    assert mutant is None or mutant in MUTANTS, mutant
    assert family in ("bert", "roberta"), family
    on, dev = bf16_storage, x.device
    W = lambda k: _r(sd[k].to(dev, dtype), on, dtype)
    F = lambda k: sd[k].to(dev, dtype)
    d, H, eps, pad = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.pad_token_id
    dh = d // H
    N, T = x.shape[:2]
    valid = torch.ones(N, T, dtype=torch.bool, device=dev) if mask is None else (mask.to(dev) != 0)
    if mutant == "mask_ignored":
        valid = torch.ones_like(valid)
    e = "embeddings."
    if x.dim() == 2:
        rows = F(e + "word_embeddings.weight")[clamp_ids(x, cfg.vocab_size)]
        pos = position_ids(x, family, pad, mutant, mask)
    else:
        rows = x.to(dtype)
        pos = embeds_position_ids(N, T, family, pad, dev)
        if mutant == "position_offset_missing" and family == "roberta":
            pos = pos - pad
    tt = torch.zeros(N, T, dtype=torch.int64, device=dev) if token_type_ids is None else token_type_ids.to(dev)
    type_rows = F(e + "token_type_embeddings.weight")[clamp_ids(tt, cfg.type_vocab_size)]
    if mutant == "token_type_dropped":
        type_rows = torch.zeros_like(type_rows)
    pos_rows = F(e + "position_embeddings.weight")[clamp_ids(pos, cfg.max_position_embeddings)]
    h = _r(embed_ref(rows, pos_rows, type_rows, F(e + "LayerNorm.weight"), F(e + "LayerNorm.bias"), eps), on, dtype)
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layer.{i}."
        ln1 = lambda t: layer_norm(t, F(a + "attention.output.LayerNorm.weight"), F(a + "attention.output.LayerNorm.bias"), eps)
        ln2 = lambda t: layer_norm(t, F(a + "output.LayerNorm.weight"), F(a + "output.LayerNorm.bias"), eps)
        src = _r(ln1(h), on, dtype) if mutant == "pre_ln" else h
        q = _r(src @ W(a + "attention.self.query.weight").T + F(a + "attention.self.query.bias"), on, dtype)
        k = _r(src @ W(a + "attention.self.key.weight").T + F(a + "attention.self.key.bias"), on, dtype)
        v = _r(src @ W(a + "attention.self.value.weight").T + F(a + "attention.self.value.bias"), on, dtype)
        q, k, v = (t.reshape(N, T, H, dh).transpose(1, 2) for t in (q, k, v))
        att = masked_attention_ref(q, k, v, valid, 1.0 / math.sqrt(dh), mutant)[0]
        att = att.transpose(1, 2).reshape(N, T, d)
        if mutant == "mask_on_queries":
            att = att * valid[..., None].to(dtype)
        att = _r(att, on, dtype)
        y = _r(att @ W(a + "attention.output.dense.weight").T + F(a + "attention.output.dense.bias") + h, on, dtype)
        if mutant == "pre_ln":
            src2 = _r(ln2(y), on, dtype)
            f1 = _r(src2 @ W(a + "intermediate.dense.weight").T, on, dtype)
            g = _r(gelu_erf(f1 + F(a + "intermediate.dense.bias")), on, dtype)
            h = _r(g @ W(a + "output.dense.weight").T + F(a + "output.dense.bias") + y, on, dtype)
            continue
        ln = _r(ln1(y), on, dtype)
        f1 = _r(ln @ W(a + "intermediate.dense.weight").T, on, dtype)
        g = _r(gelu_erf(f1 + F(a + "intermediate.dense.bias")), on, dtype)
        y = _r(g @ W(a + "output.dense.weight").T + F(a + "output.dense.bias") + ln, on, dtype)
        h = _r(ln2(y), on, dtype)
    return h


def load_golden(path):
    """tests/golden/{bert,roberta}_tiny.npz (tools/capture_bert_golden.py) -> (state_dict, input_ids, attention_mask,
    token_type_ids, last_hidden_state)"""
    import numpy as np
    z = np.load(path, allow_pickle=False)
    sd = {}
    for name in z.files:
        kind, _, key = name.partition(":")
        if kind == "q":
            sd[key] = torch.from_numpy(z[name]).float() * float(z["s:" + key])
        elif kind == "f":
            sd[key] = torch.from_numpy(z[name])
    i64 = lambda n: torch.from_numpy(z[n]).to(torch.int64)
    return sd, i64("input_ids"), i64("attention_mask"), i64("token_type_ids"), torch.from_numpy(z["last_hidden_state"])


class RefBert(torch.nn.Module):
    """``bert_forward`` behind the ``backbone=`` protocol of ``TextEncoder`` (``.config``, ``.embeddings.word_embeddings``,
    ``input_ids`` / ``inputs_embeds`` / ``attention_mask`` keywords)"""

    def __init__(self, sd, cfg, family: str, dtype=torch.float32, bf16_storage: bool = False):
        super().__init__()
        self.sd, self.family, self.dtype, self.bf16_storage = sd, family, dtype, bf16_storage
        self.config = types.SimpleNamespace(**vars(cfg), model_type=family)
        table = sd["embeddings.word_embeddings.weight"]
        self.embeddings = types.SimpleNamespace(word_embeddings=lambda ids: table.to(ids.device)[ids])

    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None, token_type_ids=None):
        with torch.no_grad():
            x = input_ids if input_ids is not None else inputs_embeds
            out = bert_forward(self.sd, x, attention_mask, self.config, self.family, dtype=self.dtype, bf16_storage=self.bf16_storage,
                               token_type_ids=token_type_ids).float()
        return types.SimpleNamespace(last_hidden_state=out)
