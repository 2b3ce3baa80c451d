"""The WavLM forward (HuggingFace ``WavLMModel`` up to ``last_hidden_state``, wavlm-base family, no mask) restated as explicit
tensor math on tests/w2v_ref.py's front end: the same feature extractor, projection, positional convolution and post-LN layers, with
the gated relative position bias in every layer's attention,

    score[b, h, i, j] = q_i . k_j / sqrt(dh) + g[b, h, i] * rel_attn_embed[bucket(j - i)][h]

``g`` from the layer's INPUT (not q) through the 8-output linear all heads share.  It imports neither transformers nor the code
under test.  ``bf16_storage`` rounds where the HIP path stores bf16 (tests/w2v_ref.py); the gate and the bias table stay f32 there, so
they are not rounded here.  ``mutant`` names one deliberate mistake (``MUTANTS``); the CPU test shows each leaves the bound the true
restatement meets.  The staged restatements of the two kernels (``gate_ref``, ``relbias_attention_ref``) are what the GPU kernel tests
compare against.
"""
import math
import types

import torch

import w2v_ref
from backbone_ref import _r, config_kwargs, gelu_erf, layer_norm  # noqa: F401

MUTANTS = ("gate_one", "bias_i_minus_j", "gate_neighbour_head", "gate_from_q", "table_shift")


def tiny_config():
    return types.SimpleNamespace(**vars(w2v_ref.tiny_config()), num_buckets=320, max_bucket_distance=800)


def base_config():
    return types.SimpleNamespace(**vars(w2v_ref.base_config()), num_buckets=320, max_bucket_distance=800)


def hf_keys(cfg, legacy_weight_norm: bool = False):
    """the ``WavLMModel`` state_dict: key -> shape, in HuggingFace's order (a module's own parameters come ahead of its children's)"""
    H, dh = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads
    out = {}
    for k, shape in w2v_ref.hf_keys(cfg, legacy_weight_norm).items():
        if k.endswith(".attention.k_proj.weight"):
            out[k[:-len("k_proj.weight")] + "gru_rel_pos_const"] = (1, H, 1, 1)
        out[k] = shape
        if k.endswith(".attention.out_proj.bias"):
            a = k[:-len("out_proj.bias")]
            out[a + "gru_rel_pos_linear.weight"], out[a + "gru_rel_pos_linear.bias"] = (8, dh), (8,)
            if a.startswith("encoder.layers.0."):
                out[a + "rel_attn_embed.weight"] = (cfg.num_buckets, H)
    return out


def seeded_weights(cfg, seed: int = 0, legacy_weight_norm: bool = False):
    """tests/w2v_ref.py's weights, and the three new kinds away from their initial values (ones, a small linear, N(0, 1) embeddings)
    so that the gate spreads over most of its range (0.5 .. 3) and differs between heads and rows"""
    sd = w2v_ref.seeded_weights(cfg, seed, legacy_weight_norm)
    g = torch.Generator().manual_seed(seed + 7919)
    out = {}
    for k, shape in hf_keys(cfg, legacy_weight_norm).items():
        if k in sd:
            out[k] = sd[k]
        elif k.endswith("gru_rel_pos_const"):
            out[k] = 1.0 + 0.8 * torch.randn(shape, generator=g)
        elif k.endswith("gru_rel_pos_linear.weight"):
            out[k] = 0.5 * torch.randn(shape, generator=g)
        elif k.endswith("gru_rel_pos_linear.bias"):
            out[k] = 0.5 * torch.randn(shape, generator=g)
        else:
            out[k] = 1.5 * torch.randn(shape, generator=g)
    return out


def relative_buckets(rel, num_buckets: int, max_distance: int):
    """the bucket of each signed distance ``rel`` = key - query (int64): half the buckets per sign, half of those exact, the rest
    log-spaced up to ``max_distance``.  The float32 expression, in HuggingFace's operation order: boundaries depend on it"""
    nb = num_buckets // 2
    max_exact = nb // 2
    a = rel.abs()
    f = torch.log(a.to(torch.float32) / max_exact)
    f = f / math.log(max_distance / max_exact)
    f = f * (nb - max_exact)
    large = torch.clamp((max_exact + f).to(torch.int64), max=nb - 1)
    return (rel > 0).to(torch.int64) * nb + torch.where(a < max_exact, a, large)


def bias_table(embed, T: int, num_buckets: int, max_distance: int):
    """(H, 2T - 1): ``table[h][j - i + T - 1]``, embed (num_buckets, H)"""
    return embed[relative_buckets(torch.arange(-(T - 1), T), num_buckets, max_distance).to(embed.device)].T


def gate_ref(x, w, b, const):
    """x (n, T, H, dh), w (8, dh), b (8), const (H) -> g (n, H, T)"""
    y = x @ w.T + b                                                            # (n, T, H, 8)
    sa, sb = torch.sigmoid(y[..., :4].sum(-1)), torch.sigmoid(y[..., 4:].sum(-1))
    return (sa * (sb * const - 1.0) + 2.0).transpose(1, 2)


def relbias_attention_ref(q, k, v, gate, table, scale):
    """q, k, v (B, H, T, dh), gate (B, H, T), table (H, 2T - 1), every offset its own entry -> (O (B, H, T, dh), LSE (B, H, T),
    the scores)"""
    T = q.shape[2]
    idx = torch.arange(T).view(1, T) - torch.arange(T).view(T, 1) + T - 1      # [i][j] = j - i + T - 1
    s = (q @ k.transpose(-1, -2)) * scale + gate.unsqueeze(-1) * table[:, idx.to(table.device)]
    lse = torch.logsumexp(s, dim=-1)
    return torch.softmax(s, dim=-1) @ v, lse, s


def relbias_staged(q, k, v, H, scale, gate, table, perturb=0.0, seed=0):
    """The forward of tests/attn_ref.py's ``staged()`` with the bias: operands (B, T, H*dh) float64 holding bf16 values, gate
    (B, H, T) and table (H, 2T - 1) float64 holding f32 values, ``scale`` the f32 value the kernel is handed.  The kernel's rounding
    points and only those: the bias joins the RAW scores as (gate / scale) * table (the plain kernel's softmax follows unchanged),
    P relative to the deferred running maximum of 32-key blocks is rounded to bf16 before P.V, the row sum takes the unrounded P.
    ``perturb`` as in ``staged()``, on the biased raw scores.  -> dict(o (B, T, H*dh), lse (B, H, T))"""
    import attn_ref as R
    qh, kh, vh = R.heads(q, H), R.heads(k, H), R.heads(v, H)
    B, _, T, dh = qh.shape
    idx = torch.arange(T).view(1, T) - torch.arange(T).view(T, 1) + T - 1
    s = qh @ kh.transpose(-1, -2) + (gate / scale).unsqueeze(-1) * table[:, idx]
    if perturb:
        g = torch.Generator().manual_seed(seed)
        s = s * (1.0 + perturb * (2.0 * torch.rand(s.shape, generator=g, dtype=torch.float64) - 1.0))
    c = scale * R.LOG2E
    m = torch.full((B, H, T), R.NEG_BIG, dtype=torch.float64)
    l = torch.zeros((B, H, T), dtype=torch.float64)
    o = torch.zeros((B, H, T, dh), dtype=torch.float64)
    qblk = torch.arange(T) // 32
    for k0 in range(0, T, 32):
        sb = s[..., k0:k0 + 32]
        mx = sb.max(-1).values * c
        over = mx > m + R.DEFER
        raise_blk = torch.nn.functional.pad(over, (0, -T % 32)).reshape(B, H, -1, 32).any(-1)
        mnew = torch.where(raise_blk[..., qblk], torch.maximum(m, mx), m)
        alpha = torch.exp2(m - mnew)
        m, l, o = mnew, l * alpha, o * alpha[..., None]
        p = torch.exp2(sb * c - m[..., None])
        l = l + p.sum(-1)
        o = o + R.bf16r(p) @ vh[:, :, k0:k0 + 32]
    return dict(o=R.merge(o / l[..., None]), lse=m * R.LN2 + torch.log(l))


def wavlm_forward(sd, x, cfg, dtype=torch.float64, bf16_storage: bool = False, mutant=None):
    """-> last_hidden_state (N, T, d) in ``dtype``"""
    assert mutant is None or mutant in MUTANTS, mutant
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
    pw = _r(w2v_ref.pos_weight(sd, dtype, dev), on, dtype)
    h = _r(h + gelu_erf(w2v_ref.pos_conv(h, pw, F(w2v_ref.WN + "bias"), cfg.num_conv_pos_embedding_groups)), on, dtype)
    h = _r(layer_norm(h, F("encoder.layer_norm.weight"), F("encoder.layer_norm.bias"), eps), on, dtype)
    T = h.shape[1]
    table = bias_table(F("encoder.layers.0.attention.rel_attn_embed.weight"), T, cfg.num_buckets, cfg.max_bucket_distance)
    if mutant == "bias_i_minus_j":
        table = table.flip(1)
    if mutant == "table_shift":
        table = table.roll(1, dims=1)
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layers.{i}."
        q = _r(h @ W(a + "attention.q_proj.weight").T + F(a + "attention.q_proj.bias"), on, dtype)
        k = _r(h @ W(a + "attention.k_proj.weight").T + F(a + "attention.k_proj.bias"), on, dtype)
        v = _r(h @ W(a + "attention.v_proj.weight").T + F(a + "attention.v_proj.bias"), on, dtype)
        src = q if mutant == "gate_from_q" else h
        gate = gate_ref(src.reshape(N, T, H, dh), F(a + "attention.gru_rel_pos_linear.weight"), F(a + "attention.gru_rel_pos_linear.bias"),
                        F(a + "attention.gru_rel_pos_const").reshape(H))
        if mutant == "gate_one":
            gate = torch.ones_like(gate)
        if mutant == "gate_neighbour_head":
            gate = gate.roll(1, dims=1)
        q, k, v = (t.reshape(N, T, H, dh).transpose(1, 2) for t in (q, k, v))
        att = relbias_attention_ref(q, k, v, gate, table, 1.0 / math.sqrt(dh))[0]
        att = _r(att.transpose(1, 2).reshape(N, T, d), on, dtype)
        y = _r(att @ W(a + "attention.out_proj.weight").T + F(a + "attention.out_proj.bias") + h, on, dtype)
        ln = _r(layer_norm(y, F(a + "layer_norm.weight"), F(a + "layer_norm.bias"), eps), on, dtype)
        f1 = _r(ln @ W(a + "feed_forward.intermediate_dense.weight").T, on, dtype)
        g = _r(gelu_erf(f1 + F(a + "feed_forward.intermediate_dense.bias")), on, dtype)
        y = _r(g @ W(a + "feed_forward.output_dense.weight").T + F(a + "feed_forward.output_dense.bias") + ln, on, dtype)
        h = _r(layer_norm(y, F(a + "final_layer_norm.weight"), F(a + "final_layer_norm.bias"), eps), on, dtype)
    return h


def load_golden(path):
    """tests/golden/wavlm_tiny.npz (tools/capture_wavlm_golden.py) -> (state_dict, input_values, last_hidden_state)"""
    import numpy as np
    z = np.load(path)
    sd = {}
    for name in z.files:
        kind, _, key = name.partition(":")
        if kind == "q":
            sd[key] = torch.from_numpy(z[name]).float() * float(z["s:" + key])
        elif kind == "f":
            sd[key] = torch.from_numpy(z[name])
    return sd, torch.from_numpy(z["input_values_q64"]).float() / 64.0, torch.from_numpy(z["last_hidden_state"])   # (int8 sixty-fourths)


class RefWavLM(torch.nn.Module):
    """``wavlm_forward`` behind the ``backbone=`` protocol of the encoders"""

    def __init__(self, sd, cfg, dtype=torch.float32):
        super().__init__()
        self.config, self.sd, self.dtype = cfg, sd, dtype

    def forward(self, input_values, attention_mask=None):
        with torch.no_grad():
            out = wavlm_forward(self.sd, input_values, self.config, dtype=self.dtype).float()
        return types.SimpleNamespace(last_hidden_state=out)
