"""The Wav2Vec2 forward (HuggingFace ``Wav2Vec2Model`` up to ``last_hidden_state``, base family, no mask) restated as
explicit tensor math, written from the architecture: Conv1d(1 -> C0) + GroupNorm(one group per channel) + exact GELU ->
bias-free strided convolutions + GELU -> LayerNorm -> projection -> x + gelu(weight-normed grouped positional convolution)
-> LayerNorm -> post-LN transformer layers.  It imports neither transformers nor the code under test.

Weights are a ``state_dict`` in ``Wav2Vec2Model``'s key naming; the positional convolution's weight norm may be spelled
``parametrizations.weight.original0/1`` or ``weight_g`` / ``weight_v``.

``bf16_storage=True`` models the storage format of the HIP path, not its kernels: values are rounded to bf16 exactly where
that path writes bf16 to memory (layer 0 after its GELU, every GEMM / LayerNorm / attention output, each GELU output, the
GEMM weights, the folded positional weight, the positional kernel's output) and everything between two stores is computed in
``dtype``.

``dtype=torch.bfloat16`` on a GPU tensor, with ``sdpa=True``, is the stock-torch yardstick of tools/w2v_bench.py.
"""
import math
import types

import torch

from backbone_ref import _r, config_kwargs, gelu_erf, layer_norm  # noqa: F401  (the tests read them from here)

GN_EPS = 1e-5            # nn.GroupNorm's default, which HuggingFace's group-norm conv layer keeps


def tiny_config():
    return types.SimpleNamespace(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                 conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), conv_bias=False,
                                 num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5,
                                 feat_extract_norm="group", do_stable_layer_norm=False)


def base_config():
    return types.SimpleNamespace(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                                 conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2),
                                 conv_bias=False, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                                 layer_norm_eps=1e-5, feat_extract_norm="group", do_stable_layer_norm=False)


WN = "encoder.pos_conv_embed.conv."
WN_NEW = (WN + "parametrizations.weight.original0", WN + "parametrizations.weight.original1")
WN_OLD = (WN + "weight_g", WN + "weight_v")


def hf_keys(cfg, legacy_weight_norm: bool = False):
    """the ``Wav2Vec2Model`` state_dict: key -> shape, in HuggingFace's order"""
    d, I, dims, ks = cfg.hidden_size, cfg.intermediate_size, cfg.conv_dim, cfg.conv_kernel
    pk, cg = cfg.num_conv_pos_embeddings, cfg.hidden_size // cfg.num_conv_pos_embedding_groups
    g, v = WN_OLD if legacy_weight_norm else WN_NEW
    fe = "feature_extractor.conv_layers."
    out = {"masked_spec_embed": (d,), fe + "0.conv.weight": (dims[0], 1, ks[0]), fe + "0.layer_norm.weight": (dims[0],),
           fe + "0.layer_norm.bias": (dims[0],)}
    for i in range(1, len(dims)):
        out[f"{fe}{i}.conv.weight"] = (dims[i], dims[i - 1], ks[i])
    out["feature_projection.layer_norm.weight"], out["feature_projection.layer_norm.bias"] = (dims[-1],), (dims[-1],)
    out["feature_projection.projection.weight"], out["feature_projection.projection.bias"] = (d, dims[-1]), (d,)
    out[WN + "bias"], out[g], out[v] = (d,), (1, 1, pk), (d, cg, pk)
    out["encoder.layer_norm.weight"], out["encoder.layer_norm.bias"] = (d,), (d,)
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out[f"{a}attention.{n}.weight"], out[f"{a}attention.{n}.bias"] = (d, d), (d,)
        out[a + "layer_norm.weight"], out[a + "layer_norm.bias"] = (d,), (d,)
        out[a + "feed_forward.intermediate_dense.weight"], out[a + "feed_forward.intermediate_dense.bias"] = (I, d), (I,)
        out[a + "feed_forward.output_dense.weight"], out[a + "feed_forward.output_dense.bias"] = (d, I), (d,)
        out[a + "final_layer_norm.weight"], out[a + "final_layer_norm.bias"] = (d,), (d,)
    return out


def seeded_weights(cfg, seed: int = 0, legacy_weight_norm: bool = False):
    """Weights with spread enough that the forward exercises everything: 1/sqrt(fan_in)-scaled matrices (sqrt 2 more for the
    convolutions, whose GELU halves the variance), the q / k projections 1.5 times that so the softmax rows are far from
    uniform; non-trivial biases, norm parameters and weight-norm gains."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in hf_keys(cfg, legacy_weight_norm).items():
        t = torch.randn(shape, generator=g)
        if k.endswith("norm.weight"):
            t = 1.0 + 0.2 * t
        elif k.endswith(".bias"):
            t = 0.1 * t
        elif k in (WN_NEW[0], WN_OLD[0]):                             # the gain per tap: v / ||v|| has entries ~ 1 / sqrt(C cg), and the
            t = math.sqrt(cfg.hidden_size / shape[2]) * (1.0 + 0.3 * torch.rand(shape, generator=g))     # effective weight wants ~ 1 / sqrt(cg k)
        elif k in (WN_NEW[1], WN_OLD[1]):
            pass
        elif k == "masked_spec_embed":
            pass
        elif len(shape) == 3:
            t = t * math.sqrt(2.0 / (shape[1] * shape[2]))
        else:
            t = t / math.sqrt(shape[1]) * (1.5 if ("q_proj" in k or "k_proj" in k) else 1.0)
        sd[k] = t
    return sd


def window(x, k, s):
    """(N, T_in, C) -> (N, T_out, k * C), row t column (j, c) = x[s t + j][c]: a strided Conv1d as a matmul"""
    N, T_in, C = x.shape
    T_out = (T_in - k) // s + 1
    idx = (torch.arange(T_out, device=x.device) * s).unsqueeze(1) + torch.arange(k, device=x.device)
    return x[:, idx].reshape(N, T_out, k * C)


def conv0_raw(wave, w0, s0):
    """Conv1d(1 -> C0, k0, stride s0, no bias), channel-last: (N, L) -> (N, T0, C0)"""
    k0 = w0.shape[-1]
    return window(wave.unsqueeze(-1), k0, s0) @ w0.reshape(w0.shape[0], k0).T


def conv0_stats(raw):
    mean = raw.mean(dim=1, keepdim=True)
    return mean, ((raw - mean) ** 2).mean(dim=1, keepdim=True)


def pos_weight(sd, dtype=torch.float64, device="cpu"):
    """the effective weight g v / ||v||, norm over dims (0, 1) per tap (``weight_norm(dim=2)``)"""
    g = sd[WN_NEW[0]] if WN_NEW[0] in sd else sd[WN_OLD[0]]
    v = sd[WN_NEW[1]] if WN_NEW[1] in sd else sd[WN_OLD[1]]
    g, v = g.to(device, dtype), v.to(device, dtype)
    return g * v / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))


def pos_conv(x, w, bias, groups):
    """x (N, T, C), w (C, cg, k): grouped Conv1d with padding k // 2, the extra last frame of an even k dropped -> (N, T, C)"""
    N, T, C = x.shape
    cg, k = w.shape[1], w.shape[2]
    pad = k // 2
    xp = torch.cat([x.new_zeros(N, pad, C), x, x.new_zeros(N, k - 1 - pad, C)], dim=1)           # rows t - pad .. t - pad + k - 1
    out = []
    for g in range(groups):
        win = window(xp[:, :, g * cg:(g + 1) * cg], k, 1)                                         # (N, T, k * cg), column (j, ci)
        wg = w[g * cg:(g + 1) * cg].permute(0, 2, 1).reshape(cg, k * cg)
        out.append(win @ wg.T)
    return torch.cat(out, dim=-1) + bias


def w2v_forward(sd, x, cfg, dtype=torch.float64, bf16_storage: bool = False, sdpa: bool = False, group_norm: bool = True,
                zero_q: bool = False):
    """-> last_hidden_state (N, T, d) in ``dtype``.  ``group_norm=False`` / ``zero_q=True`` are the two ablations the CPU test
    uses to show that the captured weights make the GroupNorm and the softmax matter."""
    on, dev = bf16_storage, x.device
    W = lambda k: _r(sd[k].to(dev, dtype), on, dtype)           # GEMM weights are read from the bf16 shadow
    F = lambda k: sd[k].to(dev, dtype)                          # biases, norm parameters and layer 0 stay f32 masters
    d, H, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    dh, ks, ss = d // H, cfg.conv_kernel, cfg.conv_stride
    fe = "feature_extractor.conv_layers."
    N = x.shape[0]
    h = conv0_raw(x.to(dtype), F(fe + "0.conv.weight"), ss[0])
    if group_norm:
        mean, var = conv0_stats(h)
        h = (h - mean) / torch.sqrt(var + GN_EPS) * F(fe + "0.layer_norm.weight") + F(fe + "0.layer_norm.bias")
    h = _r(gelu_erf(h), on, dtype)
    for i in range(1, len(ks)):
        w = W(f"{fe}{i}.conv.weight")
        raw = _r(window(h, ks[i], ss[i]) @ w.permute(0, 2, 1).reshape(w.shape[0], -1).T, on, dtype)
        h = _r(gelu_erf(raw), on, dtype)
    h = _r(layer_norm(h, F("feature_projection.layer_norm.weight"), F("feature_projection.layer_norm.bias"), eps), on, dtype)
    h = _r(h @ W("feature_projection.projection.weight").T + F("feature_projection.projection.bias"), on, dtype)
    pw = _r(pos_weight(sd, dtype, dev), on, dtype)
    h = _r(h + gelu_erf(pos_conv(h, pw, F(WN + "bias"), cfg.num_conv_pos_embedding_groups)), on, dtype)
    h = _r(layer_norm(h, F("encoder.layer_norm.weight"), F("encoder.layer_norm.bias"), eps), on, dtype)
    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layers.{i}."
        q = _r(h @ W(a + "attention.q_proj.weight").T + F(a + "attention.q_proj.bias"), on, dtype)
        k = _r(h @ W(a + "attention.k_proj.weight").T + F(a + "attention.k_proj.bias"), on, dtype)
        v = _r(h @ W(a + "attention.v_proj.weight").T + F(a + "attention.v_proj.bias"), on, dtype)
        if zero_q:
            q = torch.zeros_like(q)
        q, k, v = (t.reshape(N, -1, H, dh).transpose(1, 2) for t in (q, k, v))
        if sdpa:
            att = torch.nn.functional.scaled_dot_product_attention(q, k, v)
        else:
            att = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh), dim=-1) @ v
        att = _r(att.transpose(1, 2).reshape(N, -1, d), on, dtype)
        y = _r(att @ W(a + "attention.out_proj.weight").T + F(a + "attention.out_proj.bias") + h, on, dtype)
        ln = _r(layer_norm(y, F(a + "layer_norm.weight"), F(a + "layer_norm.bias"), eps), on, dtype)
        f1 = _r(ln @ W(a + "feed_forward.intermediate_dense.weight").T, on, dtype)               # GELU input as stored (the bias is added in f32)
        g = _r(gelu_erf(f1 + F(a + "feed_forward.intermediate_dense.bias")), on, dtype)
        y = _r(g @ W(a + "feed_forward.output_dense.weight").T + F(a + "feed_forward.output_dense.bias") + ln, on, dtype)
        h = _r(layer_norm(y, F(a + "final_layer_norm.weight"), F(a + "final_layer_norm.bias"), eps), on, dtype)
    return h


class RefWav2Vec2(torch.nn.Module):
    """``w2v_forward`` behind the ``backbone=`` protocol of the encoders (``.config.hidden_size``, one positional input)"""

    def __init__(self, sd, cfg, dtype=torch.float32):
        super().__init__()
        self.config, self.sd, self.dtype = cfg, sd, dtype

    def forward(self, input_values, attention_mask=None):
        with torch.no_grad():
            out = w2v_forward(self.sd, input_values, self.config, dtype=self.dtype).float()
        return types.SimpleNamespace(last_hidden_state=out)
