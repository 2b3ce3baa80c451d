"""The ViT forward (HuggingFace ``ViTModel`` up to ``last_hidden_state``) restated as explicit tensor math, written from the
architecture: strided patch extraction -> patch linear -> [CLS] + position embeddings -> pre-LN transformer layers
(LayerNorm, fused q/k/v, softmax attention, out-projection + residual, LayerNorm, fc1, exact GELU, fc2 + residual) ->
final LayerNorm.  It imports neither transformers nor the code under test.

Weights are a ``state_dict`` in the key naming of transformers 5.x (``layers.N.attention.q_proj.weight`` ...).

``bf16_storage=True`` models the storage format of the HIP path, not its kernels: values are rounded to bf16 exactly where
that path writes bf16 to memory (patches, GEMM weights, every GEMM / LayerNorm / attention output, the tokens, the GELU input
and output) and everything between two stores is computed in ``dtype``.

``dtype=torch.bfloat16`` on a GPU tensor, with ``sdpa=True``, is the stock-torch yardstick of tools/vit_bench.py: the same
forward through rocBLAS and torch's attention.
"""
import math
import types

import torch

from backbone_ref import _r, config_kwargs, gelu_erf, layer_norm  # noqa: F401  (the tests read them from here)


def tiny_config():
    return types.SimpleNamespace(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                                 image_size=64, patch_size=16, num_channels=3, layer_norm_eps=1e-12)


def base_config():
    return types.SimpleNamespace(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                                 image_size=224, patch_size=16, num_channels=3, layer_norm_eps=1e-12)


def hf_keys(cfg):
    """the 5.x ``ViTModel`` state_dict: key -> shape, in HuggingFace's order"""
    d, I, P, C = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size, cfg.num_channels
    T = (cfg.image_size // P) ** 2 + 1
    out = {"embeddings.cls_token": (1, 1, d), "embeddings.position_embeddings": (1, T, d),
           "embeddings.patch_embeddings.projection.weight": (d, C, P, P), "embeddings.patch_embeddings.projection.bias": (d,)}
    for i in range(cfg.num_hidden_layers):
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            out[f"layers.{i}.attention.{n}.weight"] = (d, d)
            out[f"layers.{i}.attention.{n}.bias"] = (d,)
        for n in ("layernorm_before", "layernorm_after"):
            out[f"layers.{i}.{n}.weight"] = (d,)
            out[f"layers.{i}.{n}.bias"] = (d,)
        out[f"layers.{i}.mlp.fc1.weight"], out[f"layers.{i}.mlp.fc1.bias"] = (I, d), (I,)
        out[f"layers.{i}.mlp.fc2.weight"], out[f"layers.{i}.mlp.fc2.bias"] = (d, I), (d,)
    out["layernorm.weight"], out["layernorm.bias"] = (d,), (d,)
    out["pooler.dense.weight"], out["pooler.dense.bias"] = (d, d), (d,)
    return out


def seeded_weights(cfg, seed: int = 0):
    """Weights with spread enough that the forward exercises everything: 1/sqrt(fan_in)-scaled matrices, with the q / k
    projections 1.5 times that so the softmax rows are far from uniform; non-trivial biases and LayerNorm parameters."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in hf_keys(cfg).items():
        t = torch.randn(shape, generator=g)
        if k.endswith("layernorm_before.weight") or k.endswith("layernorm_after.weight") or k == "layernorm.weight":
            t = 1.0 + 0.2 * t
        elif k.endswith(".bias"):
            t = 0.1 * t
        elif len(shape) == 3:                                   # cls token, position embeddings
            t = 0.5 * t
        else:
            fan_in = t[0].numel()
            t = t / math.sqrt(fan_in) * (1.5 if ("q_proj" in k or "k_proj" in k) else 1.0)
        sd[k] = t
    return sd


def patchify(pixels, P):
    """(N, C, H, W) -> (N * gh * gw, C * P * P), row (n, gy, gx), column (c, py, px): Conv2d(kernel P, stride P) as a matmul"""
    N, C, H, W = pixels.shape
    gh, gw = H // P, W // P
    return pixels.reshape(N, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, C * P * P)


def vit_forward(sd, pixels, cfg, bf16_storage: bool = False, dtype=torch.float64, cls_last_only: bool = False,
                sdpa: bool = False, return_probs: bool = False):
    """-> last_hidden_state (N, T, d) in ``dtype``; with ``cls_last_only`` (N, d): the last layer evaluated for the CLS
    query rows only (the same numbers as [:, 0] of the full result up to rounding, fewer operations).
    ``return_probs``: also the attention probabilities of layer 0, (N, H, T, T)."""
    on = bf16_storage
    dev = pixels.device
    W = lambda k: _r(sd[k].to(dev, dtype), on, dtype)           # GEMM weights are read from the bf16 shadow
    F = lambda k: sd[k].to(dev, dtype)                          # biases, LayerNorm parameters, cls / pos stay f32 masters
    d, H, P, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.patch_size, cfg.layer_norm_eps
    dh = d // H
    N = pixels.shape[0]
    patches = _r(patchify(pixels.to(dtype), P), on, dtype)
    pe = _r(patches @ W("embeddings.patch_embeddings.projection.weight").reshape(d, -1).T
            + F("embeddings.patch_embeddings.projection.bias"), on, dtype)
    pos = F("embeddings.position_embeddings")
    x = torch.cat([F("embeddings.cls_token").expand(N, 1, d), pe.reshape(N, -1, d)], dim=1) + pos
    x = _r(x, on, dtype)
    T = x.shape[1]
    probs0 = None
    for i in range(cfg.num_hidden_layers):
        a, last = f"layers.{i}.attention.", cls_last_only and i == cfg.num_hidden_layers - 1
        ln = _r(layer_norm(x, F(f"layers.{i}.layernorm_before.weight"), F(f"layers.{i}.layernorm_before.bias"), eps), on, dtype)
        lnq = ln[:, :1] if last else ln
        q = _r(lnq @ W(a + "q_proj.weight").T + F(a + "q_proj.bias"), on, dtype)
        k = _r(ln @ W(a + "k_proj.weight").T + F(a + "k_proj.bias"), on, dtype)
        v = _r(ln @ W(a + "v_proj.weight").T + F(a + "v_proj.bias"), on, dtype)
        Tq = q.shape[1]
        q, k, v = (t.reshape(N, -1, H, dh).transpose(1, 2) for t in (q, k, v))
        if sdpa:
            att = torch.nn.functional.scaled_dot_product_attention(q, k, v)
        else:
            s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
            p = torch.softmax(s, dim=-1)
            if i == 0:
                probs0 = p
            att = p @ v
        att = _r(att.transpose(1, 2).reshape(N, Tq, d), on, dtype)
        res = x[:, :1] if last else x
        y = _r(att @ W(a + "o_proj.weight").T + F(a + "o_proj.bias") + res, on, dtype)
        ln2 = _r(layer_norm(y, F(f"layers.{i}.layernorm_after.weight"), F(f"layers.{i}.layernorm_after.bias"), eps), on, dtype)
        h = _r(ln2 @ W(f"layers.{i}.mlp.fc1.weight").T, on, dtype)                      # GELU input as stored (the bias is added in f32)
        g = _r(gelu_erf(h + F(f"layers.{i}.mlp.fc1.bias")), on, dtype)
        x = _r(g @ W(f"layers.{i}.mlp.fc2.weight").T + F(f"layers.{i}.mlp.fc2.bias") + y, on, dtype)
    out = _r(layer_norm(x, F("layernorm.weight"), F("layernorm.bias"), eps), on, dtype)
    if cls_last_only:
        out = out[:, 0]
    return (out, probs0) if return_probs else out


class RefViT(torch.nn.Module):
    """``vit_forward`` behind the ``backbone=`` protocol of the encoders (``.config.hidden_size``, ``pixel_values=``)"""

    def __init__(self, sd, cfg, dtype=torch.float32):
        super().__init__()
        self.config, self.sd, self.dtype = cfg, sd, dtype

    def forward(self, pixel_values):
        with torch.no_grad():
            out = vit_forward(self.sd, pixel_values, self.config, dtype=self.dtype).float()
        return types.SimpleNamespace(last_hidden_state=out)
