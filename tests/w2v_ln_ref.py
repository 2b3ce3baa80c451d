"""The Wav2Vec2 forward of the layer-norm family (HuggingFace ``Wav2Vec2Model`` with ``feat_extract_norm="layer"``,
``conv_bias=True``, ``do_stable_layer_norm=True``: wav2vec2-large-lv60, large-robust, xlsr-53, XLS-R) restated as explicit tensor
math, written from the architecture: every feature-extractor layer is Conv1d(bias) -> LayerNorm over channels -> exact GELU, then
LayerNorm -> projection -> x + gelu(weight-normed grouped positional convolution) with NO LayerNorm behind it -> pre-LN transformer
layers (``Wav2Vec2EncoderStableLayerNorm``) -> ``encoder.layer_norm``.  It imports neither transformers nor the code under test;
the pieces both families share come from tests/w2v_ref.py.

``bf16_storage=True`` rounds where the HIP path stores bf16: layer 0 after its GELU, each raw conv output after the bias, each
LayerNorm + GELU output, then as ``w2v_ref`` (every GEMM / LayerNorm / attention output, the GELU output, the GEMM weights, the
folded positional weight, the positional kernel's output).

Two ablations and one wrong arrangement for the CPU test's mutants: ``inner_norm=False`` drops the LayerNorm of the conv layers
``>= 1``, ``conv_bias=False`` drops every conv bias, ``post_ln=True`` runs the base family's encoder on the same weights.
"""
import math
import types

import torch

from w2v_ref import WN, WN_NEW, WN_OLD, _r, config_kwargs, gelu_erf, layer_norm, pos_conv, pos_weight, window  # noqa: F401
import w2v_ref

CONV_LN_EPS = 1e-5       # nn.LayerNorm's default, which HuggingFace's layer-norm conv layer keeps


def _config(**kw):
    base = dict(conv_bias=True, layer_norm_eps=1e-5, feat_extract_norm="layer", do_stable_layer_norm=True)
    return types.SimpleNamespace(**{**base, **kw})


def ln_tiny():
    return _config(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, conv_dim=(256, 256, 256),
                   conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


def ln_wide():
    """the large family's widths: d 1024 in 16 heads, positional group width 64 with 128 taps, 512 channels = one wave per frame"""
    return _config(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096, conv_dim=(512, 512, 512),
                   conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)


def ln_768():
    """d 768 in 12 heads and 16 positional groups (width 48) of 15 taps, 2 layers, the tiny conv stack: the width ``AudioEncoder``'s
    tail can follow"""
    return _config(hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=512, conv_dim=(256, 256, 256),
                   conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), num_conv_pos_embeddings=15, num_conv_pos_embedding_groups=16)


def hf_keys(cfg, legacy_weight_norm: bool = False):
    """the ``Wav2Vec2Model`` state_dict of the family: key -> shape, in HuggingFace's order"""
    base = w2v_ref.hf_keys(cfg, legacy_weight_norm)
    fe = "feature_extractor.conv_layers."
    out = {}
    for k, shape in base.items():
        if k.startswith(fe) and k.endswith(".layer_norm.weight"):
            continue                                                   # (layer 0's, placed below with the other layers')
        if k.startswith(fe) and k.endswith(".layer_norm.bias"):
            continue
        out[k] = shape
        if k.startswith(fe) and k.endswith(".conv.weight"):
            i = k[len(fe):].split(".")[0]
            out[f"{fe}{i}.conv.bias"] = out[f"{fe}{i}.layer_norm.weight"] = out[f"{fe}{i}.layer_norm.bias"] = (shape[0],)
    return out


def seeded_weights(cfg, seed: int = 0, legacy_weight_norm: bool = False):
    """``w2v_ref.seeded_weights``' recipe on the family's keys (non-trivial conv biases and norm parameters among them)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in hf_keys(cfg, legacy_weight_norm).items():
        t = torch.randn(shape, generator=g)
        if k.endswith("norm.weight"):
            t = 1.0 + 0.2 * t
        elif k.endswith(".bias"):
            t = 0.1 * t
        elif k in (WN_NEW[0], WN_OLD[0]):
            t = math.sqrt(cfg.hidden_size / shape[2]) * (1.0 + 0.3 * torch.rand(shape, generator=g))
        elif k in (WN_NEW[1], WN_OLD[1]) or k == "masked_spec_embed":
            pass
        elif len(shape) == 3:
            t = t * math.sqrt(2.0 / (shape[1] * shape[2]))
        else:
            t = t / math.sqrt(shape[1]) * (1.5 if ("q_proj" in k or "k_proj" in k) else 1.0)
        sd[k] = t
    return sd


def features(sd, x, cfg, dtype=torch.float64, bf16_storage: bool = False, inner_norm: bool = True, conv_bias: bool = True):
    """the feature extractor: (N, L) -> (N, T, conv_dim[-1]) after the last layer's GELU"""
    on, dev = bf16_storage, x.device
    W = lambda k: _r(sd[k].to(dev, dtype), on, dtype)
    F = lambda k: sd[k].to(dev, dtype)
    ks, ss = cfg.conv_kernel, cfg.conv_stride
    fe = "feature_extractor.conv_layers."
    bias = lambda i: F(f"{fe}{i}.conv.bias") if conv_bias else 0.0
    norm = lambda i, h: layer_norm(h, F(f"{fe}{i}.layer_norm.weight"), F(f"{fe}{i}.layer_norm.bias"), CONV_LN_EPS)
    h = w2v_ref.conv0_raw(x.to(dtype), F(fe + "0.conv.weight"), ss[0]) + bias(0)
    h = _r(gelu_erf(norm(0, h)), on, dtype)                                                       # layer 0: one store
    for i in range(1, len(ks)):
        w = W(f"{fe}{i}.conv.weight")
        raw = _r(window(h, ks[i], ss[i]) @ w.permute(0, 2, 1).reshape(w.shape[0], -1).T + bias(i), on, dtype)
        h = _r(gelu_erf(norm(i, raw) if inner_norm else raw), on, dtype)
    return h


def w2v_forward(sd, x, cfg, dtype=torch.float64, bf16_storage: bool = False, sdpa: bool = False, inner_norm: bool = True,
                conv_bias: bool = True, post_ln: bool = False):
    """-> last_hidden_state (N, T, d) in ``dtype``"""
    on, dev = bf16_storage, x.device
    W = lambda k: _r(sd[k].to(dev, dtype), on, dtype)
    F = lambda k: sd[k].to(dev, dtype)
    LN = lambda h, name: _r(layer_norm(h, F(name + ".weight"), F(name + ".bias"), eps), on, dtype)
    d, H, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    dh, N = d // H, x.shape[0]
    h = features(sd, x, cfg, dtype, bf16_storage, inner_norm, conv_bias)
    h = LN(h, "feature_projection.layer_norm")
    h = _r(h @ W("feature_projection.projection.weight").T + F("feature_projection.projection.bias"), on, dtype)
    pw = _r(pos_weight(sd, dtype, dev), on, dtype)
    h = _r(h + gelu_erf(pos_conv(h, pw, F(WN + "bias"), cfg.num_conv_pos_embedding_groups)), on, dtype)
    if post_ln:
        h = LN(h, "encoder.layer_norm")

    def attention(src, a):
        q, k, v = (_r(src @ W(f"{a}attention.{n}_proj.weight").T + F(f"{a}attention.{n}_proj.bias"), on, dtype) for n in "qkv")
        q, k, v = (t.reshape(N, -1, H, dh).transpose(1, 2) for t in (q, k, v))
        if sdpa:
            att = torch.nn.functional.scaled_dot_product_attention(q, k, v)
        else:
            att = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh), dim=-1) @ v
        att = _r(att.transpose(1, 2).reshape(N, -1, d), on, dtype)
        return att @ W(a + "attention.out_proj.weight").T + F(a + "attention.out_proj.bias")

    def mlp(src, a):
        f1 = _r(src @ W(a + "feed_forward.intermediate_dense.weight").T, on, dtype)               # GELU input as stored (the bias is added in f32)
        g = _r(gelu_erf(f1 + F(a + "feed_forward.intermediate_dense.bias")), on, dtype)
        return g @ W(a + "feed_forward.output_dense.weight").T + F(a + "feed_forward.output_dense.bias")

    for i in range(cfg.num_hidden_layers):
        a = f"encoder.layers.{i}."
        if post_ln:
            ln = LN(_r(attention(h, a) + h, on, dtype), a + "layer_norm")
            h = LN(_r(mlp(ln, a) + ln, on, dtype), a + "final_layer_norm")
        else:
            y = _r(attention(LN(h, a + "layer_norm"), a) + h, on, dtype)
            h = _r(mlp(LN(y, a + "final_layer_norm"), a) + y, on, dtype)
    return h if post_ln else LN(h, "encoder.layer_norm")


class RefWav2Vec2(torch.nn.Module):
    """``w2v_forward`` behind the ``backbone=`` protocol of the encoders (``.config.hidden_size``, one positional input)"""

    def __init__(self, sd, cfg, dtype=torch.float32):
        super().__init__()
        self.config, self.sd, self.dtype = cfg, sd, dtype

    def forward(self, input_values, attention_mask=None):
        with torch.no_grad():
            out = w2v_forward(self.sd, input_values, self.config, dtype=self.dtype).float()
        return types.SimpleNamespace(last_hidden_state=out)
