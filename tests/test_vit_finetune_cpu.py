"""CPU: the bookkeeping of ``NativeViT.set_trainable_layers`` (which parameters require a gradient, the refusals, the unchanged
``state_dict`` surface), ``VideoEncoder``'s ``config.video_backbone_trainable_layers``, the K-slab cut of a weight gradient's rows,
and the fact the backward relies on for the key bias: its exact gradient is zero."""
import pytest
import torch

import vit_ref


def _model(cfg=None):
    from mmfusion.vit import NativeViT
    return NativeViT(**vit_ref.config_kwargs(cfg or vit_ref.tiny_config()))


def _trainable(m):
    return sorted(n for n, p in m.named_parameters() if p.requires_grad)


def _layers(m, k):
    L = m.config.num_hidden_layers
    return sorted([n for i in range(L - k, L) for n in m._layer_params(i)] + (["ln_w", "ln_b"] if k else []))


EMBEDDINGS = ["cls_token", "patch_bias", "patch_weight", "position_embeddings"]


def test_which_parameters_require_a_gradient():
    m = _model()
    L = m.config.num_hidden_layers
    assert m.trainable_layers == 0 and m.trainable_embeddings is False and _trainable(m) == []
    for k in (1, L, 0):
        m.set_trainable_layers(k)
        assert m.trainable_layers == k and m.trainable_embeddings is False
        assert _trainable(m) == _layers(m, k)
    m.set_trainable_layers(L, embeddings=True)
    assert m.trainable_layers == L and m.trainable_embeddings is True
    assert _trainable(m) == sorted(_layers(m, L) + EMBEDDINGS)
    assert not m.pooler_w.requires_grad and not m.pooler_b.requires_grad
    m.set_trainable_layers(0)
    assert m.trainable_layers == 0 and m.trainable_embeddings is False and _trainable(m) == []
    with pytest.raises(AttributeError):                            # both are read-only
        m.trainable_layers = 1
    with pytest.raises(AttributeError):
        m.trainable_embeddings = True


def test_refusals():
    m = _model()
    L = m.config.num_hidden_layers
    for bad in (True, False, -1, L + 1, 1.0, "1", None):
        with pytest.raises(ValueError):
            m.set_trainable_layers(bad)
    for k in range(L):
        with pytest.raises(ValueError):
            m.set_trainable_layers(k, embeddings=True)
    with pytest.raises(ValueError):
        m.set_trainable_layers(L, embeddings=1)
    assert m.trainable_layers == 0 and _trainable(m) == []          # a refused call changes nothing


def test_state_dict_surface_is_unchanged():
    cfg = vit_ref.tiny_config()
    m = _model(cfg)
    want = vit_ref.hf_keys(cfg)
    for k, emb in ((0, False), (1, False), (cfg.num_hidden_layers, True)):
        m.set_trainable_layers(k, embeddings=emb)
        sd = m.state_dict()
        assert list(sd) == list(want)
        assert all(tuple(sd[key].shape) == tuple(shape) for key, shape in want.items())
        assert not any(v.requires_grad for v in sd.values())


def test_video_encoder_config_values():
    import config as cfgmod
    from models.encoders import VideoEncoder

    def build(**kw):
        cfg = cfgmod.ModelConfig()
        cfg.fusion_hidden_size, cfg.fusion_dropout = 256, 0.0
        cfg.video_hidden_size, cfg.video_frame_size = 256, (64, 64)
        cfg.video_backbone = "native"
        cfg.video_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=1024, num_attention_heads=4)
        for key, v in kw.items():
            setattr(cfg, key, v)
        return VideoEncoder(cfg)
    enc = build()
    assert enc.vit.trainable_layers == 0 and _trainable(enc.vit) == []
    enc = build(video_backbone_trainable_layers=0)
    assert enc.vit.trainable_layers == 0 and _trainable(enc.vit) == []
    enc = build(video_backbone_trainable_layers=1)
    assert enc.vit.trainable_layers == 1 and not enc.vit.trainable_embeddings and _trainable(enc.vit) == _layers(enc.vit, 1)
    enc = build(video_backbone_trainable_layers="all")
    assert enc.vit.trainable_layers == 2 and enc.vit.trainable_embeddings
    assert _trainable(enc.vit) == sorted(_layers(enc.vit, 2) + EMBEDDINGS)
    with pytest.raises(ValueError):
        build(video_backbone_trainable_layers=3)


@pytest.mark.parametrize("rows,slabs", [(1000, 1), (1000, 3), (1000, 7), (31520, 7), (31520, 28), (40, 5), (1, 3), (64, 2)])
def test_slab_bounds_cut_the_rows_at_multiples_of_32(rows, slabs):
    from mmfusion.backbone import FrozenBackbone
    cuts = FrozenBackbone._slab_bounds(rows, slabs)
    assert cuts[0] == 0 and cuts[-1] == rows and all(a < b for a, b in zip(cuts, cuts[1:]))
    assert len(cuts) - 1 == min(slabs, (rows + 31) // 32)
    assert all(c % 32 == 0 for c in cuts[:-1])
    lengths = [b - a for a, b in zip(cuts, cuts[1:])]
    assert max(lengths) - min(lengths[:-1] or lengths) <= 32


@pytest.mark.parametrize("cls", [False, True], ids=["forward", "cls_features"])
def test_the_key_bias_has_no_gradient_in_float64(cls):
    """a shift of every key by one vector moves every score of a softmax row equally: d k_proj.bias is zero, on both routes"""
    cfg = vit_ref.tiny_config()
    sd = vit_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, cfg.num_channels, cfg.image_size, cfg.image_size, generator=g)
    leaves = {k: v.double().clone().requires_grad_(".attention." in k and k.endswith("_proj.bias")) for k, v in sd.items()}
    out = vit_ref.vit_forward(leaves, x, cfg, dtype=torch.float64, cls_last_only=cls)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    for i in range(cfg.num_hidden_layers):
        gk = float(leaves[f"layers.{i}.attention.k_proj.bias"].grad.norm())
        gq = float(leaves[f"layers.{i}.attention.q_proj.bias"].grad.norm())
        print(f"layer {i} ({'cls' if cls else 'full'}): ||d k_proj.bias|| {gk:.3e}, ||d q_proj.bias|| {gq:.3e}")
        assert gq > 0 and gk <= 1e-10 * gq
