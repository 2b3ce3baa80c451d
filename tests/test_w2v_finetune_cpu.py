"""CPU: the bookkeeping of ``NativeWav2Vec2.set_trainable_layers`` (which parameters require a gradient, the refusals, the
unchanged ``state_dict`` surface), ``AudioEncoder``'s ``config.audio_backbone_trainable_layers``, the restatements of the positional
convolution's backward in tests/w2v_grad_ref.py against float64 autograd, the bound feasibility of the front end's tensors, and the
fact the backward relies on for the key bias: its exact gradient is zero."""
import pytest
import torch

import w2v_grad_ref as G
import w2v_ref

FRONT = ["enc_ln_b", "enc_ln_w", "fp_b", "fp_ln_b", "fp_ln_w", "fp_w", "pos_b", "pos_g", "pos_v"]
NEVER = ["masked_spec_embed", "conv0_w", "conv0_gn_w", "conv0_gn_b", "conv1_w", "conv2_w"]


def _model(cfg=None):
    from mmfusion.wav2vec2 import NativeWav2Vec2
    return NativeWav2Vec2(**w2v_ref.config_kwargs(cfg or w2v_ref.tiny_config()))


def _trainable(m):
    return sorted(n for n, p in m.named_parameters() if p.requires_grad)


def _layers(m, k):
    L = m.config.num_hidden_layers
    return sorted(n for i in range(L - k, L) for n in m._layer_params(i))


def test_which_parameters_require_a_gradient():
    m = _model()
    L = m.config.num_hidden_layers
    assert m.trainable_layers == 0 and m.trainable_front is False and _trainable(m) == []
    for k in (1, L, 0):
        m.set_trainable_layers(k)
        assert m.trainable_layers == k and m.trainable_front is False
        assert _trainable(m) == _layers(m, k)
    m.set_trainable_layers(L, front=True)
    assert m.trainable_layers == L and m.trainable_front is True
    assert _trainable(m) == sorted(_layers(m, L) + FRONT)
    assert not any(getattr(m, n).requires_grad for n in NEVER)      # the feature extractor, its GroupNorm, the mask embedding
    m.set_trainable_layers(0)
    assert m.trainable_layers == 0 and m.trainable_front is False and _trainable(m) == []
    with pytest.raises(AttributeError):                            # both are read-only
        m.trainable_layers = 1
    with pytest.raises(AttributeError):
        m.trainable_front = True


def test_refusals():
    m = _model()
    L = m.config.num_hidden_layers
    for bad in (True, False, -1, L + 1, 1.0, "1", None):
        with pytest.raises(ValueError):
            m.set_trainable_layers(bad)
    for k in range(L):
        with pytest.raises(ValueError):
            m.set_trainable_layers(k, front=True)
    with pytest.raises(ValueError):
        m.set_trainable_layers(L, front=1)
    assert m.trainable_layers == 0 and _trainable(m) == []          # a refused call changes nothing


def test_state_dict_surface_is_unchanged():
    cfg = w2v_ref.tiny_config()
    m = _model(cfg)
    want = w2v_ref.hf_keys(cfg)
    for k, front in ((0, False), (1, False), (cfg.num_hidden_layers, True)):
        m.set_trainable_layers(k, front=front)
        sd = m.state_dict()
        assert list(sd) == list(want)
        assert all(tuple(sd[key].shape) == tuple(shape) for key, shape in want.items())
        assert not any(v.requires_grad for v in sd.values())


def test_audio_encoder_config_values():
    import config as cfgmod
    from models.encoders import AudioEncoder
    tcfg = w2v_ref.tiny_config()

    def build(**kw):
        cfg = cfgmod.ModelConfig()
        cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 256
        cfg.audio_backbone = "native"
        cfg.audio_backbone_kwargs = {k: v for k, v in w2v_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
        for key, v in kw.items():
            setattr(cfg, key, v)
        return AudioEncoder(cfg)
    enc = build()
    assert enc.model.trainable_layers == 0 and _trainable(enc.model) == []
    enc = build(audio_backbone_trainable_layers=0)
    assert enc.model.trainable_layers == 0 and _trainable(enc.model) == []
    enc = build(audio_backbone_trainable_layers=1)
    assert enc.model.trainable_layers == 1 and not enc.model.trainable_front and _trainable(enc.model) == _layers(enc.model, 1)
    enc = build(audio_backbone_trainable_layers="all")
    assert enc.model.trainable_layers == 2 and enc.model.trainable_front
    assert _trainable(enc.model) == sorted(_layers(enc.model, 2) + FRONT)
    with pytest.raises(ValueError):
        build(audio_backbone_trainable_layers=3)


def test_finetune_optimizer_collects_by_requires_grad():
    """``mmfusion.train.finetune_optimizer`` needs no change for the audio backbone: it takes what requires a gradient"""
    import inspect
    from mmfusion import train
    assert "if p.requires_grad" in inspect.getsource(train.finetune_optimizer)


# ---- the restatements of tests/w2v_grad_ref.py against float64 autograd ------------------------------------------------
def _l2(a, b):
    return float((a - b).norm() / b.norm())


CASES = [(2, 40, 2, 16, 5), (2, 40, 2, 16, 16), (1, 9, 2, 32, 16), (3, 7, 4, 16, 15), (2, 21, 3, 48, 4), (1, 130, 2, 16, 128)]


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=[f"T{c[1]}-cg{c[3]}-k{c[4]}" for c in CASES])
def test_packings_and_the_two_gradients_against_float64_autograd(N, T, groups, cg, k):
    """odd and even k, T shorter than k: the forward on the packed weight, the input gradient as the forward on the reversed /
    swapped weight with k - 1 - k // 2 rows in front (for an even k that is one less than the forward's k // 2), the weight
    gradient as a sum over time per tap"""
    g = torch.Generator().manual_seed(T * k + cg)
    C = groups * cg
    x = torch.randn(N, T, C, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(C, cg, k, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    dz = torch.randn(N, T, C, generator=g, dtype=torch.float64)
    z = w2v_ref.pos_conv(x, w, bias, groups)
    dx, dw = torch.autograd.grad(z, [x, w], dz)
    assert _l2(G.conv_packed(x.detach(), G.pack(w.detach()), cg, k, k // 2) + bias, z.detach()) <= 1e-10
    assert _l2(G.conv_input_grad(dz, w.detach()), dx) <= 1e-10
    assert _l2(G.conv_weight_grad(dz, x.detach(), cg, k), G.pack(dw)) <= 1e-10
    assert torch.equal(G.unpack(G.pack(dw), cg), dw)
    if k % 2 == 0 and T > 1:                                          # the forward's padding in the input gradient is wrong for an even k
        wrong = G.conv_packed(dz, G.pack_transposed(w.detach()), cg, k, k // 2)
        assert _l2(wrong, dx) > 1e-2


@pytest.mark.parametrize("C,cg,k", [(32, 16, 5), (64, 16, 16), (96, 48, 15)])
def test_weightnorm_backward_against_float64_autograd(C, cg, k):
    g = torch.Generator().manual_seed(C + k)
    gain = (1.0 + torch.rand(1, 1, k, generator=g, dtype=torch.float64)).requires_grad_(True)
    v = torch.randn(C, cg, k, generator=g, dtype=torch.float64).requires_grad_(True)
    dw = torch.randn(C, cg, k, generator=g, dtype=torch.float64)
    w = w2v_ref.pos_weight({w2v_ref.WN_NEW[0]: gain, w2v_ref.WN_NEW[1]: v})
    dg, dv = torch.autograd.grad(w, [gain, v], dw)
    got_g, got_v = G.weightnorm_bwd(dw, gain.detach(), v.detach())
    assert got_g.shape == dg.shape and got_v.shape == dv.shape
    assert _l2(got_g, dg) <= 1e-10 and _l2(got_v, dv) <= 1e-10


# ---- facts the GPU tests' bounds rely on --------------------------------------------------------------------------------
def _grads(sd, x, cfg, dout, keys, bf16_storage):
    leaves = {k: v.double().clone().requires_grad_(k in keys) for k, v in sd.items()}
    out = w2v_ref.w2v_forward(leaves, x.double(), cfg, dtype=torch.float64, bf16_storage=bf16_storage)
    return dict(zip(keys, torch.autograd.grad(out, [leaves[k] for k in keys], dout)))


def test_the_key_bias_has_no_gradient_in_float64():
    """a shift of every key by one vector moves every score of a softmax row equally: d k_proj.bias is zero"""
    cfg = w2v_ref.tiny_config()
    sd = w2v_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1500, generator=g)
    keys = [k for k in sd if ".attention." in k and k.endswith(("k_proj.bias", "q_proj.bias"))]
    T = w2v_ref.w2v_forward(sd, x.double(), cfg).shape[1]
    grads = _grads(sd, x, cfg, torch.randn(2, T, cfg.hidden_size, generator=g, dtype=torch.float64), keys, False)
    for i in range(cfg.num_hidden_layers):
        gk = float(grads[f"encoder.layers.{i}.attention.k_proj.bias"].norm())
        gq = float(grads[f"encoder.layers.{i}.attention.q_proj.bias"].norm())
        print(f"layer {i}: ||d k_proj.bias|| {gk:.3e}, ||d q_proj.bias|| {gq:.3e}")
        assert gq > 0 and gk <= 1e-10 * gq


def test_rule_b_is_not_degenerate_for_the_front_end():
    """Rule (b) of tests/test_w2v_finetune_gpu.py, ||got - exact|| <= 2 ||stored - exact||, needs the bf16-storage gradient to
    differ from the exact one: it does for every tensor of the front end, the weight norm's g and v and the feature projection
    included (printed: ||stored - exact|| / ||exact|| per tensor)"""
    cfg = w2v_ref.tiny_config()
    sd = w2v_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 1500, generator=g)
    keys = [k for k in sd if k.startswith(("feature_projection.", "encoder.pos_conv_embed.", "encoder.layer_norm."))]
    T = w2v_ref.w2v_forward(sd, x.double(), cfg).shape[1]
    dout = torch.randn(2, T, cfg.hidden_size, generator=g, dtype=torch.float64)
    exact, stored = _grads(sd, x, cfg, dout, keys, False), _grads(sd, x, cfg, dout, keys, True)
    assert len(keys) == 9
    for k in keys:
        rel = float((stored[k] - exact[k]).norm() / exact[k].norm())
        print(f"{k}: ||stored - exact|| / ||exact|| = {rel:.3e}")
        assert 1e-4 < rel < 0.5, k
