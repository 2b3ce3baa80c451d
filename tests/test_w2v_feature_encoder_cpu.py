"""CPU: the bookkeeping of ``NativeWav2Vec2.set_trainable_layers(L, front=True, feature_encoder=True)`` (which parameters require a
gradient beside those of ``front=True``, the refusals, the unchanged ``state_dict`` surface), ``"full"`` through ``AudioEncoder``'s
``config.audio_backbone_trainable_layers``, ``finetune_optimizer`` on it, and two facts the GPU bounds of
tests/test_w2v_feature_encoder_gpu.py and tests/test_w2v_feature_encoder_kernels_gpu.py rest on, in float64 through tests/w2v_ref.py."""
import pytest
import torch

import w2v_ref
from test_w2v_finetune_cpu import FRONT, _grads, _layers, _model, _trainable

FEATURE = ["conv0_gn_b", "conv0_gn_w", "conv0_w", "conv1_w", "conv2_w"]          # the tiny config's feature extractor
FEATURE_KEYS = ["feature_extractor.conv_layers.0.conv.weight", "feature_extractor.conv_layers.0.layer_norm.weight",
                "feature_extractor.conv_layers.0.layer_norm.bias", "feature_extractor.conv_layers.1.conv.weight",
                "feature_extractor.conv_layers.2.conv.weight"]


def test_which_parameters_require_a_gradient():
    m = _model()
    L = m.config.num_hidden_layers
    assert m.trainable_feature_encoder is False
    m.set_trainable_layers(L, front=True)
    all_ = _trainable(m)
    assert all_ == sorted(_layers(m, L) + FRONT) and m.trainable_feature_encoder is False
    m.set_trainable_layers(L, front=True, feature_encoder=True)
    assert m.trainable_layers == L and m.trainable_front is True and m.trainable_feature_encoder is True
    assert _trainable(m) == sorted(all_ + FEATURE)                                  # "full" = "all" + the feature extractor
    assert not m.masked_spec_embed.requires_grad                                  # today's rule: with the time mask only
    m.set_regularisation(mask_time_prob=0.05)
    assert _trainable(m) == sorted(all_ + FEATURE + ["masked_spec_embed"])
    m.set_regularisation(mask_time_prob=0.0)
    assert _trainable(m) == sorted(all_ + FEATURE)
    assert sorted(m._trainable_names()) == _trainable(m)
    m.set_trainable_layers(L, front=True)                                         # back to "all": the flag does not stick
    assert m.trainable_feature_encoder is False and _trainable(m) == all_
    m.set_trainable_layers(L, front=True, feature_encoder=True)
    m.set_trainable_layers(0)
    assert m.trainable_feature_encoder is False and m.trainable_front is False and _trainable(m) == []
    with pytest.raises(AttributeError):                                           # read-only
        m.trainable_feature_encoder = True


def test_refusals():
    m = _model()
    L = m.config.num_hidden_layers
    with pytest.raises(ValueError, match="feature_encoder"):
        m.set_trainable_layers(L, front=False, feature_encoder=True)
    with pytest.raises(ValueError, match="feature_encoder"):
        m.set_trainable_layers(L, feature_encoder=True)
    for k in range(L):
        with pytest.raises(ValueError):
            m.set_trainable_layers(k, front=True, feature_encoder=True)
        with pytest.raises(ValueError):
            m.set_trainable_layers(k, feature_encoder=True)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="feature_encoder"):
            m.set_trainable_layers(L, front=True, feature_encoder=bad)
    assert m.trainable_layers == 0 and not m.trainable_feature_encoder and _trainable(m) == []       # a refused call changes nothing
    m.set_trainable_layers(L, front=True, feature_encoder=True)
    with pytest.raises(ValueError):
        m.set_trainable_layers(1, front=True, feature_encoder=True)
    assert m.trainable_layers == L and m.trainable_feature_encoder


def test_state_dict_surface_is_unchanged():
    cfg = w2v_ref.tiny_config()
    m = _model(cfg)
    want = w2v_ref.hf_keys(cfg)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.set_trainable_layers(cfg.num_hidden_layers, front=True, feature_encoder=True)
    sd = m.state_dict()
    assert list(sd) == list(want)
    assert all(tuple(sd[key].shape) == tuple(shape) for key, shape in want.items())
    assert not any(v.requires_grad for v in sd.values())
    assert all(torch.equal(sd[k], before[k]) for k in want)
    assert [k for k in want if m._hf[k][0] in FEATURE] == FEATURE_KEYS


def _encoder(**kw):
    import config as cfgmod
    from models.encoders import AudioEncoder
    tcfg = w2v_ref.tiny_config()
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 256
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = {k: v for k, v in w2v_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
    for key, v in kw.items():
        setattr(cfg, key, v)
    return AudioEncoder(cfg)


def test_audio_encoder_config_full():
    enc = _encoder(audio_backbone_trainable_layers="full")
    assert enc.model.trainable_layers == 2 and enc.model.trainable_front and enc.model.trainable_feature_encoder
    assert _trainable(enc.model) == sorted(_layers(enc.model, 2) + FRONT + FEATURE)
    enc = _encoder(audio_backbone_trainable_layers="all")                          # "all", integers and 0: as before
    assert enc.model.trainable_front and not enc.model.trainable_feature_encoder
    assert _trainable(enc.model) == sorted(_layers(enc.model, 2) + FRONT)
    enc = _encoder(audio_backbone_trainable_layers=1)
    assert enc.model.trainable_layers == 1 and not enc.model.trainable_front and not enc.model.trainable_feature_encoder
    assert not _encoder(audio_backbone_trainable_layers=0).model.trainable_feature_encoder
    with pytest.raises(ValueError):
        _encoder(audio_backbone_trainable_layers="everything")


def test_finetune_optimizer_collects_the_feature_extractor():
    """what ``mmfusion.train.finetune_optimizer`` hands to ``FusedAdamW``: the parameters that require a gradient, the feature
    extractor's five tensors among them under "full" and not under "all" (the optimiser itself needs a GPU: tests/
    test_w2v_feature_encoder_gpu.py steps it)"""
    for mode, there in (("full", True), ("all", False)):
        enc = _encoder(audio_backbone_trainable_layers=mode)
        picked = {id(p) for p in enc.parameters() if p.requires_grad}               # finetune_optimizer's own expression
        for n in FEATURE:
            assert (id(getattr(enc.model, n)) in picked) == there, (mode, n)
    import inspect
    from mmfusion import train
    assert "if p.requires_grad" in inspect.getsource(train.finetune_optimizer)


# ---- facts the GPU tests' bounds rely on --------------------------------------------------------------------------------
def test_rule_b_is_not_degenerate_for_the_feature_extractor():
    """Rule (b), ||got - exact|| <= 2 ||stored - exact||, needs the bf16-storage gradient to differ from the exact one: it does for
    the five feature-extractor tensors of the tiny config at 3 x 3000 samples, for the random gradient of the result and for the
    one on frame 0 only (printed: ||stored - exact|| / ||exact|| per tensor; 1.6e-2 to 2.0e-2)"""
    cfg = w2v_ref.tiny_config()
    sd = w2v_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(7)
    x = 0.5 * torch.randn(3, 3000, generator=g) + 0.1
    T = w2v_ref.w2v_forward(sd, x[:1].double(), cfg).shape[1]
    dout = torch.randn(3, T, cfg.hidden_size, generator=g, dtype=torch.float64)
    row0 = torch.zeros_like(dout)
    row0[:, 0] = dout[:, 0]
    for tag, d in (("random", dout), ("frame-0", row0)):
        exact, stored = _grads(sd, x, cfg, d, FEATURE_KEYS, False), _grads(sd, x, cfg, d, FEATURE_KEYS, True)
        for k in FEATURE_KEYS:
            rel = float((stored[k] - exact[k]).norm() / exact[k].norm())
            print(f"{tag} dO, {k}: ||stored - exact|| / ||exact|| = {rel:.3e}")
            assert 1e-3 < rel < 0.5, (tag, k)


def test_the_unread_trailing_frame_of_layer_0_matters():
    """3007 samples give layer 0 600 frames of which layer 1 (kernel 3, stride 2) reads 0 .. 598.  Frame 599 receives no gradient
    from above (dy = 0) but took part in the GroupNorm's statistics, so the gradient dc of the convolution's output is not zero
    there and the frame belongs in d conv0.weight: with dc zeroed on it the weight gradient moves by far more than the 1e-5 the
    GPU test of ``mmf_w2v_conv0_bwd_wgrad`` holds it to"""
    g = torch.Generator().manual_seed(8)
    C0, k0, s0, k1, s1 = 16, 10, 5, 3, 2
    wave = (0.5 * torch.randn(2, 3007, generator=g) + 0.1).double()
    gamma, beta = (1.0 + 0.2 * torch.randn(C0, generator=g)).double(), (0.1 * torch.randn(C0, generator=g)).double()
    w_init = (0.3 * torch.randn(C0, 1, k0, generator=g)).double()
    T0 = (3007 - k0) // s0 + 1
    T1 = (T0 - k1) // s1 + 1
    assert T0 == 600 and s1 * (T1 - 1) + k1 - 1 == 598
    dwin = torch.randn(2, T1, k1 * C0, generator=g, dtype=torch.float64)

    def dw0(drop_unread: bool):
        w = w_init.clone().requires_grad_(True)
        c = w2v_ref.conv0_raw(wave, w, s0)
        if drop_unread:
            keep = torch.ones(T0, 1, dtype=torch.float64)
            keep[599:] = 0.0
            c.register_hook(lambda grad: grad * keep)
        mean, var = w2v_ref.conv0_stats(c)
        y = (c - mean) / torch.sqrt(var + w2v_ref.GN_EPS) * gamma + beta
        return torch.autograd.grad(w2v_ref.window(w2v_ref.gelu_erf(y), k1, s1), w, dwin)[0]
    full, dropped = dw0(False), dw0(True)
    rel = float((dropped - full).norm() / full.norm())
    print(f"d conv0.weight with dc zeroed on the unread frame 599: {rel:.3e} from the full gradient (relative L2)")
    assert rel > 1e-4
