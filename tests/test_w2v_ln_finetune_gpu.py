"""GPU: fine-tuning the native Wav2Vec2 of the layer-norm family (pre-LN layers, ``encoder.layer_norm`` on top of them) in
HuggingFace's ``freeze_feature_encoder()`` regime.  The weight gradients of ``NativeWav2Vec2.set_trainable_layers(k[, front=True])``
against float64 autograd through the restatement tests/w2v_ln_ref.py, the arena's accumulation protocol, graph capture, and the
optimiser step through ``AudioEncoder``.

Bounds.  Rule (b) per parameter tensor, ||got - exact|| <= 2 ||stored - exact|| (``_rule_b`` of tests/test_deberta_finetune_gpu.py),
``exact`` / ``stored`` the autograd gradients of ``w2v_ln_ref.w2v_forward`` without / with ``bf16_storage``; both sides are computed
here and printed per tensor.  tests/test_w2v_ln_ref_cpu.py shows that the rule is degenerate for no tensor but the key bias, whose
exact gradient is zero and to which the backward adds nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_ln_ref  # noqa: E402
from test_deberta_finetune_gpu import _frozen_grads_are_empty, _hf_grads, _rule_b  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402
from helpers import l2_rel  # noqa: E402

_FRONT = ("feature_projection.", "encoder.pos_conv_embed.")
_TOP = "encoder.layer_norm."
_CFG = {"tiny": w2v_ln_ref.ln_tiny, "768": w2v_ln_ref.ln_768}
_ref_cache = {}


def _setup(which, n=3, L=3000, seed=21, chunk=2):
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg = _CFG[which]()
    sd = w2v_ln_ref.seeded_weights(cfg, seed=seed)
    m = NativeWav2Vec2(**{**w2v_ln_ref.config_kwargs(cfg), "chunk": chunk})
    m.load_state_dict(sd)
    x = 0.5 * torch.randn(n, L, generator=torch.Generator().manual_seed(seed + 1)) + 0.1
    return cfg, sd, m.cuda().eval(), x


def _keys(cfg, k, front=False):
    """HuggingFace's keys of what ``set_trainable_layers(k, front)`` trains: the top ``k`` layers, ``encoder.layer_norm`` above them
    from k = 1 on, and with ``front`` the feature projection and the positional convolution"""
    L = cfg.num_hidden_layers
    names = w2v_ln_ref.hf_keys(cfg)
    keys = [key for key in names if any(key.startswith(f"encoder.layers.{i}.") for i in range(L - k, L))]
    return ([key for key in names if key.startswith(_FRONT)] if front else []) + keys + ([key for key in names if key.startswith(_TOP)] if k else [])


def _ref_grads(tag, sd, x, cfg, dout, bf16_storage, keys):
    """float64 autograd through the restatement with the state dict's tensors as leaves -> {key: gradient}; kept per ``tag`` so that
    the tests that share a case compute it once"""
    key_ = (tag, bf16_storage, tuple(keys))
    if key_ not in _ref_cache:
        leaves = {key: v.double().clone().requires_grad_(key in keys) for key, v in sd.items()}
        out = w2v_ln_ref.w2v_forward(leaves, x.double(), cfg, bf16_storage=bf16_storage, dtype=torch.float64)
        _ref_cache[key_] = dict(zip(keys, torch.autograd.grad(out, [leaves[key] for key in keys], dout.double())))
    return _ref_cache[key_]


def _native_grads(m, x, dout, keys, zero=True):
    from mmfusion import arena
    ar = arena.ensure(m)
    if zero:
        ar.zero_grad()
    out = m(x).last_hidden_state
    assert out.requires_grad and out.dtype == torch.float32
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    return _hf_grads(m, keys), out.detach()


def _douts(cfg, n, T, seed):
    """a random gradient of the result and one that is non-zero on frame 0 of each clip only"""
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(n, T, cfg.hidden_size, generator=g)
    row0 = torch.zeros_like(dout)
    row0[:, 0] = dout[:, 0]
    return [("random", dout), ("frame-0", row0)]


def _without_key_bias(keys):
    return [k for k in keys if not k.endswith("k_proj.bias")]


def _check_key_bias(m, keys):
    for key in keys:
        if key.endswith("k_proj.bias"):
            name, rows, _ = m._hf[key]
            assert not bool(getattr(m, name).grad[rows[0]:rows[1]].any()), f"{key} received a gradient"


def _pick(d, keys):
    return {key: d[key] for key in keys}


@pytest.mark.parametrize("k,front", [(1, False), (2, False), (2, True)], ids=["k1", "k2", "all"])
@pytest.mark.parametrize("which", ["tiny", "768"])
def test_weight_gradients_against_float64_autograd(which, k, front):
    """2 layers; 3 clips of 3000 samples in chunks of 2: T = 149, odd and past one 128-row block"""
    cfg, sd, m, x = _setup(which)
    T = m.frames(3000)
    assert T == 149
    with torch.no_grad():
        plain = m(x.cuda()).last_hidden_state.clone()
    m.set_trainable_layers(k, front=front)
    keys = _keys(cfg, k, front)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted({m._hf[key][0] for key in keys})
    assert any(key.startswith(_TOP) for key in keys)
    every = _keys(cfg, 2, True)                                     # one autograd pass serves the three parametrisations
    for tag, dout in _douts(cfg, 3, T, 51):
        exact = _ref_grads((which, tag), sd, x, cfg, dout, False, every)
        stored = _ref_grads((which, tag), sd, x, cfg, dout, True, every)
        got, out = _native_grads(m, x.cuda(), dout, keys)
        assert torch.equal(_bits(out), _bits(plain)), "the differentiable forward's bits are not the inference call's"
        kept = _without_key_bias(keys)
        _rule_b(f"NativeWav2Vec2 ln_{which} 3 x 3000, k={k}{' + front end' if front else ''}, {tag} dO,", _pick(got, kept), _pick(exact, kept),
                _pick(stored, kept))
        assert float(got[_TOP + "weight"].norm()) > 0 and float(got[_TOP + "bias"].norm()) > 0      # encoder.layer_norm at k = 1 as well
        _check_key_bias(m, keys)
        _frozen_grads_are_empty(m)


def test_gradients_accumulate_to_twice_one():
    """two backward calls without zeroing give twice the gradient within ``F32_TOL``, and hold rule (b) on the doubled reference"""
    cfg, sd, m, x = _setup("tiny")
    L = cfg.num_hidden_layers
    m.set_trainable_layers(L, front=True)
    keys = _without_key_bias(_keys(cfg, L, True))
    (tag, dout), _ = _douts(cfg, 3, m.frames(3000), 51)
    every = _keys(cfg, 2, True)
    exact = _ref_grads(("tiny", tag), sd, x, cfg, dout, False, every)
    stored = _ref_grads(("tiny", tag), sd, x, cfg, dout, True, every)
    once, _ = _native_grads(m, x.cuda(), dout, keys)
    twice, _ = _native_grads(m, x.cuda(), dout, keys, zero=False)
    _rule_b("NativeWav2Vec2 ln_tiny, two backwards without zeroing against 2 x the reference,", twice, {k: 2 * exact[k] for k in keys},
            {k: 2 * stored[k] for k in keys})
    for key in keys:
        e = l2_rel(twice[key], 2 * once[key])
        print(f"two backwards vs 2 x one, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    _frozen_grads_are_empty(m)


def test_forward_and_backward_replay_from_a_captured_graph():
    """k = 2 with the front end, a fixed shape, one stream: the replayed gradients are the eager call's within ``F32_TOL`` (the bound
    of a change of summation order: the LayerNorm parameters' and the biases' sums go through f32 atomics)"""
    from mmfusion import arena
    cfg, sd, m, x = _setup("tiny")
    m.set_trainable_layers(2, front=True)
    keys = _without_key_bias(_keys(cfg, 2, True))
    (_, dout), _ = _douts(cfg, 3, m.frames(3000), 63)
    eager, _ = _native_grads(m, x.cuda(), dout, keys)
    ar = arena.ensure(m)
    static, dO = x.cuda().clone(), dout.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        m(static).last_hidden_state.backward(dO)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m(static).last_hidden_state.backward(dO)
    with torch.no_grad():
        static.copy_(torch.randn_like(static))
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    other = _hf_grads(m, keys)
    with torch.no_grad():
        static.copy_(x.cuda())
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    got = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(got[key], eager[key])
        print(f"captured forward + backward, {key}: rel L2 vs eager {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    assert any(l2_rel(other[key], eager[key]) > 1e-2 for key in keys)


def test_audio_encoder_steps_the_trainable_parameters():
    """one ``finetune_optimizer`` step at width 768 with ``audio_backbone_trainable_layers = 1``: the top layer and
    ``encoder.layer_norm`` move with the encoder's own parameters, everything else stays, and the next forward follows the new weights"""
    import config as cfgmod
    from mmfusion import arena
    from mmfusion.train import finetune_optimizer
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = {k: v for k, v in w2v_ln_ref.config_kwargs(w2v_ln_ref.ln_768()).items() if k != "hidden_size"}
    cfg.audio_backbone_trainable_layers = 1
    cfg.encoder_attention_weights = False
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    wcfg = enc.model.config
    L = wcfg.num_hidden_layers
    assert enc.model.trainable_layers == 1 and not enc.model.trainable_front and wcfg.do_stable_layer_norm
    sd = w2v_ln_ref.seeded_weights(wcfg, seed=31)
    enc.model.load_state_dict(sd)
    enc = enc.cuda().train()
    wave = (0.5 * torch.randn(2, 3000, generator=torch.Generator().manual_seed(32))).cuda()
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    ar.zero_grad()
    feats = enc(wave)["features"]
    assert feats.requires_grad
    first = feats.detach().clone()
    feats.sum().backward()
    torch.cuda.synchronize()
    opt.advance()
    opt.launch()
    torch.cuda.synchronize()
    names = enc.model._layer_params(L - 1) + ["enc_ln_w", "enc_ln_b"]
    assert sorted(n for n, p in enc.model.named_parameters() if p.requires_grad) == sorted(names)
    for n, p in enc.named_parameters():
        same = torch.equal(_bits(p.detach()), _bits(before[n]))
        if n.startswith("model."):
            key_bias = "_qkv_b" in n                                                   # (a third of it, the key bias, has no gradient)
            assert same != p.requires_grad or key_bias, f"{n}: {'did not move' if same else 'is frozen and moved'}"
        elif p.requires_grad and n.startswith(("temporal_attention.", "projection.")):
            assert not same, f"{n} did not move"
        elif not p.requires_grad:
            assert same, f"the frozen {n} moved"
    with torch.no_grad():
        second = enc(wave)["features"]
    moved = l2_rel(second, first)
    # the same encoder on the restatement of the stepped weights: the next forward reads what the optimiser wrote
    sd2 = {k: v.detach().cpu().clone() for k, v in enc.model.state_dict().items()}
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = AudioEncoder(cfg_ref, backbone=w2v_ln_ref.RefWav2Vec2(sd2, wcfg))
    ref.load_state_dict({k: v for k, v in enc.state_dict().items() if not k.startswith("model.")})
    with torch.no_grad():
        want = ref.cuda().eval()(wave)["features"]
    err, scale = float((second - want).abs().max()), max(1.0, float(want.abs().max()))
    print(f"after one step the features moved by {moved:.3e}; against the restatement of the new weights: abs err {err:.3e} (bound {1e-2 * scale:.3e}), "
          f"of the old ones' output {float((first - want).abs().max()):.3e}")
    assert moved > 0 and err <= 1e-2 * scale
