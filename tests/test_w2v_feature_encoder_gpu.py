"""GPU: training the native Wav2Vec2's feature encoder, ``NativeWav2Vec2.set_trainable_layers(L, front=True, feature_encoder=True)``
(``config.audio_backbone_trainable_layers = "full"``): every gradient of that mode against float64 autograd through the restatement
tests/w2v_ref.py, the K-slab form of the conv layers' weight gradients, the arena's accumulation protocol, graph capture, the
optimiser step through ``AudioEncoder`` with the stale-shadow check, and the regularised step.

Bounds.  Rule (b) per parameter tensor, ||got - exact|| <= 2 ||stored - exact|| (tests/test_deberta_finetune_gpu.py's ``_rule_b``;
``exact`` / ``stored``: autograd through ``w2v_ref.w2v_forward`` without / with ``bf16_storage``).  It is not degenerate for the
feature extractor's tensors: tests/test_w2v_feature_encoder_cpu.py measures ||stored - exact|| / ||exact|| at 1.4e-2 to 2.0e-2 for
each.  The key bias is held to zero, as in tests/test_w2v_finetune_gpu.py.  The swapped conv weights' gradients are compared in
HuggingFace's (C_out, C_in, k)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_ref  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402
from test_deberta_finetune_gpu import _frozen_grads_are_empty, _rule_b  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402
from test_w2v_finetune_gpu import _check_key_bias, _douts, _pick, _ref_grads, _setup, _without_key_bias  # noqa: E402

_FE = "feature_extractor."


def _hf_grads(m, keys):
    """{key: the f32 gradient in HuggingFace's shape}: a parameter stored with its last two dims swapped (the inner conv weights,
    (C_out, k, C_in)) is permuted back"""
    out = {}
    for key in keys:
        name, rows, swapped = m._hf[key]
        g = getattr(m, name).grad
        assert g is not None and g.dtype == torch.float32, key
        g = g if rows is None else g[rows[0]:rows[1]]
        out[key] = (g.permute(0, 2, 1) if swapped else g).detach().cpu().clone()
    return out


def _full_keys(cfg):
    """every tensor "full" trains: all of the state dict but the mask embedding (frozen while the time mask is off)"""
    return [k for k in w2v_ref.hf_keys(cfg) if k != "masked_spec_embed"]


def _feature_keys(cfg):
    return [k for k in w2v_ref.hf_keys(cfg) if k.startswith(_FE)]


def _full(m):
    m.set_trainable_layers(m.config.num_hidden_layers, front=True, feature_encoder=True)


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


def _tiny_case(which="tiny"):
    cfg, sd, m, x = _setup(which, 3, 3007)
    assert m.frames(3007) == 149
    return cfg, sd, m, x, _full_keys(cfg)


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_every_gradient_of_full_against_float64_autograd(which):
    """3 clips of 3007 samples in chunks of 2 (a chunk of 2 and one of 1): 600 / 299 / 149 frames, so layers 0 and 1 both end in a
    frame the layer above never reads; a random gradient of the result and one on frame 0 only"""
    cfg, sd, m, x, keys = _tiny_case(which)
    with torch.no_grad():
        plain = m(x.cuda()).last_hidden_state.clone()
    _full(m)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted({m._hf[key][0] for key in keys})
    kept = _without_key_bias(keys)
    for tag, dout in _douts(cfg, 3, 149, 51):
        exact = _ref_grads((which, 3007, tag), sd, x, cfg, dout, torch.float64, False, keys)
        stored = _ref_grads((which, 3007, tag), sd, x, cfg, dout, torch.float64, True, keys)
        got, out = _native_grads(m, x.cuda(), dout, keys)
        assert torch.equal(_bits(out), _bits(plain)), "the differentiable forward's bits are not the inference call's"
        _rule_b(f"NativeWav2Vec2 {which} 3 x 3007, full, {tag} dO,", _pick(got, kept), _pick(exact, kept), _pick(stored, kept))
        _check_key_bias(m, keys)
        _frozen_grads_are_empty(m)


def test_every_gradient_of_full_at_base_sizes():
    """wav2vec2-base sizes (7 conv layers of 512 channels, 12 layers), 2 clips of 16000 samples (T = 49), float32 references.  The
    worst error / bound is in profiles/w2v_feature_encoder.txt"""
    cfg, sd, m, x = _setup("base", 2, 16000)
    _full(m)
    keys = _full_keys(cfg)
    (_, dout), _ = _douts(cfg, 2, m.frames(16000), 53)
    exact = _ref_grads("base-full", sd, x, cfg, dout, torch.float32, False, keys)
    stored = _ref_grads("base-full", sd, x, cfg, dout, torch.float32, True, keys)
    got, _ = _native_grads(m, x.cuda(), dout, keys)
    kept = _without_key_bias(keys)
    _rule_b("NativeWav2Vec2 base 2 x 16000, full,", _pick(got, kept), _pick(exact, kept), _pick(stored, kept))
    _check_key_bias(m, keys)
    _frozen_grads_are_empty(m)


def test_the_k_slab_weight_gradient_form_forced(monkeypatch):
    """small shapes never pick the K-slab form (``_slabs_for`` gives 1), so it is forced: 3 slabs for every weight-gradient launch.
    The conv weights' gradients hold rule (b) as the plain launches' do, differ from them by a change of summation order at
    most, and have the same bits on two runs"""
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg, sd, m, x, _ = _tiny_case()
    keys = [k for k in _feature_keys(cfg) if k.endswith("conv.weight")]
    _full(m)
    (tag, dout), _ = _douts(cfg, 3, 149, 51)
    every = _full_keys(cfg)
    exact = _pick(_ref_grads(("tiny", 3007, tag), sd, x, cfg, dout, torch.float64, False, every), keys)
    stored = _pick(_ref_grads(("tiny", 3007, tag), sd, x, cfg, dout, torch.float64, True, every), keys)
    plain, _ = _native_grads(m, x.cuda(), dout, keys)
    seen = []

    def three(rows, tiles):
        seen.append((rows, tiles))
        return 3
    monkeypatch.setattr(NativeWav2Vec2, "_slabs_for", staticmethod(three))
    slabbed, _ = _native_grads(m, x.cuda(), dout, keys)
    again, _ = _native_grads(m, x.cuda(), dout, keys)
    assert (2 * 149, 2) in seen and (2 * 299, 3) in seen                # conv2_w (256 x 512: 2 tiles) and conv1_w (256 x 768: 3) asked
    _rule_b("NativeWav2Vec2 tiny 3 x 3007, full, 3 K-slabs forced,", slabbed, exact, stored)
    for key in keys:
        e = l2_rel(slabbed[key], plain[key])
        print(f"3 K-slabs vs the plain launch, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
        assert torch.equal(_bits(slabbed[key]), _bits(again[key])), key


def test_gradients_accumulate_and_honour_the_lazy_zero_protocol():
    from mmfusion import arena
    cfg, sd, m, x, _ = _tiny_case()
    _full(m)
    keys = _feature_keys(cfg)
    (_, dout), _ = _douts(cfg, 3, 149, 51)
    once, _ = _native_grads(m, x.cuda(), dout, keys)
    twice, _ = _native_grads(m, x.cuda(), dout, keys, zero=False)
    for key in keys:
        e = l2_rel(twice[key], 2 * once[key])
        print(f"two backwards vs 2 x one, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    ar = arena.ensure(m)
    ar.zero_grad(lazy=True)
    _native_grads(m, x.cuda(), dout, keys, zero=False)
    ar.finalize_grads()
    torch.cuda.synchronize()
    again = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(again[key], once[key])
        print(f"after zero_grad(lazy=True), {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    _frozen_grads_are_empty(m)


def test_forward_and_backward_replay_from_a_captured_graph():
    """a fixed shape, one stream: the replayed feature-extractor gradients are the eager call's bits (their sums go through no
    atomics), and they follow the static input"""
    from mmfusion import arena
    cfg, sd, m, x, _ = _tiny_case()
    _full(m)
    keys = _feature_keys(cfg)
    (_, dout), _ = _douts(cfg, 3, 149, 63)
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
        assert torch.equal(_bits(got[key]), _bits(eager[key])), key
    assert all(l2_rel(other[key], eager[key]) > 1e-2 for key in keys)


def test_audio_encoder_full_steps_the_feature_extractor_and_keeps_its_shadows_current():
    """one ``finetune_optimizer`` step through ``AudioEncoder`` with ``audio_backbone_trainable_layers = "full"`` moves ``conv0_w`` (read
    as an f32 master) and ``conv3_w`` (read through its bf16 shadow), and the next forward is the restatement's on the UPDATED
    state dict within ``BOUND_A``: a conv weight's shadow left at its old value would show (the restatement on the old state dict
    is printed beside it)"""
    import config as cfgmod
    from mmfusion import arena
    from mmfusion.train import finetune_optimizer
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=512, conv_dim=(256, 256, 256, 256), conv_kernel=(10, 3, 3, 2),
                                     conv_stride=(5, 2, 2, 2), num_conv_pos_embeddings=16)
    cfg.audio_backbone_trainable_layers = "full"
    cfg.encoder_attention_weights = False
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    wcfg = enc.model.config
    assert enc.model.trainable_feature_encoder and enc.model.trainable_front and enc.model.trainable_layers == 2
    old = w2v_ref.seeded_weights(wcfg, seed=31)
    enc.model.load_state_dict(old)
    enc = enc.cuda().train()
    wave = (0.5 * torch.randn(2, 3000, generator=torch.Generator().manual_seed(32))).cuda()
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    before = {n: p.detach().clone() for n, p in enc.model.named_parameters()}
    ar.zero_grad()
    enc(wave)["features"].sum().backward()
    opt.advance()
    opt.launch()
    torch.cuda.synchronize()
    for n in ("conv0_w", "conv0_gn_w", "conv0_gn_b", "conv1_w", "conv2_w", "conv3_w"):
        p = getattr(enc.model, n)
        assert p.requires_grad and not torch.equal(_bits(p.detach()), _bits(before[n])), f"{n} did not move"
    assert torch.equal(_bits(enc.model.masked_spec_embed.detach()), _bits(before["masked_spec_embed"]))
    with torch.no_grad():
        got = enc.model(wave).last_hidden_state.cpu()
    new = {k: v.detach().cpu().clone() for k, v in enc.model.state_dict().items()}
    want = w2v_ref.w2v_forward(new, wave.cpu().double(), wcfg, dtype=torch.float64)
    stale = w2v_ref.w2v_forward(old, wave.cpu().double(), wcfg, dtype=torch.float64)
    e, e_old = l2_rel(got, want), l2_rel(got, stale)
    print(f"AudioEncoder 'full', the forward after one step vs the restatement on the updated state dict: rel L2 {e:.3e} (bound {BOUND_A}); "
          f"on the old one {e_old:.3e}")
    assert e <= BOUND_A < e_old


def test_regularised_step_gives_finite_repeatable_feature_encoder_gradients():
    """``train()`` under wav2vec2-base-960h's regularisers without LayerDrop: a fixed seed gives the same bits twice, another seed
    other gradients"""
    from mmfusion import ops
    from mmfusion.wav2vec2 import REG_960H
    cfg, sd, m, x, _ = _tiny_case()
    _full(m)
    m.set_regularisation(**dict(REG_960H, layerdrop=0.0))
    m.train()
    keys = _feature_keys(cfg)
    (_, dout), _ = _douts(cfg, 3, 149, 71)
    runs = []
    for seed in (5, 5, 6):
        ops.seed_dropout(seed)
        runs.append(_native_grads(m, x.cuda(), dout, keys)[0])
    for key in keys:
        assert bool(torch.isfinite(runs[0][key]).all()) and float(runs[0][key].norm()) > 0, key
        assert torch.equal(_bits(runs[0][key]), _bits(runs[1][key])), key
        assert not torch.equal(_bits(runs[0][key]), _bits(runs[2][key])), key
    assert m.masked_spec_embed.requires_grad and bool(torch.isfinite(m.masked_spec_embed.grad).all())
