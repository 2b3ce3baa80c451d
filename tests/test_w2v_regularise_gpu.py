"""GPU: ``NativeWav2Vec2`` fine-tuned under HuggingFace's training-mode regularisers.  The forward and every trainable gradient,
``masked_spec_embed``'s included, against float64 autograd through tests/w2v_regularise_ref.py under the masks it restates; chunk
independence; the plain call's bits and launch list where nothing acts; LayerDrop; graph capture; the optimiser step through
``AudioEncoder``.

Bounds are tests/test_w2v_finetune_gpu.py's: rule (b) per parameter tensor, ||got - exact|| <= 2 ||stored - exact||, both references
computed here under the restated masks; the forward within BOUND_A of the bf16-storage restatement.  The key bias still receives
nothing.  3 clips of 3000 samples (T = 149) in chunks of 2, as there.  ``mask_time_prob`` is 0.2 here so that a clip draws 2 or 3
spans of 10 frames (0.05 at T = 149 always draws the minimum of 2)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_ref  # noqa: E402
import w2v_regularise_ref as R  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402
from test_backbone_launches_gpu import _assert_same, _recorded  # noqa: E402
from test_deberta_finetune_gpu import _frozen_grads_are_empty, _hf_grads, _rule_b  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402
from test_w2v_finetune_gpu import _check_key_bias, _douts, _keys, _pick, _setup, _without_key_bias  # noqa: E402

SEED = 1234
STATE = (SEED << 20) + 1
SETTINGS = dict(R.SETTINGS_960H, layerdrop=0.0, mask_time_prob=0.2)
N, LW, T = 3, 3000, 149
_refs = {}


def _model(which, k, front, settings=SETTINGS, chunk=2):
    cfg, sd, m, x = _setup(which, N, LW, chunk=chunk)
    m.set_trainable_layers(k, front=front)
    m.set_regularisation(**settings)
    return cfg, sd, m.train(), x


def _all_keys(cfg):
    return ["masked_spec_embed"] + _keys(cfg, cfg.num_hidden_layers, True)


def _ref(which, cfg, sd, x, dout, bf16_storage, settings=SETTINGS, skip=None, state=STATE):
    """float64 autograd through the training-mode restatement under the restated masks -> ({key: gradient}, the output); once per case"""
    key = (which, bf16_storage, tuple(sorted(settings.items())), None if skip is None else tuple(skip), state)
    if key not in _refs:
        keys = _all_keys(cfg)
        masks = R.call_masks(state, R.sites(cfg.num_hidden_layers), cfg, N, T, settings)
        leaves = {k_: v.double().clone().requires_grad_(k_ in keys) for k_, v in sd.items()}
        out = R.w2v_forward(leaves, x.double(), cfg, masks, skip=skip, bf16_storage=bf16_storage)
        grads = torch.autograd.grad(out, [leaves[k_] for k_ in keys], dout.double(), allow_unused=True)
        _refs[key] = ({k_: (torch.zeros_like(leaves[k_]) if g is None else g) for k_, g in zip(keys, grads)}, out.detach())
    return _refs[key]


def _grads(m, x, dout, keys, seed=SEED, zero=True):
    from mmfusion import arena, ops
    ar = arena.ensure(m)
    if zero:
        ar.zero_grad()
    if seed is not None:
        ops.seed_dropout(seed)
    out = m(x).last_hidden_state
    assert out.requires_grad and out.dtype == torch.float32
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    return _hf_grads(m, keys), out.detach()


@pytest.mark.parametrize("k,front", [(1, False), (2, False), (2, True)], ids=["k1", "k2", "all"])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_forward_and_gradients_against_float64_autograd_under_the_restated_masks(which, k, front):
    cfg, sd, m, x = _model(which, k, front)
    assert m.frames(LW) == T
    keys = (["masked_spec_embed"] if front else []) + _keys(cfg, k, front)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted({m._hf[key][0] for key in keys})
    (tag, dout), _ = _douts(cfg, N, T, 51)
    exact, out_exact = _ref(which, cfg, sd, x, dout, False)
    stored, out_stored = _ref(which, cfg, sd, x, dout, True)
    got, out = _grads(m, x.cuda(), dout, keys)
    a, b, model_err = l2_rel(out.cpu(), out_stored), l2_rel(out.cpu(), out_exact), l2_rel(out_stored, out_exact)
    plain = w2v_ref.w2v_forward(sd, x, cfg, bf16_storage=True)
    print(f"NativeWav2Vec2 {which} {N} x {LW}, regularised: forward (a) vs the bf16-storage restatement under the restated masks {a:.3e} "
          f"(bound {BOUND_A}); (b) vs the exact one {b:.3e} (bound {2 * model_err:.3e}); the inference restatement is {l2_rel(out.cpu(), plain):.3e} away")
    assert a <= BOUND_A and b <= 2 * model_err and l2_rel(out.cpu(), plain) > 10 * BOUND_A
    kept = _without_key_bias(keys)
    _rule_b(f"NativeWav2Vec2 {which} {N} x {LW}, regularised, k={k}{' + front end' if front else ''}, {tag} dO,", _pick(got, kept), _pick(exact, kept),
            _pick(stored, kept))
    _check_key_bias(m, keys)
    _frozen_grads_are_empty(m)
    if front:
        assert float(got["masked_spec_embed"].norm()) > 0


def test_chunk_size_does_not_change_the_result():
    runs = {}
    for chunk in (1, 2, 3):
        cfg, sd, m, x = _model("tiny", 2, True, chunk=chunk)
        keys = _without_key_bias(_all_keys(cfg))
        (_, dout), _ = _douts(cfg, N, T, 51)
        runs[chunk] = _grads(m, x.cuda(), dout, keys)
    for chunk in (1, 2):
        assert torch.equal(_bits(runs[chunk][1]), _bits(runs[3][1])), f"the output at chunk {chunk} differs from chunk 3's"
        for key, g in runs[chunk][0].items():                       # parameter gradients are sums over the chunks: f32 summation order
            e = l2_rel(g, runs[3][0][key])
            print(f"chunk {chunk} vs chunk 3, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
            assert e <= F32_TOL, key


def test_eval_no_grad_and_zero_settings_give_the_plain_bits_and_launch_list():
    cfg, sd, plain, x = _model("tiny", 2, True, settings={})
    xd = x.cuda()
    keys = _without_key_bias(_keys(cfg, 2, True))
    (_, dout), _ = _douts(cfg, N, T, 51)
    want, want_out = _grads(plain, xd, dout, keys)
    step = lambda mod: (lambda: mod(xd).last_hidden_state.backward(dout.cuda()))
    want_list = _recorded(step(plain))
    with torch.no_grad():
        infer_list = _recorded(lambda: plain(xd))
    _, _, m, _ = _model("tiny", 2, True)
    with torch.no_grad():
        out = m(xd).last_hidden_state
        _assert_same(_recorded(lambda: m(xd)), infer_list)
    assert not out.requires_grad and torch.equal(_bits(out), _bits(want_out)), "no_grad"
    m.eval()
    got, out = _grads(m, xd, dout, keys)
    assert torch.equal(_bits(out), _bits(want_out)), "eval()"
    _assert_same(_recorded(step(m)), want_list)
    m.train()
    m.set_regularisation(**{n: 0.0 for n in R.SETTINGS_960H if n not in ("mask_time_length", "mask_time_min_masks")})
    got0, out0 = _grads(m, xd, dout, keys)
    assert torch.equal(_bits(out0), _bits(want_out)), "all settings 0 in train()"
    _assert_same(_recorded(step(m)), want_list)
    for key in keys:
        for g in (got, got0):
            if key.endswith(".bias") or "layer_norm" in key:            # (sums through f32 atomics: two runs differ in the last bits)
                assert l2_rel(g[key], want[key]) <= F32_TOL, key
            else:
                assert torch.equal(_bits(g[key]), _bits(want[key])), key
    assert not m.masked_spec_embed.requires_grad
    # a frozen module with the settings on: every call is the inference call
    m.set_regularisation(**SETTINGS)
    m.set_trainable_layers(0)
    again = m(xd).last_hidden_state
    assert not again.requires_grad and torch.equal(_bits(again), _bits(want_out))
    # and with them on the regularised call's list differs
    m.set_trainable_layers(2, front=True)
    assert len(_recorded(step(m))) > len(want_list)


def test_successive_calls_draw_new_masks_and_a_state_gives_its_bits_again():
    from mmfusion import ops
    cfg, sd, m, x = _model("tiny", 2, True)
    keys = _without_key_bias(_all_keys(cfg))
    (_, dout), _ = _douts(cfg, N, T, 51)
    a = _grads(m, x.cuda(), dout, keys)
    assert int(ops.rng_state().item()) == STATE, "a call on its own advances the state by one"
    b = _grads(m, x.cuda(), dout, keys, seed=None)
    assert int(ops.rng_state().item()) == STATE + 1
    a2 = _grads(m, x.cuda(), dout, keys)
    w = "encoder.layers.1.feed_forward.output_dense.weight"
    assert torch.equal(_bits(a[1]), _bits(a2[1])) and torch.equal(_bits(a[0][w]), _bits(a2[0][w]))
    assert torch.equal(_bits(a[0]["masked_spec_embed"]), _bits(a2[0]["masked_spec_embed"])), "the embedding's gradient is repeatable bit for bit"
    assert not torch.equal(_bits(a[1]), _bits(b[1])) and not torch.equal(_bits(a[0][w]), _bits(b[0][w]))
    before = int(ops.rng_state().item())
    with ops.dropout_state(torch.tensor([STATE - 1], dtype=torch.int64, device="cuda")) as st:
        inner = _grads(m, x.cuda(), dout, keys, seed=None)
        assert int(st.item()) == STATE
    assert int(ops.rng_state().item()) == before
    assert torch.equal(_bits(inner[1]), _bits(a[1])) and torch.equal(_bits(inner[0][w]), _bits(a[0][w]))


def test_a_forced_layerdrop_pattern_matches_the_restatement_and_the_skipped_layer_gets_nothing():
    from mmfusion import arena
    settings = dict(SETTINGS, layerdrop=0.5)
    cfg, sd, m, x = _model("tiny", 2, True, settings=settings)
    L = cfg.num_hidden_layers
    seed, skip = None, None
    for s in range(64):                                              # a generator seed whose first L draws skip layer 0 only
        g = torch.Generator().manual_seed(s)
        pattern = [bool(torch.rand([], generator=g).item() < 0.5) for _ in range(L)]
        if pattern == [True] + [False] * (L - 1):
            seed, skip = s, pattern
            break
    assert seed is not None
    keys = _all_keys(cfg)
    (tag, dout), _ = _douts(cfg, N, T, 51)
    exact, _ = _ref("tiny", cfg, sd, x, dout, False, settings, skip)
    stored, out_stored = _ref("tiny", cfg, sd, x, dout, True, settings, skip)
    ar = arena.ensure(m)
    _grads(m, x.cuda(), dout, keys)                                  # a step in which every layer may run: the weights' regions become managed
    ar.zero_grad(lazy=True)
    m.layerdrop_generator.manual_seed(seed)
    got, out = _grads(m, x.cuda(), dout, keys, zero=False)
    ar.finalize_grads()
    torch.cuda.synchronize()
    got = _hf_grads(m, keys)
    assert l2_rel(out.cpu(), out_stored) <= BOUND_A
    zero = [k_ for k_ in keys if k_.startswith("encoder.layers.0.")]
    live = [k_ for k_ in _without_key_bias(keys) if k_ not in zero]
    for k_ in zero:
        assert not bool(got[k_].any()), f"{k_} of the skipped layer received a gradient"
        assert not bool(exact[k_].any())
    _rule_b(f"NativeWav2Vec2 tiny, layer 0 skipped, {tag} dO,", _pick(got, live), _pick(exact, live), _pick(stored, live))
    _check_key_bias(m, keys)


def test_forward_and_backward_replay_from_a_captured_graph_and_layerdrop_refuses_capture():
    from mmfusion import arena, ops
    cfg, sd, m, x = _model("tiny", 2, True)
    keys = _without_key_bias(_all_keys(cfg))
    (_, dout), _ = _douts(cfg, N, T, 63)
    ar = arena.ensure(m)

    def eager_at(state):
        ar.zero_grad()
        ops.rng_state().fill_(state)
        out = m(x.cuda()).last_hidden_state
        out.backward(dout.cuda())
        torch.cuda.synchronize()
        return out.detach().clone(), _hf_grads(m, keys)
    first, later = eager_at(STATE - 1), eager_at(STATE + 1)
    static, dO = x.cuda().clone(), dout.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        m(static).last_hidden_state.backward(dO)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ops.rng_state().fill_(STATE - 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(static).last_hidden_state
        out.backward(dO)

    def replayed():
        ar.zero_grad()
        graph.replay()
        torch.cuda.synchronize()
        return out.detach().clone(), _hf_grads(m, keys)
    got = replayed()
    assert int(ops.rng_state().item()) == STATE, "the replay advances the device state"
    ops.rng_state().add_(1)
    got2 = replayed()
    assert int(ops.rng_state().item()) == STATE + 2
    for (o, g), (eo, eg) in ((got, first), (got2, later)):
        assert torch.equal(_bits(o), _bits(eo)), "a replay's result is not the eager call's at that state"
        for key in keys:
            if key.endswith(".bias") or "layer_norm" in key:            # (f32 atomics: tests/test_w2v_finetune_gpu.py's capture test)
                assert l2_rel(g[key], eg[key]) <= F32_TOL, key
            else:
                assert torch.equal(_bits(g[key]), _bits(eg[key])), key
    assert not torch.equal(_bits(got[0]), _bits(got2[0])), "every replay draws new masks"
    m.set_regularisation(layerdrop=0.1)
    refuse = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="layerdrop"):
        with torch.cuda.graph(refuse):
            m(static)
    torch.cuda.synchronize()


def test_audio_encoder_steps_with_the_regularisers_and_the_mask_embedding_moves():
    import config as cfgmod
    from mmfusion import arena, ops
    from mmfusion.train import finetune_optimizer
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=512, conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2),
                                     conv_stride=(5, 2, 2), num_conv_pos_embeddings=16)
    cfg.audio_backbone_trainable_layers = "all"
    cfg.audio_backbone_regularisation = True
    cfg.encoder_attention_weights = False
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    assert {n: getattr(enc.model.config, n) for n in R.SETTINGS_960H} == R.SETTINGS_960H
    enc.model.load_state_dict(w2v_ref.seeded_weights(enc.model.config, seed=31))
    enc = enc.cuda().train()
    wave = (0.5 * torch.randn(2, 3000, generator=torch.Generator().manual_seed(32))).cuda()
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    ops.seed_dropout(SEED)
    for _ in range(3):                                               # (LayerDrop may skip a layer in a step; three steps move every one)
        ar.zero_grad()
        feats = enc(wave)["features"]
        assert feats.requires_grad
        feats.sum().backward()
        opt.advance()
        opt.launch()
    torch.cuda.synchronize()
    assert int(ops.rng_state().item()) == STATE + 2, "under a root module the backbone must not advance the state again"
    assert not torch.equal(_bits(enc.model.masked_spec_embed.detach()), _bits(before["model.masked_spec_embed"])), "masked_spec_embed did not move"
    for n, p in enc.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if n.startswith("model.") and not p.requires_grad:
            assert torch.equal(_bits(p.detach()), _bits(before[n])), f"the frozen {n} moved"
    assert not torch.equal(_bits(enc.model.fp_w.detach()), _bits(before["model.fp_w"]))
    enc.eval()
    with torch.no_grad():
        a = enc(wave)["features"]
        b = enc(wave)["features"]
    assert torch.equal(_bits(a), _bits(b)), "eval() is deterministic: nothing regularises"
