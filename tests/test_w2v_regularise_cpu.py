"""CPU: the training-mode restatement tests/w2v_regularise_ref.py against tests/w2v_ref.py (all-ones masks) and against a live
HuggingFace ``Wav2Vec2Model`` in ``train()`` whose dropouts, span draw and layer-skip draws are made to apply the restated masks
(which pins the 3 + 4 L sites and their order); the statistics of the restated masks and of the restated span draw against
HuggingFace's own ``_compute_mask_indices``; and the argument checks of ``NativeWav2Vec2.set_regularisation`` /
``config.audio_backbone_regularisation`` that need no GPU.

The GPU tests (tests/test_w2v_regularise_kernels_gpu.py, tests/test_w2v_regularise_gpu.py) hold the kernels to these masks bit for
bit, so the statistics are checked here, on the host restatement."""
import math

import numpy as np
import pytest
import torch

import attn_ref
import w2v_ref
import w2v_regularise_ref as R
from helpers import l2_rel
from test_w2v_cpu import RESTATE_TOL, _native

STATE = (1234 << 20) + 1                     # ops.seed_dropout(1234), then one begin_training_forward
SETTINGS = dict(R.SETTINGS_960H, mask_time_prob=0.2)          # (0.05 at T = 199 draws the minimum of 2 spans; 0.2 draws 3 or 4)


def _case(L=4000, seed=5):
    cfg = w2v_ref.tiny_config()
    sd = w2v_ref.seeded_weights(cfg, seed=seed)
    x = 0.5 * torch.randn(2, L, generator=torch.Generator().manual_seed(seed + 1)) + 0.05
    return cfg, sd, x


def test_all_ones_masks_give_the_inference_restatement_exactly():
    cfg, sd, x = _case()
    T = w2v_ref.w2v_forward(sd, x, cfg).shape[1]
    want = w2v_ref.w2v_forward(sd, x, cfg)
    got = R.w2v_forward(sd, x, cfg, R.ones_masks(cfg, 2, T), skip=[False] * cfg.num_hidden_layers)
    assert torch.equal(got, want)
    off = R.call_masks(STATE, R.sites(cfg.num_hidden_layers), cfg, 2, T, {})
    assert off.fp is None and off.spans is None and off.probs[0] is None and off.act[1] is None and off.c_h == 1.0
    assert torch.equal(R.w2v_forward(sd, x, cfg, off, bf16_storage=True), w2v_ref.w2v_forward(sd, x, cfg, bf16_storage=True))
    # a skipped layer is the identity: skipping every layer leaves the encoder LayerNorm's output
    one = R.w2v_forward(sd, x, cfg, off, skip=[False, True])
    assert not torch.equal(one, want) and one.shape == want.shape


def test_restatement_against_huggingface_in_train_mode_with_the_restated_masks(monkeypatch):
    """every dropout of a live Wav2Vec2Model in train() (eager attention) returns input * restated mask * c, ``_compute_mask_indices``
    returns the restated spans and the layer-skip draws are forced; the hooks fire in the order the sites are numbered, once each"""
    transformers = pytest.importorskip("transformers")
    from transformers.models.wav2vec2 import modeling_wav2vec2 as M
    cfg, sd, x = _case()
    L, N = cfg.num_hidden_layers, x.shape[0]
    T = w2v_ref.w2v_forward(sd, x, cfg).shape[1]
    st = R.sites(L)
    masks = R.call_masks(STATE, st, cfg, N, T, SETTINGS)
    assert masks.spans.any() and not masks.spans.all()
    kw = dict(w2v_ref.config_kwargs(cfg), hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1,
              layerdrop=0.1, apply_spec_augment=True, mask_time_prob=0.2, mask_time_length=10, mask_time_min_masks=2, mask_feature_prob=0.0,
              attn_implementation="eager")
    hf = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**kw))
    hf.load_state_dict(sd)
    hf.train()
    plan = {"feature_projection.dropout": (st.fp, masks.fp, masks.c_fp), "encoder.dropout": (st.enc, masks.enc, masks.c_h)}
    for i in range(L):
        a = f"encoder.layers.{i}."
        plan[a + "dropout"] = (st.out[i], masks.out[i], masks.c_h)
        plan[a + "feed_forward.intermediate_dropout"] = (st.act[i], masks.act[i], masks.c_act)
        plan[a + "feed_forward.output_dropout"] = (st.mlp[i], masks.mlp[i], masks.c_h)
    drops = {name: mod for name, mod in hf.named_modules() if isinstance(mod, torch.nn.Dropout)}
    assert set(drops) == set(plan), set(drops) ^ set(plan)
    fired = []

    def hook_for(name):
        site, keep, c = plan[name]

        def hook(module, inputs, output):
            assert module.training and inputs[0].numel() == keep.numel(), (name, tuple(inputs[0].shape), tuple(keep.shape))
            fired.append(site)
            return inputs[0] * (keep.reshape(inputs[0].shape).to(inputs[0].dtype) * c)
        return hook
    for name, mod in drops.items():
        mod.register_forward_hook(hook_for(name))
    plain_dropout, layer = torch.nn.functional.dropout, [0]

    def functional_dropout(t, p=0.5, training=True, inplace=False):
        if t.dim() == 4 and training:                                 # the attention's probabilities (N, H, T, T), layer by layer
            i = layer[0]
            layer[0] += 1
            fired.append(st.probs[i])
            assert tuple(t.shape) == tuple(masks.probs[i].shape)
            return t * (masks.probs[i].to(t.dtype) * masks.c_a)
        return plain_dropout(t, p, training, inplace)
    monkeypatch.setattr(torch.nn.functional, "dropout", functional_dropout)

    def spans(shape, mask_prob, mask_length, attention_mask=None, min_masks=0):
        assert tuple(shape) == (N, T) and (mask_prob, mask_length, min_masks) == (0.2, 10, 2) and attention_mask is None
        fired.append(st.spans)
        return masks.spans.numpy()
    monkeypatch.setattr(M, "_compute_mask_indices", spans)
    draws = iter([0.5] * L)                                           # no layer skipped: every draw is above layerdrop
    plain_rand = torch.rand
    monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.tensor(next(draws)) if a == ([],) else plain_rand(*a, **k))
    with torch.no_grad():
        want = hf(x).last_hidden_state
    assert fired == list(range(1, 4 + 4 * L)), fired
    got = R.w2v_forward(sd, x, cfg, masks)
    plain = w2v_ref.w2v_forward(sd, x, cfg)
    err = l2_rel(got, want.double())
    print(f"training-mode restatement vs HuggingFace train() under the restated masks: {err:.3e} (bound {RESTATE_TOL}); "
          f"the inference restatement is {l2_rel(plain, want.double()):.3e} away")
    assert err <= RESTATE_TOL
    assert l2_rel(plain, want.double()) > 100 * RESTATE_TOL
    # one layer's masks moved to its neighbour are seen, site kind by site kind
    for kind in ("probs", "out", "act", "mlp"):
        swapped = R.call_masks(STATE, st, cfg, N, T, SETTINGS)
        lst = getattr(swapped, kind)
        lst[0], lst[1] = lst[1], lst[0]
        assert l2_rel(R.w2v_forward(sd, x, cfg, swapped), want.double()) > 100 * RESTATE_TOL, kind
    # a forced skip of layer 0: HuggingFace's layer loop under draws (0.05, 0.5) against skip = [True, False]
    layer[0], draws = 1, iter([0.05, 0.5])                            # (the skipped layer's probabilities are never dropped: its site idles)
    fired.clear()
    with torch.no_grad():
        want_skip = hf(x).last_hidden_state
    assert st.probs[0] not in fired and st.out[0] not in fired and st.probs[1] in fired
    got_skip = R.w2v_forward(sd, x, cfg, masks, skip=[True, False])
    assert l2_rel(got_skip, want_skip.double()) <= RESTATE_TOL
    assert l2_rel(got, want_skip.double()) > 100 * RESTATE_TOL


def test_restated_masks_keep_rate_and_chunk_independence():
    """>= 1e5 draws per site kind at p = 0.1: the keep-rate within 5 binomial standard deviations of 0.9; a chunk's masks are the
    batch's"""
    cfg = w2v_ref.tiny_config()
    N, T, H, d, I, L = 3, 60, cfg.num_attention_heads, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    st = R.sites(L)
    m = R.call_masks(STATE, st, cfg, N, T, R.SETTINGS_960H)
    th = attn_ref.mmf_drop_thresh(0.1)
    named = [("fp", torch.cat([m.fp.reshape(-1), R.hidden_keep(STATE, st.fp, 3, 5, T * d, th).reshape(-1)])),
             ("enc", torch.cat([m.enc.reshape(-1), R.hidden_keep(STATE, st.enc, 3, 5, T * d, th).reshape(-1)])),
             ("probs", R.probs_keep(STATE, st.probs[0], 0, 2, H, 128, th)), ("act", torch.cat([a.reshape(-1) for a in m.act])),
             ("out", torch.cat([a.reshape(-1) for a in m.out] + [R.hidden_keep(STATE, st.out[0], 3, 3, T * d, th).reshape(-1)])),
             ("mlp", torch.cat([a.reshape(-1) for a in m.mlp] + [R.hidden_keep(STATE, st.mlp[0], 3, 3, T * d, th).reshape(-1)]))]
    for name, keep in named:
        n, rate = keep.numel(), float(keep.double().mean())
        z = abs(rate - 0.9) / math.sqrt(0.1 * 0.9 / n)
        print(f"keep-rate of {name}: {rate:.5f} over {n} draws ({z:.2f} sd from 0.9)")
        assert n >= 100000 and z <= 5.0, (name, n, rate, z)
    for a, b, what in ((m.fp, m.enc, "sites"), (m.out[0], m.out[1], "layers"), (m.act[0][0], m.act[0][1], "clips"),
                       (m.probs[0][:, 0], m.probs[0][:, 1], "heads"), (m.out[0], m.mlp[0], "sites of a layer")):
        assert not torch.equal(a, b), what
    assert torch.equal(R.hidden_keep(STATE, st.act[1], 1, 2, T * I, th).reshape(2, T, I), m.act[1][1:])
    assert torch.equal(R.probs_keep(STATE, st.probs[1], 1, 2, H, T, th), m.probs[1][1:])
    table = R.span_table(STATE, st.spans, 0, N, T, 0.05, 10, 2, 2)
    assert torch.equal(R.span_table(STATE, st.spans, 1, 2, T, 0.05, 10, 2, 2), table[1:])
    assert R.sites(L, first=7).fp == 7 and R.sites(L).mlp[-1] == 3 + 4 * L


@pytest.mark.parametrize("prob,min_masks", [(0.2, 0), (0.05, 2)])
def test_restated_span_draw_against_huggingfaces(prob, min_masks):
    """T = 149, length 10, 3000 clips: the span count takes only the values the rule allows, the upper one with frequency
    frac(prob T / length) within 5 standard errors; the starts are distinct and in range; the mean masked fraction agrees with a
    sample of HuggingFace's own ``_compute_mask_indices`` within 5 standard errors of the difference"""
    M = pytest.importorskip("transformers.models.wav2vec2.modeling_wav2vec2")
    T, length, clips = 149, 10, 3000
    e = prob * T / length
    n0, frac = int(e), e - int(e)
    lo, hi = R.span_count(n0, T, length, min_masks), R.span_count(n0 + 1, T, length, min_masks)
    counts, fracs = [], []
    for c in range(clips):
        s = R.span_starts(STATE, 2, c, T, prob, length, min_masks)
        assert len(set(s)) == len(s) and all(0 <= v <= T - length for v in s), s
        assert len(s) in (lo, hi)
        counts.append(len(s))
        row = np.zeros(T, dtype=bool)
        for v in s:
            row[v:v + length] = True
        fracs.append(row.mean())
    if hi != lo:
        up = sum(c == hi for c in counts) / clips
        se = math.sqrt(frac * (1 - frac) / clips)
        print(f"prob {prob}: {hi} spans in {up:.4f} of the clips, frac(e) = {frac:.4f} ({abs(up - frac) / se:.2f} se)")
        assert abs(up - frac) <= 5 * se
    np.random.seed(7)
    theirs = M._compute_mask_indices((clips, T), prob, length, min_masks=min_masks).mean(axis=1)
    ours = np.asarray(fracs)
    se = math.sqrt(ours.var(ddof=1) / clips + theirs.var(ddof=1) / clips)
    print(f"prob {prob}, min {min_masks}: masked fraction {ours.mean():.5f} here, {theirs.mean():.5f} HuggingFace ({abs(ours.mean() - theirs.mean()) / se:.2f} se)")
    assert abs(ours.mean() - theirs.mean()) <= 5 * se
    # the other clips of a batch, other states and other sites draw other spans
    assert R.span_starts(STATE, 2, 0, T, prob, length, min_masks) != R.span_starts(STATE, 2, 1, T, prob, length, min_masks)
    assert R.span_starts(STATE, 2, 0, T, prob, length, min_masks) != R.span_starts(STATE + 1, 2, 0, T, prob, length, min_masks)


def test_span_draw_edges():
    """length == T leaves one start; a count above the room is capped and the starts stay distinct (the redraw / probe path)"""
    assert R.span_starts(STATE, 2, 0, 10, 0.5, 10, 2) == [0]
    s = R.span_starts(STATE, 2, 0, 11, 1.0, 10, 0)                  # e = 1.1 -> 1 or 2 spans; 2 * 10 > 11 -> 1
    assert len(s) == 1 and s[0] in (0, 1)
    s = R.span_starts(STATE, 2, 3, 12, 1.0, 1, 0)                   # 12 spans of length 1 in 12 places: every place once
    assert sorted(s) == list(range(12))


# ---- argument checks ---------------------------------------------------------------------------------------------
def test_set_regularisation_and_constructor_arguments():
    cfg = w2v_ref.tiny_config()
    m = _native(cfg)
    c = m.config
    assert all(getattr(c, n) == 0.0 for n in R.SETTINGS_960H if n not in ("mask_time_length", "mask_time_min_masks"))
    assert (c.mask_time_length, c.mask_time_min_masks, c.apply_spec_augment, c.mask_feature_prob) == (10, 2, False, 0.0)
    m = _native(cfg, **R.SETTINGS_960H)
    assert {n: getattr(m.config, n) for n in R.SETTINGS_960H} == R.SETTINGS_960H and m.config.apply_spec_augment
    m.set_regularisation(hidden_dropout=0.3, mask_time_prob=0.0)
    assert m.config.hidden_dropout == 0.3 and m.config.attention_dropout == 0.1 and not m.config.apply_spec_augment
    for bad in (dict(hidden_dropout=1.0), dict(attention_dropout=-0.1), dict(layerdrop=float("nan")), dict(feat_proj_dropout="0.1"),
                dict(activation_dropout=True), dict(mask_time_prob=1.5), dict(mask_time_length=0), dict(mask_time_length=2.5),
                dict(mask_time_min_masks=-1), dict(mask_channel_prob=0.1)):
        with pytest.raises(ValueError, match="set_regularisation"):
            m.set_regularisation(**bad)
        with pytest.raises((ValueError, TypeError)):
            _native(cfg, **bad)
    assert m.config.hidden_dropout == 0.3                                          # a refused call changes nothing
    with pytest.raises(ValueError, match="not built"):
        _native(cfg, mask_feature_prob=0.1)
    with pytest.raises(ValueError, match="not built"):
        m.set_regularisation(mask_feature_prob=0.1)
    assert list(m.state_dict()) == list(w2v_ref.hf_keys(cfg))                      # the state_dict surface does not know about them


def test_masked_spec_embed_trains_with_the_front_end_and_the_mask_only():
    cfg = w2v_ref.tiny_config()
    m = _native(cfg)
    L = cfg.num_hidden_layers
    m.set_trainable_layers(L, front=True)
    assert not m.masked_spec_embed.requires_grad
    m.set_regularisation(mask_time_prob=0.05)
    assert m.masked_spec_embed.requires_grad and "masked_spec_embed" in m._trainable_names()
    m.set_trainable_layers(L)
    assert not m.masked_spec_embed.requires_grad
    m.set_trainable_layers(L, front=True)
    assert m.masked_spec_embed.requires_grad
    m.set_regularisation(mask_time_prob=0.0)
    assert not m.masked_spec_embed.requires_grad and m.fp_w.requires_grad


def test_a_mask_longer_than_the_clip_is_refused_on_the_host():
    cfg = w2v_ref.tiny_config()
    m = _native(cfg, mask_time_prob=0.05, mask_time_length=10).train()
    m.set_trainable_layers(1)
    with pytest.raises(ValueError, match="longer than the clip"):
        m._reg_of_call(2, 9, torch.device("cpu"))
    m.eval()
    assert m._reg_of_call(2, 9, torch.device("cpu")) is None                       # nothing acts outside train()
    from mmfusion.wav2vec2 import span_count, span_slots
    for T, prob, length, mn in ((149, 0.2, 10, 0), (149, 0.05, 10, 2), (10, 0.5, 10, 2), (11, 1.0, 10, 0), (12, 1.0, 1, 0)):
        assert span_count(7, T, length, mn) == R.span_count(7, T, length, mn)
        assert span_slots(T, prob, length, mn) == max(1, R.span_count(int(prob * T / length) + 1, T, length, mn))


def test_audio_encoder_reads_audio_backbone_regularisation():
    import config as cfgmod
    from models.encoders import AudioEncoder

    def build(**extra):
        cfg = cfgmod.ModelConfig()
        cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768
        cfg.audio_backbone = "native"
        cfg.audio_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=512, conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2),
                                         conv_stride=(5, 2, 2), num_conv_pos_embeddings=16)
        for k, v in extra.items():
            setattr(cfg, k, v)
        return AudioEncoder(cfg)
    got = lambda enc: {n: getattr(enc.model.config, n) for n in R.SETTINGS_960H}
    off = dict(R.SETTINGS_960H, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0,
               mask_time_prob=0.0)
    assert got(build()) == off and got(build(audio_backbone_regularisation=0)) == off
    assert got(build(audio_backbone_regularisation=True)) == R.SETTINGS_960H
    assert got(build(audio_backbone_regularisation=dict(hidden_dropout=0.2, layerdrop=0.05))) == dict(off, hidden_dropout=0.2, layerdrop=0.05)
    for bad in (0.1, "on", (0.1, 0.1), {}, dict(hidden_dropout=1.0), dict(mask_feature_prob=0.1), dict(dropout=0.1)):
        with pytest.raises(ValueError, match="audio_backbone_regularisation|set_regularisation"):
            build(audio_backbone_regularisation=bad)
    enc = build(audio_backbone_regularisation=True, audio_backbone_trainable_layers="all")
    assert enc.model.trainable_front and enc.model.masked_spec_embed.requires_grad
    enc.eval()
    assert not enc.model.training


def test_wrappers_refuse_cpu_tensors():
    from mmfusion import lib
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.w2v_mask_drop(x, x, 2, 2, 10, (0.1, None, 1, 0))
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.bias_gelu_drop_to(x, torch.zeros(64), x, 2, (0.1, None, 1, 0))
