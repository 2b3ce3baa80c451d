"""CPU: the training-mode restatement tests/deberta_dropout_ref.py against tests/deberta_ref.py (all-ones masks) and against a
live HuggingFace ``DebertaV2Model`` in ``train()`` whose ``nn.Dropout`` modules are made to apply the restated masks (which pins
the five sites, their order and the per-layer ``pos_dropout``); the statistics of the restated masks; and the argument checks
of ``NativeDeberta.set_dropout`` / ``config.text_backbone_dropout`` that need no GPU.

The GPU tests (tests/test_deberta_dropout_kernels_gpu.py, tests/test_deberta_dropout_gpu.py) hold the kernels to these masks bit
for bit, so the statistics are checked here, on the host restatement."""
import math

import numpy as np
import pytest
import torch

import attn_ref
import deberta_dropout_ref as D
import deberta_ref
from helpers import l2_rel
from test_deberta_cpu import RESTATE_TOL, _golden, _native

STATE = (1234 << 20) + 1                     # ops.seed_dropout(1234), then one begin_training_forward


def test_all_ones_masks_give_the_inference_restatement_exactly():
    cfg, sd, ids, mask, _, _ = _golden()
    N, T = ids.shape
    want = deberta_ref.deberta_forward(sd, ids, mask, cfg)
    got = D.deberta_forward(sd, ids, mask, cfg, D.ones_masks(cfg, N, T))
    assert torch.equal(got, want)
    # sites switched off (threshold 0: None masks) leave deberta_ref's rounding points alone, so the storage model is its too
    off = D.call_masks(STATE, D.sites(cfg.num_hidden_layers), cfg, N, T, 0.0, 0.0)
    assert off.emb is None and off.probs[0] is None and off.c_h == 1.0
    assert torch.equal(D.deberta_forward(sd, ids, mask, cfg, off, bf16_storage=True), deberta_ref.deberta_forward(sd, ids, mask, cfg, bf16_storage=True))


def test_restatement_against_huggingface_in_train_mode_with_the_restated_masks():
    """every nn.Dropout of a live DebertaV2Model in train() returns input * restated mask * c; the hooks fire in the order the
    sites are numbered, once each"""
    from transformers import DebertaV2Config, DebertaV2Model
    cfg, sd, ids, mask, _, _ = _golden()
    N, T = ids.shape
    L, p_h, p_a = cfg.num_hidden_layers, 0.1, 0.1
    st = D.sites(L)
    masks = D.call_masks(STATE, st, cfg, N, T, p_h, p_a)
    hf = DebertaV2Model(DebertaV2Config(**dict(deberta_ref.hf_config_kwargs(cfg), hidden_dropout_prob=p_h, attention_probs_dropout_prob=p_a)))
    hf.load_state_dict(sd)
    hf.train()
    plan = {"embeddings.dropout": (st.emb, masks.emb, masks.c_h)}
    for i in range(L):
        a = f"encoder.layer.{i}."
        plan[a + "attention.self.pos_dropout"] = (st.rel[i], masks.rel[i], masks.c_h)
        plan[a + "attention.self.dropout"] = (st.probs[i], masks.probs[i], masks.c_a)
        plan[a + "attention.output.dropout"] = (st.out[i], masks.out[i], masks.c_h)
        plan[a + "output.dropout"] = (st.mlp[i], masks.mlp[i], masks.c_h)
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
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask).last_hidden_state
    assert fired == list(range(1, 2 + 4 * L)), fired
    got = D.deberta_forward(sd, ids, mask, cfg, masks)
    plain = deberta_ref.deberta_forward(sd, ids, mask, cfg)
    err = l2_rel(got, want.double())
    print(f"training-mode restatement vs HuggingFace train() under the restated masks: {err:.3e} (bound {RESTATE_TOL}); "
          f"the inference restatement is {l2_rel(plain, want.double()):.3e} away")
    assert err <= RESTATE_TOL
    assert l2_rel(plain, want.double()) > 100 * RESTATE_TOL
    # a mask moved to the neighbouring layer is seen: the per-layer pos_dropout is per layer
    swapped = D.call_masks(STATE, st, cfg, N, T, p_h, p_a)
    swapped.rel[0], swapped.rel[1] = swapped.rel[1], swapped.rel[0]
    assert l2_rel(D.deberta_forward(sd, ids, mask, cfg, swapped), want.double()) > 100 * RESTATE_TOL


def _rate_ok(keep, p=0.1):
    n = keep.numel()
    rate = float(keep.double().mean())
    sd = math.sqrt(p * (1.0 - p) / n)
    return n, rate, abs(rate - (1.0 - p)) / sd


def test_restated_masks_keep_rate_and_independence():
    """>= 1e5 draws per site at p = 0.1: the keep-rate within 5 binomial standard deviations of 0.9; masks of different sites,
    layers, items and heads differ (and agree no more often than independent ones would: 0.82 +- 5 sd)"""
    cfg = deberta_ref.tiny_config()
    N, T, H, d = 3, 24, cfg.num_attention_heads, cfg.hidden_size
    L = cfg.num_hidden_layers
    st = D.sites(L)
    m = D.call_masks(STATE, st, cfg, N, T, 0.1, 0.1)
    big = D.probs_keep(STATE, st.probs[0], 0, 2, H, 128, attn_ref.mmf_drop_thresh(0.1))          # 2 x 4 x 128 x 128 = 131072 draws
    named = [("emb", torch.cat([m.emb.reshape(-1), D.hidden_keep(STATE, st.emb, 3, 15, T * d, attn_ref.mmf_drop_thresh(0.1)).reshape(-1)])),
             ("probs", big)]
    for i in range(L):
        more = D.hidden_keep(STATE, st.rel[i], 1, 30, 16 * d, attn_ref.mmf_drop_thresh(0.1))      # further sub-streams of the rel site
        named += [(f"rel[{i}]", torch.cat([m.rel[i].reshape(-1), more.reshape(-1)])),
                  (f"out[{i}]", torch.cat([m.out[i].reshape(-1), D.hidden_keep(STATE, st.out[i], 3, 15, T * d, attn_ref.mmf_drop_thresh(0.1)).reshape(-1)])),
                  (f"mlp[{i}]", torch.cat([m.mlp[i].reshape(-1), D.hidden_keep(STATE, st.mlp[i], 3, 15, T * d, attn_ref.mmf_drop_thresh(0.1)).reshape(-1)]))]
    for name, keep in named:
        n, rate, z = _rate_ok(keep)
        print(f"keep-rate of {name}: {rate:.5f} over {n} draws ({z:.2f} sd from 0.9)")
        assert n >= 100000 and z <= 5.0, (name, n, rate, z)

    def differ(a, b, what):
        agree = (a == b).double()
        n = agree.numel()
        indep = 0.9 * 0.9 + 0.1 * 0.1
        z = abs(float(agree.mean()) - indep) / math.sqrt(indep * (1 - indep) / n)
        assert not torch.equal(a, b) and z <= 5.0, (what, float(agree.mean()), z)
    differ(m.emb, m.out[0], "sites")
    differ(m.out[0], m.mlp[0], "sites of one layer")
    differ(m.out[0], m.out[1], "layers")
    differ(m.rel[0], m.rel[1], "the layers' relative embeddings")
    differ(m.emb[0], m.emb[1], "items")
    differ(m.probs[0][0], m.probs[0][1], "items of the attention")
    differ(m.probs[0][:, 0], m.probs[0][:, 1], "heads")
    differ(m.probs[0], m.probs[1], "layers of the attention")
    other = D.call_masks(STATE + 1, st, cfg, N, T, 0.1, 0.1)
    differ(m.emb, other.emb, "steps")
    # keyed by the element: items 1 .. 2 drawn as a chunk of their own are the batch's items 1 .. 2
    th = attn_ref.mmf_drop_thresh(0.1)
    assert torch.equal(D.hidden_keep(STATE, st.emb, 1, 2, T * d, th).reshape(2, T, d), m.emb[1:])
    assert torch.equal(D.probs_keep(STATE, st.probs[1], 1, 2, H, T, th), m.probs[1][1:])
    assert D.sites(L, first=7).emb == 7 and D.sites(L).mlp[-1] == 1 + 4 * L


def test_threshold_and_factor_are_the_projects():
    assert attn_ref.mmf_drop_thresh(0.0) == 0 and attn_ref.inv_keep_of(0) == 1.0
    th = attn_ref.mmf_drop_thresh(0.5)
    assert th == 1 << 31 and attn_ref.inv_keep_of(th) == 2.0
    assert abs(attn_ref.inv_keep_of(attn_ref.mmf_drop_thresh(0.1)) - 1.0 / 0.9) < 1e-6


# ---- argument checks ---------------------------------------------------------------------------------------------
def test_set_dropout_and_constructor_arguments():
    cfg = deberta_ref.tiny_config()
    m = _native(cfg)
    assert m.training and (m.config.hidden_dropout_prob, m.config.attention_probs_dropout_prob) == (0.0, 0.0)   # off by default
    m = _native(cfg, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.2)
    assert (m.config.hidden_dropout_prob, m.config.attention_probs_dropout_prob) == (0.1, 0.2)
    m.set_dropout(0.3, 0.0)
    assert (m.config.hidden_dropout_prob, m.config.attention_probs_dropout_prob) == (0.3, 0.0)
    m.set_dropout()
    assert (m.config.hidden_dropout_prob, m.config.attention_probs_dropout_prob) == (0.0, 0.0)
    for bad in ((1.0, 0.0), (0.0, 1.0), (-0.1, 0.0), (0.0, float("nan")), ("0.1", 0.0), (True, 0.0), (None, 0.0)):
        with pytest.raises(ValueError, match="set_dropout"):
            m.set_dropout(*bad)
        with pytest.raises(ValueError, match="set_dropout"):
            _native(cfg, hidden_dropout_prob=bad[0], attention_probs_dropout_prob=bad[1])
    assert (m.config.hidden_dropout_prob, m.config.attention_probs_dropout_prob) == (0.0, 0.0)                 # a refused call changes nothing
    # the state_dict surface does not know about dropout
    assert list(m.state_dict()) == list(deberta_ref.hf_keys(cfg))


def test_text_encoder_reads_text_backbone_dropout():
    import config as cfgmod
    from models.encoders import TextEncoder
    tcfg = deberta_ref.tiny_config()

    def build(**extra):
        cfg = cfgmod.ModelConfig()
        cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
        cfg.text_backbone = "native"
        cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
        for k, v in extra.items():
            setattr(cfg, k, v)
        return TextEncoder(cfg)
    probs = lambda enc: (enc.model.config.hidden_dropout_prob, enc.model.config.attention_probs_dropout_prob)
    assert probs(build()) == (0.0, 0.0)
    assert probs(build(text_backbone_dropout=0)) == (0.0, 0.0)
    assert probs(build(text_backbone_dropout=True)) == (0.1, 0.1)
    assert probs(build(text_backbone_dropout=(0.2, 0.05))) == (0.2, 0.05)
    for bad in (0.1, "on", (0.1,), (0.1, 1.0), (0.1, 0.1, 0.1)):
        with pytest.raises(ValueError, match="text_backbone_dropout|set_dropout"):
            build(text_backbone_dropout=bad)
    enc = build(text_backbone_dropout=True, text_backbone_trainable_layers=1)
    assert enc.model.training and enc.model.trainable_layers == 1
    enc.eval()
    assert not enc.model.training                      # .eval() / .train() reach the backbone as any submodule
    enc.train()
    assert enc.model.training


def test_wrapper_refuses_cpu_tensors():
    from mmfusion import lib
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.hidden_dropout(x, x, 2, (0.1, None, 1, 0))
