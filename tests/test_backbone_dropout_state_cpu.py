"""CPU: the dropout state of one differentiable training call (``mmfusion.backbone._CallDropout``) and what the two backbones
that have one (``mmfusion.deberta._Drop``, ``mmfusion.wav2vec2._Reg``) add to it: which sites a call takes from ``ops.next_site()``
and in which order (1 + 4 L for DeBERTa, 3 + 4 L for Wav2Vec2), the (p, state, site, base) tuples the launches take, the shared
``join`` hooks and the two host-side helpers.  No kernel runs: the device state is stood in for by a CPU tensor, which the tuples
carry as they would carry the device one (tests/test_deberta_dropout_gpu.py and tests/test_w2v_regularise_gpu.py hold the masks
themselves to these sites, bit for bit)."""
import types

import pytest
import torch

from mmfusion import ops
from mmfusion.backbone import FrozenBackbone, _CallDropout, _check_probability
from mmfusion.deberta import _Drop
from mmfusion.wav2vec2 import _Reg

SEED = 1234 << 20                            # ops.seed_dropout(1234)


@pytest.fixture
def state(monkeypatch):
    """a CPU tensor in the device state's place, and the site counter and root depth put back afterwards"""
    st = torch.full((1,), SEED, dtype=torch.int64)
    monkeypatch.setattr(ops, "_rng_state", st)
    monkeypatch.setattr(ops, "_site", 0)
    monkeypatch.setattr(ops, "_roots", 0)
    return st


def _w2v_config(**kw):
    c = dict(hidden_dropout=0.1, attention_dropout=0.2, activation_dropout=0.3, feat_proj_dropout=0.4, layerdrop=0.0, mask_time_prob=0.0,
             mask_time_length=10, mask_time_min_masks=2, num_attention_heads=4, num_hidden_layers=2)
    return types.SimpleNamespace(**{**c, **kw})


def test_deberta_call_takes_the_embeddings_site_then_four_per_layer(state):
    ops.begin_training_forward()
    d = _Drop(0.1, 0.2, 2)
    assert isinstance(d, _CallDropout)
    assert d.emb == 1 and d.layers == [(2, 3, 4, 5), (6, 7, 8, 9)]
    assert (_Drop.REL, _Drop.PROBS, _Drop.OUT, _Drop.MLP) == (0, 1, 2, 3)
    assert ops.next_site() == 10                                   # 1 + 4 L sites were taken, no more
    assert int(state.item()) == SEED + 1
    p, st, site, base = d.hidden(d.emb, 5)
    assert (p, site, base) == (0.1, 1, 5) and st is state            # the live state, not a copy
    assert d.hidden(d.layers[1][_Drop.REL], 0)[1:] == (state, 6, 0)
    p, st, site, base = d.probs(1, 3)
    assert (p, site, base) == (0.2, 7, 3) and st is state            # the item base: the kernel multiplies by H itself
    assert d.join_sites(0) == (4, 5) and d.join_sites(1) == (8, 9)
    assert _Drop(0.1, 0.0, 1).probs(0, 3) is None


def test_wav2vec2_call_takes_three_leading_sites_then_four_per_layer(state):
    ops.begin_training_forward()
    skip = [False, True]
    r = _Reg(_w2v_config(), 3, 24, torch.device("cpu"), skip)
    assert isinstance(r, _CallDropout)
    assert (r.fp, r.mask, r.enc) == (1, 2, 3) and r.layers == [(4, 5, 6, 7), (8, 9, 10, 11)]
    assert (_Reg.PROBS, _Reg.OUT, _Reg.ACT, _Reg.MLP) == (0, 1, 2, 3)
    assert ops.next_site() == 12                                   # a layer LayerDrop skips still owns its four sites
    assert r.starts is None and r.spans(0, 2) is None and r.skip is skip and r.front        # (front: the projection's dropout is on)
    assert r.hidden(r.enc, 2) == (0.1, state, 3, 2)
    assert r.feat_proj(2) == (0.4, state, 1, 2)
    assert r.probs(1, 3) == (0.2, state, 8, 3 * 4)                 # the stream base: item0 * H
    assert r.act(0, 3) == (0.3, state, 6, 3)
    assert r.join_sites(0) == (5, 7) and r.join_sites(1) == (9, 11)
    off = _Reg(_w2v_config(attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0), 3, 24, torch.device("cpu"), skip)
    assert off.probs(0, 3) is None and off.act(0, 3) is None and not off.front


def test_hidden_joins_are_none_without_hidden_dropout_and_launch_at_the_two_sites(state, monkeypatch):
    from mmfusion import lib
    ops.begin_training_forward()
    assert FrozenBackbone._hidden_joins(None, None, 2, 0) == (None, None)
    assert FrozenBackbone._hidden_joins(_Drop(0.0, 0.1, 2), (4, 5), 2, 0) == (None, None)
    calls = []
    monkeypatch.setattr(lib, "hidden_dropout", lambda y, out, items, drop, resid=None: calls.append((y, out, items, drop, resid)))
    d = _Drop(0.25, 0.0, 2)
    join, join_bwd = FrozenBackbone._hidden_joins(d, d.join_sites(1), 2, 6)
    join("o", "y", "x")
    join("fc2", "y", "ln")
    join_bwd("fc2", "dy", "out")
    o, m = d.layers[1][_Drop.OUT], d.layers[1][_Drop.MLP]
    assert calls == [("y", "y", 2, (0.25, state, o, 6), "x"), ("y", "y", 2, (0.25, state, m, 6), "ln"), ("dy", "out", 2, (0.25, state, m, 6), None)]


def test_a_call_on_its_own_starts_a_training_forward_and_one_under_a_root_does_not(state):
    ops.begin_training_forward()
    assert ops.next_site() == 1 and ops.next_site() == 2
    FrozenBackbone._own_training_forward()                         # on its own: new masks, sites from 1
    assert int(state.item()) == SEED + 2 and ops.next_site() == 1
    ops.root_entered()
    try:
        FrozenBackbone._own_training_forward()                     # under a root's forward: its numbering goes on
        assert int(state.item()) == SEED + 2 and ops.next_site() == 2
    finally:
        ops.root_left()


def test_the_models_calls_go_through_it(state):
    import deberta_ref
    from test_deberta_cpu import _native
    m = _native(deberta_ref.tiny_config(), hidden_dropout_prob=0.1).train()
    L = m.config.num_hidden_layers
    d = m._drop_of_call()
    assert int(state.item()) == SEED + 1 and d.emb == 1 and d.layers[-1][-1] == 1 + 4 * L and d.probs(0, 0) is None
    m.eval()
    assert m._drop_of_call() is None and int(state.item()) == SEED + 1


def test_check_probability():
    for ok in (0, 0.0, 0.5, 0.999):
        _check_probability("M: set", "p", ok)
    _check_probability("M: set", "p", 1.0, closed=True)
    for bad in (1.0, -0.1, float("nan"), "0.1", True, None):
        with pytest.raises(ValueError, match=r"M: set\(p=.*\): a probability in \[0, 1\)$"):
            _check_probability("M: set", "p", bad)
    for bad in (1.5, -0.1, float("nan"), False):
        with pytest.raises(ValueError, match=r"M: set\(p=.*\): a probability in \[0, 1\]$"):
            _check_probability("M: set", "p", bad, closed=True)
