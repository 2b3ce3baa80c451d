"""GPU: the whole model on its three native backbones, seam by seam (tests/native_model_cases.py has the shapes).

Every native backbone is held to float64 on its own and inside its own encoder, and the fusion side is held to the oracle on
feature inputs.  What this file pins is the composition: a ``MultimodalEmotionModel`` (and its Robust / FewShot / distillation
wrappers) with ``config.<kind>_backbone = "native"`` for all three kinds, in ONE parameter arena with ONE dropout site counter.

Method (the rule of tests/test_mult_fused_seams_gpu.py): the whole model against a composition of pieces that are each pinned
already, on identical bits:

  * the stand-alone encoders and backbones: deep copies of the whole model's, made before it had an arena, so each lives in an
    arena of its own; they get the whole model's inputs, and the backbones the gradient that arrived at the whole model's backbone
    output (a tensor hook);
  * the twin: the same model with ``feature_inputs = True`` and the whole model's non-backbone ``state_dict``, fed the backbones'
    outputs (``TextEncoder`` pools row 0 on feature inputs and behind a backbone whose ``model_type`` contains "bert", which
    "deberta-v2" does: the twin's text input is the backbone's whole output).

The launches are the same on the same bits, so no tolerance is introduced: equality of bits wherever an element has one writer,
and the existing ``F32_TOL`` (relative L2) for what float atomics accumulate in an order that differs between two runs of even the
same call (bias column sums, LayerNorm dgamma / dbeta, the GAT and adaptive-combine vectors, the InfoNCE
value).  ``_atomic`` is that list by shape: every parameter that is not a 2-D matrix.  The measured ratios are the SEAM lines
(profiles/native_model_seams.txt is those lines from an MI355X)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import native_model_cases as cases  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402
from test_deberta_finetune_gpu import _frozen_grads_are_empty  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402

KINDS = cases.KINDS
HEADS = ("emotion_logits", "valence", "arousal", "uncertainty")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
class Taps:
    """Records every call of a whole model's three backbones, in call order per kind: the arguments, the output, the gradient
    that arrives at the output (a tensor hook) and the dropout site counter on entry and on return."""

    def __init__(self, model):
        self.bb = cases.backbones(model)
        self.calls = {kind: [] for kind in KINDS}
        self.order = []
        self._undo = []

    def _record(self, kind, args, kwargs, out, site0):
        from mmfusion import ops
        rec = {"args": args, "kwargs": kwargs, "out": out, "grad": None, "site0": site0, "site1": ops._site}
        if out.requires_grad:
            out.register_hook(lambda g, rec=rec: rec.__setitem__("grad", g.detach().clone()))
        self.calls[kind].append(rec)
        self.order.append(kind)

    def __enter__(self):
        from mmfusion import ops
        entered = {}
        for kind in ("text", "audio"):
            pre = self.bb[kind].register_forward_pre_hook(lambda m, a, kind=kind: entered.__setitem__(kind, ops._site))
            post = self.bb[kind].register_forward_hook(
                lambda m, a, kw, out, kind=kind: self._record(kind, a, kw, out.last_hidden_state, entered[kind]), with_kwargs=True)
            self._undo += [pre.remove, post.remove]
        vit = self.bb["video"]
        real = vit.cls_features

        def cls_features(*a, **kw):
            site0 = ops._site
            out = real(*a, **kw)
            self._record("video", a, kw, out, site0)
            return out
        vit.cls_features = cls_features
        self._undo.append(lambda: vit.__dict__.pop("cls_features"))
        return self

    def __exit__(self, *exc):
        for fn in self._undo:
            fn()

    def one(self, kind):
        (rec,) = self.calls[kind]
        return rec


def _cuda(data):
    text, wave, frames, labels = data
    return {k: v.cuda() for k, v in text.items()}, wave.cuda(), frames.cuda(), labels.cuda()


def _zeroed(data, missing):
    """the inputs as ``MultimodalEmotionModel.encode`` hands them to the encoders under ``missing_modalities``"""
    text, wave, frames, labels = data
    missing = missing or ()
    if "text" in missing:
        text = {k: torch.zeros_like(v) for k, v in text.items()}
    return text, torch.zeros_like(wave) if "audio" in missing else wave, torch.zeros_like(frames) if "video" in missing else frames, labels


def _build(fusion="hierarchical", k=1, dropout=0.0, backbone_dropout=False):
    """-> (the whole model, {kind: stand-alone encoder}, {kind: stand-alone backbone}, the twin), on the GPU in train mode"""
    model = cases.base_model(cases.config(fusion, k, dropout, backbone_dropout))
    enc, bb = cases.pieces(model)
    twin = cases.twin_of(model, fusion, dropout)
    on = lambda m: m.cuda().train()
    return on(model), {kind: on(e) for kind, e in enc.items()}, {kind: on(b) for kind, b in bb.items()}, on(twin)


def _atomic(t: torch.Tensor) -> bool:
    """whether a parameter's gradient is summed by float atomics (module docstring): everything but the 2-D matrices"""
    return t.dim() != 2


def _without_key_bias(name: str, g: torch.Tensor) -> torch.Tensor:
    """a fused Q/K/V bias gradient without its key third, which the backward leaves alone (the encoder tests exempt it)"""
    if name.endswith("_qkv_b"):
        d = g.numel() // 3
        return torch.cat([g[:d], g[2 * d:]])
    return g


def _same(what, got, want, worst, atomic=None):
    """``got`` against ``want`` (tensors, or dicts of them by name): bits, or ``F32_TOL`` in relative L2 where ``_atomic``"""
    if not isinstance(got, dict):
        got, want = {"": got}, {"": want}
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want))[:6])
    for name in got:
        a, b = _without_key_bias(name, got[name]), _without_key_bias(name, want[name])
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), (what, name)
        if _atomic(got[name]) if atomic is None else atomic:
            e = l2_rel(a, b)
            if e / F32_TOL > worst[0]:
                worst[0], worst[1] = e / F32_TOL, f"{what} {name}"
            assert e <= F32_TOL, f"{what} {name}: rel L2 {e:.3e} (bound {F32_TOL})"
        else:
            assert torch.equal(_bits(a), _bits(b)), f"{what} {name}: not bit-equal (rel L2 {l2_rel(a, b):.3e})"


def _grads(module, only=None):
    """{name: a copy of the gradient} of the parameters that require one"""
    return {n: p.grad.detach().clone() for n, p in module.named_parameters() if p.requires_grad and (only is None or only(n))}


def _twin_inputs(taps, grad):
    """the twin's three inputs from the whole model's backbone outputs -> (text dict, audio, video, {kind: leaf})"""
    t, a, v = taps.one("text"), taps.one("audio"), taps.one("video")
    leaves = {kind: rec["out"].detach().clone().requires_grad_(grad) for kind, rec in (("text", t), ("audio", a), ("video", v))}
    mask = t["kwargs"]["attention_mask"]
    return {"input_ids": leaves["text"], "attention_mask": mask}, leaves["audio"], leaves["video"].view(mask.shape[0], -1, cases.HIDDEN), leaves


def _forward_seams(tag, model, enc, twin, data, fusion, train, missing=None):
    """test 1's assertions: the whole model's features are the stand-alone encoders', its heads and contrastive losses the twin's"""
    hier = fusion == "hierarchical"
    kw = {"compute_contrastive_loss": True} if hier else {}
    for m in (model, twin, *enc.values()):
        m.train(train)
    text, wave, frames, _ = data
    ztext, zwave, zframes, _ = _zeroed(data, missing)
    worst = [0.0, ""]
    feats, hooks = {}, []
    for kind, e in cases.encoders(model).items():        # (MulT returns its pooled features under the encoders' output names)
        hooks.append(e.register_forward_hook(lambda m, a, o, kind=kind: feats.__setitem__(kind, o["features"].detach())))
    with contextlib.nullcontext() if train else torch.no_grad():
        with Taps(model) as taps:
            out = model(text, wave, frames, missing_modalities=missing, **kw)
        for h in hooks:
            h.remove()
        alone = {"text": enc["text"](ztext["input_ids"], ztext["attention_mask"])["features"], "audio": enc["audio"](zwave)["features"],
                 "video": enc["video"](zframes)["features"]}
        t_in, a_in, v_in, _ = _twin_inputs(taps, False)
        tout = twin(t_in, a_in, v_in, **kw)
    torch.cuda.synchronize()
    for kind in KINDS:
        _same(f"{tag}: the {kind} encoder's features vs the stand-alone encoder", feats[kind], alone[kind], worst, atomic=False)
        if hier:
            _same(f"{tag}: {kind}_features are the encoder's", out[f"{kind}_features"], feats[kind], worst, atomic=False)
        _same(f"{tag}: {kind}_features vs the twin", out[f"{kind}_features"], tout[f"{kind}_features"], worst, atomic=False)
    for key in HEADS:
        _same(f"{tag}: {key} vs the twin", out[key], tout[key], worst, atomic=False)
    if hier:
        assert out["contrastive_losses"] and sorted(out["contrastive_losses"]) == sorted(tout["contrastive_losses"])
        _same(f"{tag}: contrastive loss", {k: v.reshape(1) for k, v in out["contrastive_losses"].items()},
              {k: v.reshape(1) for k, v in tout["contrastive_losses"].items()}, worst, atomic=True)
    for v in [out[k] for k in HEADS] + [out[f"{kind}_features"] for kind in KINDS]:
        assert bool(torch.isfinite(v).all())
    print(f"SEAM {tag}: forward, worst atomic ratio (rel L2 / F32_TOL) {worst[0]:.3e} {worst[1]}")
    for m in (model, twin, *enc.values()):
        m.train(True)


def _step(model, data, zero="full", missing=None, **kw):
    """one forward + ``fusion_loss`` (contrastive terms included) + ``backward_from`` of a whole model or a twin -> (outputs, loss,
    gradients, taps | None)"""
    from mmfusion import arena
    from mmfusion.train import backward_from, fusion_loss
    ar = arena.ensure(model)
    ar.zero_grad(lazy=True) if zero == "lazy" else ar.zero_grad()
    text, wave, frames, labels = data
    native = model.text_encoder.model is not None
    with Taps(model) if native else contextlib.nullcontext() as taps:
        out = model(text, wave, frames, compute_contrastive_loss=True, **({"missing_modalities": missing} if native else {}), **kw)
        loss = fusion_loss(out, labels)
        backward_from(loss)
    ar.finalize_grads()
    torch.cuda.synchronize()
    return out, loss.detach().clone(), _grads(model), taps


def _alone_backward(kind, bb, rec, dout):
    """the stand-alone backbone on the recorded call's arguments, its backward from ``dout`` -> (output, its gradients)"""
    from mmfusion import arena
    arena.ensure(bb).zero_grad()
    kwargs = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in rec["kwargs"].items()}
    args = tuple(a.detach() if isinstance(a, torch.Tensor) else a for a in rec["args"])
    out = bb.cls_features(*args, **kwargs) if kind == "video" else bb(*args, **kwargs).last_hidden_state
    assert out.requires_grad
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), _grads(bb)


def _backward_seams(tag, model, bb, twin, data, missing=None, zero="full"):
    """test 2's assertions on one whole step -> that step's (outputs, loss, gradients, taps)"""
    out, loss, grads, taps = _step(model, data, zero, missing)
    worst = [0.0, ""]
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    # the twin on the backbones' outputs: its input gradients are what arrived at the backbones' outputs
    t_in, a_in, v_in, leaves = _twin_inputs(taps, True)
    tout, tloss, tgrads, _ = _step(twin, (t_in, a_in, v_in, data[3]))
    for kind in KINDS:
        captured = taps.one(kind)["grad"]
        assert captured is not None and leaves[kind].grad is not None, kind
        _same(f"{tag}: d loss / d {kind} backbone output, twin vs captured", leaves[kind].grad, captured, worst, atomic=False)
    _same(f"{tag}: loss", loss.reshape(1), tloss.reshape(1), worst, atomic=True)
    _same(f"{tag}: non-backbone gradient vs the twin", {n: g for n, g in grads.items() if not cases.is_backbone(n)}, tgrads, worst)
    # each stand-alone backbone, given the gradient that arrived, reproduces the whole model's backbone gradients
    whole_bb = cases.backbones(model)
    for kind in KINDS:
        rec = taps.one(kind)
        alone_out, alone = _alone_backward(kind, bb[kind], rec, rec["grad"])
        _same(f"{tag}: {kind} backbone output vs stand-alone", rec["out"].detach(), alone_out, worst, atomic=False)
        _same(f"{tag}: {kind} backbone gradient vs stand-alone", _grads(whole_bb[kind]), alone, worst)
        assert any(bool(g.any()) for g in alone.values()) or (missing and kind in missing), f"{kind}: no gradient at all"
    _frozen_grads_are_empty(model)
    print(f"SEAM {tag}: backward ({zero} zero), worst atomic ratio (rel L2 / F32_TOL) {worst[0]:.3e} {worst[1]}")
    return out, loss, grads, taps


# ---- 1. forward seams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", ["hierarchical", "mult"])
def test_forward_seams(fusion):
    """eval mode and train mode (every dropout probability and ``modality_dropout`` at 0): the whole model's three features are
    the stand-alone encoders', its logits, valence, arousal, uncertainty and contrastive losses the twin's"""
    model, enc, _, twin = _build(fusion)
    data = _cuda(cases.inputs())
    for train in (False, True):
        _forward_seams(f"{fusion} {'train' if train else 'eval'}", model, enc, twin, data, fusion, train)


# ---- 2. backward seams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, "all"])
def test_backward_seams(k):
    """``fusion_loss`` with the contrastive terms, ``backward_from``: the twin's input gradients are the gradients that arrive at
    the backbones' outputs, each stand-alone backbone reproduces the whole model's backbone gradients from them, every other
    gradient is the twin's, frozen parameters have none; then the same step again after ``zero_grad(lazy=True)`` with no full
    zero in between: the lazy-zero protocol across the four owners of one arena"""
    model, _, bb, twin = _build(k=k)
    data = _cuda(cases.inputs())
    _, _, first, _ = _backward_seams(f"k={k}", model, bb, twin, data)
    _, _, again, _ = _backward_seams(f"k={k} lazy", model, bb, twin, data, zero="lazy")
    worst = [0.0, ""]
    _same(f"k={k}: the lazily zeroed step vs the first", again, first, worst)
    print(f"SEAM k={k}: lazy step vs first step, worst atomic ratio {worst[0]:.3e} {worst[1]}")


# ---- 3. sites and masks -------------------------------------------------------------------------------------------------------
class Census:
    """every site ``ops.next_site`` hands out, and the counter's value at each ``begin_training_forward``"""

    def __enter__(self):
        from mmfusion import ops
        self.ops, self.real = ops, (ops.next_site, ops.begin_training_forward)
        self.forwards = []

        def next_site():
            s = self.real[0]()
            self.forwards[-1].append(s)
            return s

        def begin_training_forward():
            self.forwards.append([])
            return self.real[1]()
        ops.next_site, ops.begin_training_forward = next_site, begin_training_forward
        return self

    def __exit__(self, *exc):
        self.ops.next_site, self.ops.begin_training_forward = self.real


def test_sites_and_masks_with_dropout_on():
    """the text backbone's dropout, the audio regularisers with span masking and ``fusion_dropout = 0.1``: the census of one root
    forward, each backbone's bits from the whole forward's state behind the sites handed out before it, a second step from the
    same seeded state, and a step from the next state"""
    from mmfusion import ops
    model, _, bb, _ = _build(k=1, dropout=0.1, backbone_dropout=True)
    data = _cuda(cases.inputs())
    L = cases.LAYERS
    ops.seed_dropout(77)
    with Census() as census:
        _, loss_a, first, taps = _step(model, data)
        used = ops.rng_state().clone()
        _step(model, data)
    assert len(census.forwards) == 2, "one begin_training_forward per root forward"
    for sites in census.forwards:                                              # restarts at each root forward, strictly increasing
        assert sites == list(range(1, len(sites) + 1)) and len(sites) == len(census.forwards[0])
    share = {kind: taps.one(kind)["site1"] - taps.one(kind)["site0"] for kind in KINDS}
    before = {kind: taps.one(kind)["site0"] for kind in KINDS}
    total = len(census.forwards[0])
    print(f"SEAM sites: {total} per root forward; text backbone {share['text']} from {before['text']}, audio {share['audio']} from "
          f"{before['audio']}, video {share['video']} from {before['video']}, behind the video backbone {total - taps.one('video')['site1']}")
    assert taps.order == ["text", "audio", "video"]
    assert share == {"text": 1 + 4 * L, "audio": 3 + 4 * L, "video": 0}
    assert before["text"] == 0 and before["audio"] > share["text"] and before["video"] > before["audio"] + share["audio"]
    assert total > taps.one("video")["site1"], "the fusion layer's sites come behind the backbones'"
    # each backbone alone: the whole forward's state, behind as many sites as were handed out before it
    worst = [0.0, ""]
    whole_bb = cases.backbones(model)
    for kind in ("text", "audio"):
        rec = taps.one(kind)
        with ops.dropout_state(used.clone()):
            for _ in range(before[kind]):
                ops.next_site()
            ops.root_entered()                                                 # (continue this numbering: no forward of its own)
            try:
                alone_out, alone = _alone_backward(kind, bb[kind], rec, rec["grad"])
            finally:
                ops.root_left()
        _same(f"dropout: {kind} backbone output vs stand-alone", rec["out"].detach(), alone_out, worst, atomic=False)
        _same(f"dropout: {kind} backbone gradient vs stand-alone", {n: first[n] for n in _names_of(model, whole_bb[kind])},
              {_prefix(model, whole_bb[kind]) + n: g for n, g in alone.items()}, worst)
        # ... and with the sites one off, the masks are others
        with ops.dropout_state(used.clone()):
            for _ in range(before[kind] + 1):
                ops.next_site()
            ops.root_entered()
            try:
                off_out, _ = _alone_backward(kind, bb[kind], rec, rec["grad"])
            finally:
                ops.root_left()
        assert not torch.equal(_bits(off_out), _bits(alone_out)), f"{kind}: the sites do not select the masks"
    # a second whole step from the same seeded state: every single-writer gradient bit for bit; from the next state: not
    ops.seed_dropout(77)
    _, loss_b, second, _ = _step(model, data)
    _same("dropout: a second step from the same state", second, first, worst)
    assert torch.equal(_bits(loss_a.reshape(1)), _bits(loss_b.reshape(1))) or l2_rel(loss_b, loss_a) <= F32_TOL
    _, _, third, _ = _step(model, data)
    differs = [n for n in first if not _atomic(first[n]) and not torch.equal(_bits(first[n]), _bits(third[n]))]
    assert differs, "a step from the next state reproduced every single-writer gradient"
    for kind in KINDS[:2]:
        assert any(n in differs for n in _names_of(model, whole_bb[kind])), f"{kind}: the next state drew the same masks"
    print(f"SEAM dropout: worst atomic ratio {worst[0]:.3e} {worst[1]}; {len(differs)} of {sum(not _atomic(g) for g in first.values())} "
          f"single-writer gradients differ under the next state")


def _prefix(model, module):
    for name, m in model.named_modules():
        if m is module:
            return name + "."
    raise KeyError


def _names_of(model, module):
    pre = _prefix(model, module)
    return [pre + n for n, p in module.named_parameters() if p.requires_grad]


# ---- 4. edge inputs through missing_modalities --------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", [["text"], ["audio"], ["video"], ["text", "audio", "video"]], ids=lambda m: "+".join(m))
def test_missing_modalities_edge_inputs(missing):
    """train mode, k = 1: the all-zero attention mask (every query row and every key masked), the zero waveform (a GroupNorm
    variance of exactly 0) and zero frames, each the whole input of a training scenario.  Every output and gradient is finite, and
    the seams of tests 1 and 2 hold on the zeroed inputs (the text encoder pools row 0, so the all-masked backbone output reaches
    the loss and a gradient comes back into rows that are masked as queries and as keys)."""
    model, enc, bb, twin = _build(k=1)
    data = _cuda(cases.inputs())
    tag = "missing " + "+".join(missing)
    _forward_seams(tag, model, enc, twin, data, "hierarchical", True, missing)
    out, loss, grads, taps = _backward_seams(tag, model, bb, twin, data, missing)
    for key in HEADS + tuple(f"{kind}_features" for kind in KINDS):
        assert bool(torch.isfinite(out[key]).all()), key
    assert all(bool(torch.isfinite(v).all()) for v in out["contrastive_losses"].values())
    if "text" in missing:
        rec = taps.one("text")
        assert not bool(rec["kwargs"]["attention_mask"].any()) and not bool(rec["kwargs"]["input_ids"].any()) and bool(rec["grad"].any())
    if "audio" in missing:
        assert not bool(taps.one("audio")["args"][0].any())
    if "video" in missing:
        assert not bool(taps.one("video")["args"][0].any())


def _rule_b_or_zero(what, got, exact, stored):
    """rule (b) of tests/test_w2v_finetune_gpu.py per tensor, ||got - exact|| <= 2 ||stored - exact||; a tensor whose exact
    gradient and whose bf16-storage gradient are both exactly 0 has no scale: the kernels must return exactly 0 for it"""
    worst = 0.0
    for key in exact:
        err = float((got[key].double() - exact[key].double()).norm())
        model = float((stored[key].double() - exact[key].double()).norm())
        assert bool(torch.isfinite(got[key]).all())
        print(f"SEAM {what} {key}: ||got - exact|| {err:.3e} (bound (b) 2 x {model:.3e}), ||exact|| {float(exact[key].norm()):.3e}")
        if model == 0.0 and float(exact[key].norm()) == 0.0:
            assert err == 0.0, (key, err)
            continue
        worst = max(worst, err / (2 * model))
        assert err <= 2 * model, (key, err, 2 * model)
    print(f"SEAM {what}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
def test_backbone_on_its_zeroed_input_against_float64(kind):
    """each stand-alone backbone on the input ``missing_modalities`` gives it, against its float64 restatement with the bounds of
    its own tests: the output to ``BOUND_A`` (relative L2 against the restatement with bf16 storage), the top layer's weight
    gradients for a random output gradient to rule (b).  tests/test_native_model_cpu.py shows the restatements finite and
    well-scaled on these inputs."""
    import deberta_ref
    import vit_ref
    import w2v_ref
    from test_deberta_finetune_gpu import _hf_grads
    model = cases.base_model(cases.config(k=1))
    sds = cases.seed_backbones(model)
    bb = cases.backbones(model)[kind].cuda().train()
    cfg, sd = bb.config, sds[kind]
    text, wave, frames, _ = _zeroed(cases.inputs(), list(KINDS))
    L = cfg.num_hidden_layers
    if kind == "text":
        ids, mask = text["input_ids"], text["attention_mask"]
        call = lambda: bb(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
        ref = lambda s, st, dt=torch.float64: deberta_ref.deberta_forward(s, ids, mask, cfg, bf16_storage=st, dtype=dt)
        keys = [key for key in deberta_ref.hf_keys(cfg) if key.startswith(f"encoder.layer.{L - 1}.")]
    elif kind == "audio":
        call = lambda: bb(wave.cuda()).last_hidden_state
        ref = lambda s, st, dt=torch.float64: w2v_ref.w2v_forward(s, wave.to(dt), cfg, bf16_storage=st, dtype=dt)
        keys = [key for key in w2v_ref.hf_keys(cfg) if key.startswith(f"encoder.layers.{L - 1}.") and not key.endswith("k_proj.bias")]
    else:
        flat = frames.reshape(-1, 3, 64, 64)
        call = lambda: bb.cls_features(flat.cuda())
        ref = lambda s, st, dt=torch.float64: vit_ref.vit_forward(s, flat.to(dt), cfg, bf16_storage=st, dtype=dt, cls_last_only=True)
        keys = [key for key in vit_ref.hf_keys(cfg) if key.startswith(f"layers.{L - 1}.") and not key.endswith("k_proj.bias")] \
            + ["layernorm.weight", "layernorm.bias"]
    from mmfusion import arena
    arena.ensure(bb).zero_grad()
    out = call()
    want = ref(sd, True)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(out).all())
    dout = torch.randn(want.shape, generator=torch.Generator().manual_seed(51), dtype=torch.float64)
    out.backward(dout.float().cuda())
    torch.cuda.synchronize()
    err = l2_rel(out.detach(), want)
    print(f"SEAM zeroed input, {kind} backbone: output vs the restatement with bf16 storage {err:.3e} (bound {BOUND_A}); "
          f"||want|| {float(want.norm()):.3e}")
    assert err <= BOUND_A

    def autograd(stored):
        leaves = {key: v.double().clone().requires_grad_(key in keys) for key, v in sd.items()}
        return dict(zip(keys, torch.autograd.grad(ref(leaves, stored), [leaves[key] for key in keys], dout)))
    _rule_b_or_zero(f"zeroed input, {kind} backbone, d", _hf_grads(bb, keys), autograd(False), autograd(True))


# ---- 5. the training steps ----------------------------------------------------------------------------------------------------
LR, WD = 1e-2, 0.1            # lr * wd >= 2^-24 for every step below: a decay of frozen weights shows in f32


def _snapshot(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _check_moved(tag, model, before, opt, reached=None, frozen_backbones=False):
    """every ``requires_grad = False`` parameter is bit-unchanged and has no moment; every trainable backbone parameter (and every
    one of ``reached``) has moved, and by a gradient: weight decay alone moves a parameter too, but leaves Adam's first moment 0"""
    where = {id(q): o for q, o in zip(opt.arena.params, opt.arena.offsets)}
    moment = lambda p: opt.exp_avg[where[id(p)]:where[id(p)] + p.numel()]
    moved = 0
    for n, p in model.named_parameters():
        same = torch.equal(_bits(p.detach()), _bits(before[n]))
        if not p.requires_grad:
            assert same, f"{tag}: the frozen {n} moved by {float((p.detach() - before[n]).abs().max()):.3e}"
            assert not bool(moment(p).any()), f"{tag}: the frozen {n} has a moment"
        elif cases.is_backbone(n) or (reached is not None and id(p) in reached):
            assert not same, f"{tag}: {n} is trainable and reached, and did not move"
            assert bool(moment(p).any()), f"{tag}: {n} moved without a gradient (its first moment is 0)"
            moved += 1
    assert moved > 0 or frozen_backbones
    return moved


def _stepped_forward_seams(tag, base, data):
    """test 1 again on the stepped weights: stand-alone encoders and a twin that LOAD the whole model's stepped ``state_dict``
    (a load moves every version counter and re-casts) against the whole model, which reads what the optimiser's kernel wrote
    (the arena's bf16 shadow) and what the backbones derive from their weights"""
    fresh = cases.base_model(base.config)
    enc = {kind: e.cuda() for kind, e in cases.encoders(fresh).items()}
    for kind, e in cases.encoders(base).items():
        enc[kind].load_state_dict(e.state_dict())
    twin = cases.twin_of(base).cuda()
    _forward_seams(tag, base, enc, twin, data, "hierarchical", False)


def _wrapper_data(data):
    text, wave, frames, labels = data
    return {"text": text, "audio": wave, "video": frames}, labels


def test_robust_step_leaves_frozen_backbone_weights_alone():
    from mmfusion.train import RobustTrainStep
    from models.multimodal_model import RobustMultimodalModel
    torch.manual_seed(3)
    model = RobustMultimodalModel(cases.config(k=1))
    cases.seed_backbones(model.base_model)
    model.base_model.modality_dropout.dropout_rate = 0.0
    model = model.cuda().train()
    text, wave, frames, labels = data = _cuda(cases.inputs())
    ts = RobustTrainStep(model, lr=LR, weight_decay=WD)
    before = _snapshot(model)
    for i in range(3):
        loss = ts(text, wave, frames, labels, missing_modalities=["audio"] if i == 1 else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    moved = _check_moved("RobustTrainStep", model, before, ts.opt, {id(p) for p in ts.reached if p.requires_grad})
    assert all(p.requires_grad for p in ts.reached)
    print(f"SEAM RobustTrainStep: {moved} reached parameters moved, lr * wd = {LR / 25 * WD:.1e}")
    _stepped_forward_seams("RobustTrainStep, stepped", model.base_model, data)


def test_distill_step_leaves_frozen_backbone_weights_alone():
    from mmfusion.train import DistillTrainStep
    from models.multimodal_model import KnowledgeDistillationModel
    teacher = cases.base_model(cases.config(k=0), seed=5)
    torch.manual_seed(3)
    kd = KnowledgeDistillationModel(teacher, cases.config(k=1))
    cases.seed_backbones(kd.student)
    kd.student.modality_dropout.dropout_rate = 0.0
    kd = kd.cuda().train()
    text, wave, frames, labels = data = _cuda(cases.inputs())
    ts = DistillTrainStep(kd, lr=LR, weight_decay=WD, total_steps=10)
    before, t_before = _snapshot(kd.student), _snapshot(kd.teacher)
    for _ in range(3):
        loss = ts(text, wave, frames, labels)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    moved = _check_moved("DistillTrainStep", kd.student, before, ts.opt)
    assert ts.opt.ranges is not None, "a student with frozen parameters takes the subset form"
    for n, p in kd.teacher.named_parameters():
        assert torch.equal(_bits(p.detach()), _bits(t_before[n])), f"the teacher's {n} moved"
    print(f"SEAM DistillTrainStep: {moved} trainable backbone parameters moved")
    _stepped_forward_seams("DistillTrainStep, stepped", kd.student, data)


def test_fewshot_step_freezes_the_backbones_in_both_places():
    """``FewShotTrainStep`` sets ``requires_grad`` by the reference's name rule, which freezes every backbone parameter: the
    backbones' ``trainable_layers`` must then say 0 too (the choice: frozen in both places, as the by-name rule implies), and the
    step moves the adapters, the prompt and the prototype network only"""
    from mmfusion.train import FewShotTrainStep
    from models.multimodal_model import FewShotModel
    base = cases.base_model(cases.config(k=1))
    model = FewShotModel(base, base.config).cuda().train()
    sup, y = _wrapper_data(_cuda(cases.inputs(seed=41)))                       # n_way 2, n_shot 1
    qry, _ = _wrapper_data(_cuda(cases.inputs(seed=42)))                       # 2 queries
    ts = FewShotTrainStep(model, 2, 1, lr=LR, weight_decay=WD)
    for kind, b in cases.backbones(base).items():
        assert b.trainable_layers == 0 and not any(p.requires_grad for p in b.parameters()), kind
    assert ts.reached and all(p.requires_grad for p in ts.reached)
    before = _snapshot(model)
    for _ in range(3):
        loss = ts(sup, qry, y % 2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    moved = _check_moved("FewShotTrainStep", model, before, ts.opt, {id(p) for p in ts.reached}, frozen_backbones=True)
    assert not torch.equal(base.text_encoder.prompt_embeddings.detach(), before["base_model.text_encoder.prompt_embeddings"])
    print(f"SEAM FewShotTrainStep: {moved} reached parameters moved")
    _stepped_forward_seams("FewShotTrainStep, stepped", base, _cuda(cases.inputs()))


@pytest.mark.parametrize("k", [1, "all"])
def test_plain_finetune_loop_leaves_frozen_backbone_weights_alone(k):
    from mmfusion import arena
    from mmfusion.train import backward_from, finetune_optimizer, fusion_loss
    model = cases.base_model(cases.config(k=k)).cuda().train()
    text, wave, frames, labels = data = _cuda(cases.inputs())
    ar = arena.ensure(model)
    opt = finetune_optimizer(model, ar, lr=LR, weight_decay=WD)
    before = _snapshot(model)
    for _ in range(3):
        ar.zero_grad()
        out = model(text, wave, frames, compute_contrastive_loss=True)
        loss = fusion_loss(out, labels)
        backward_from(loss)
        opt.advance()
        opt.launch()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    moved = _check_moved(f"finetune_optimizer k={k}", model, before, opt)
    print(f"SEAM finetune_optimizer loop k={k}: {moved} trainable backbone parameters moved")
    _stepped_forward_seams(f"finetune_optimizer k={k}, stepped", model, data)


# ---- 6. two passes through one backbone before one backward ----------------------------------------------------------------
def test_two_passes_one_backward_accumulate():
    """``FewShotModel`` on the prompt route with the text backbone's top layer trainable: after one backward over the support
    and the query pass, the gradients of ``prompt_embeddings`` and of the text backbone's top layer are, to ``F32_TOL``, the sum of
    the gradients of each pass alone with the other's features detached (gradients accumulate: the order of the f32 additions
    may differ)"""
    from mmfusion import arena, ops, small_ops
    from mmfusion.train import backward_from
    from models.multimodal_model import FewShotModel
    cfg = cases.config(k=0)
    cfg.text_backbone_trainable_layers = 1
    base = cases.base_model(cfg)
    model = FewShotModel(base, cfg).cuda().train()
    sup, y = _wrapper_data(_cuda(cases.inputs(seed=41)))
    qry, _ = _wrapper_data(_cuda(cases.inputs(seed=42)))
    ar = arena.ensure(model)
    picked = lambda n: n.endswith("prompt_embeddings") or n.startswith("base_model.text_encoder.model.")
    encode = model._encode

    def run(live):
        """``live``: which of the two passes (0 support, 1 query) keep their graph"""
        calls = []

        def _encode(data):
            feats = encode(data)
            calls.append(1)
            return feats if len(calls) - 1 in live else tuple(t.detach() for t in feats)
        model._encode = _encode
        try:
            ar.zero_grad()
            ops.seed_dropout(78)                         # (the adapters' dropout is a constant 0.1: the same masks in every run)
            with Taps(base) as taps:
                out = model(sup, qry, 2, 1)
                backward_from(small_ops.fusion_loss(out["predictions"], y % 2, 0.0, [], []))
            torch.cuda.synchronize()
        finally:
            del model._encode
        return _grads(model, picked), taps
    both, taps = run({0, 1})
    assert len(taps.calls["text"]) == 2 and all("inputs_embeds" in rec["kwargs"] and rec["grad"] is not None for rec in taps.calls["text"])
    first, _ = run({0})
    second, _ = run({1})
    worst = [0.0, ""]
    _same("two passes, one backward vs the sum of each alone", both, {n: first[n] + second[n] for n in both}, worst, atomic=True)
    assert bool(both["base_model.text_encoder.prompt_embeddings"].any())
    assert l2_rel(both["base_model.text_encoder.prompt_embeddings"], first["base_model.text_encoder.prompt_embeddings"]) > 1e-2
    print(f"SEAM two passes, one backward: worst rel L2 / F32_TOL {worst[0]:.3e} {worst[1]}")


# ---- 7. the captured step -----------------------------------------------------------------------------------------------------
def test_captured_robust_step_on_native_backbones():
    """``RobustTrainStep`` at k = 1 with every dropout on, captured single-stream after a warm-up on a side stream and replayed
    twice.  The first replay against an eager step from the same optimiser state, arena and rng state: gradients and the stepped
    masters of the matrices bit for bit, the atomics list to ``F32_TOL`` (the stepped vectors are not compared: Adam normalises a
    gradient that is atomic-order noise to +- lr, DESIGN.md section 5, "drift").  The second replay draws other masks;
    ``step_dev`` advances by one per replay."""
    import bench
    from mmfusion import ops
    from mmfusion.train import RobustTrainStep
    from models.multimodal_model import RobustMultimodalModel
    torch.manual_seed(3)
    model = RobustMultimodalModel(cases.config(k=1, dropout=0.1, backbone_dropout=True))
    cases.seed_backbones(model.base_model)
    model = model.cuda().train()
    text, wave, frames, labels = _cuda(cases.inputs())
    ts = RobustTrainStep(model, lr=LR, weight_decay=WD)
    ar, opt = ts.arena, ts.opt
    step = lambda: ts(text, wave, frames, labels)
    state = [ar.master_full, ar.shadow_full, ar.grads_full, opt.exp_avg, opt.exp_avg_sq, opt.step_dev, opt.hparams, ops.rng_state()]

    def restore(saved):
        for x, v in zip(state, saved):
            x.copy_(v)
        torch.cuda.synchronize()

    def snap(loss):
        torch.cuda.synchronize()
        return loss.detach().clone(), _grads(model), _snapshot(model)
    with bench.single_stream():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = step()
        torch.cuda.synchronize()
        s0 = [x.clone() for x in state]
        t0 = int(opt.step_dev.item())
        loss_e, grads_e, params_e = snap(step())
        restore(s0)
        graph.replay()
        loss_1, grads_1, params_1 = snap(static_loss)
        graph.replay()
        loss_2, grads_2, _ = snap(static_loss)
        t2 = int(opt.step_dev.item())
    worst = [0.0, ""]
    _same("captured step: gradient, first replay vs eager", grads_1, grads_e, worst)
    _same("captured step: loss", loss_1.reshape(1), loss_e.reshape(1), worst, atomic=True)
    _same("captured step: stepped matrices", {n: p for n, p in params_1.items() if not _atomic(p)},
          {n: p for n, p in params_e.items() if not _atomic(p)}, worst)
    differs = [n for n in grads_1 if not _atomic(grads_1[n]) and bool(grads_1[n].any()) and not torch.equal(_bits(grads_1[n]), _bits(grads_2[n]))]
    assert differs, "the second replay drew the first one's masks"
    assert t2 == t0 + 2, (t0, t2)
    _frozen_grads_are_empty(model)
    print(f"SEAM captured RobustTrainStep: worst atomic ratio {worst[0]:.3e} {worst[1]}; {len(differs)} single-writer gradients differ "
          f"between the two replays; step_dev {t0} -> {t2}")
