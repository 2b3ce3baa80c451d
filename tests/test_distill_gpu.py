"""Knowledge distillation on the MI355X: the two KD entry points of csrc/loss.hip against the float64 restatement of
tests/distill_ref.py (per-case f32 error models, worst error reported as a fraction of its bound), their refusals, the
``KnowledgeDistillationModel`` wrapper and ``mmfusion.train.DistillTrainStep`` (loss value, student gradients against the
torch formulation, a frozen teacher that stays bitwise unchanged, dropout isolation of the teacher's forward)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from distill_ref import kd_grad_bound, kd_loss_bound, kd_value_grad
from helpers import check_graph_replay_matches_eager, hip_lib, l2_rel

pytestmark = pytest.mark.gpu

MMF_E_SHAPE = -1


def _kl(s, t, T, grad=True):
    L, st = hip_lib()
    B, Cn = s.shape
    loss = torch.full((), float("nan"), device="cuda")
    ds = torch.full((B, Cn), float("nan"), device="cuda") if grad else None
    rc = L.mmf_distill_kl(s.data_ptr(), s.stride(0), t.data_ptr(), t.stride(0), B, Cn, float(T), loss.data_ptr(),
                          ds.data_ptr() if grad else None, st)
    return rc, loss, ds


def _ptrs(extras, weights):
    n = len(extras)
    return (C.c_void_p * max(n, 1))(*[e.data_ptr() for e in extras]), (C.c_float * max(n, 1))(*weights), n


def _fl(s, y, eps, extras, weights):
    L, st = hip_lib()
    B, Cn = s.shape
    loss = torch.full((), float("nan"), device="cuda")
    d = torch.full((B, Cn), float("nan"), device="cuda")
    pe, pw, n = _ptrs(extras, weights)
    rc = L.mmf_fusion_loss(s.data_ptr(), s.stride(0), y.data_ptr(), B, Cn, float(eps), pe, pw, n, loss.data_ptr(), d.data_ptr(), st)
    assert rc == 0
    return loss, d


def _flkd(s, y, eps, extras, weights, t, T, w, ldt=None, B=None, Cn=None):
    L, st = hip_lib()
    B = s.shape[0] if B is None else B
    Cn = s.shape[1] if Cn is None else Cn
    loss = torch.full((), float("nan"), device="cuda")
    d = torch.full((max(B, 1), max(Cn, 1)), float("nan"), device="cuda")
    pe, pw, n = _ptrs(extras, weights)
    rc = L.mmf_fusion_loss_kd(s.data_ptr(), s.stride(0), y.data_ptr(), B, Cn, float(eps), pe, pw, n,
                              t.data_ptr() if t is not None else None, (t.stride(0) if t is not None else 80) if ldt is None else ldt, float(T), float(w),
                              loss.data_ptr(), d.data_ptr(), st)
    return rc, loss, d


def _logits(B, Cn, scale, seed, ld=None):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, Cn, generator=g) * scale).clamp_(-20.0 if scale <= 20 else -scale, 20.0 if scale <= 20 else scale)
    if ld is None:
        return x.cuda()
    buf = torch.randn(B, ld, generator=g).cuda() * 1e3            # padding that must not be read
    buf[:, :Cn] = x.cuda()
    return buf[:, :Cn]


def _check_kd(s, t, T, worst, label, bar=True):
    rc, loss, ds = _kl(s, t, T)
    assert rc == 0, label
    torch.cuda.synchronize()
    ref, gref = kd_value_grad(s, t, T)
    ref = float(ref)
    e = abs(float(loss) - ref)
    b = kd_loss_bound(s, t, T, ref)
    eg = float((ds.double().cpu() - gref).abs().max())
    bg = kd_grad_bound(s, T)
    worst["loss"] = max(worst["loss"], e / b)
    worst["grad"] = max(worst["grad"], eg / bg)
    assert e <= b, f"{label}: loss err {e:.3e} > bound {b:.3e}"
    assert eg <= bg, f"{label}: grad err {eg:.3e} > bound {bg:.3e}"
    if bar:                                          # the issue's fixed bar for |logits| <= 20
        B = s.shape[0]
        assert e <= 1e-5 * max(1.0, abs(ref)), f"{label}: loss err {e:.3e}"
        assert eg <= 2e-6 * (1 + T) / B, f"{label}: grad err {eg:.3e}"
    return loss, ds


def test_distill_kl_against_float64():
    worst = {"loss": 0.0, "grad": 0.0}
    for B in (1, 16, 257, 1024):
        for Cn in (2, 7, 64):
            for T in (0.5, 1.0, 4.0):
                s = _logits(B, Cn, 5.0, 1000 * B + Cn)
                t = _logits(B, Cn, 5.0, 7 + 1000 * B + Cn)
                _check_kd(s, t, T, worst, f"B={B} C={Cn} T={T}")
                # teacher equal to student: exactly zero
                rc, loss, ds = _kl(s, s, T)
                torch.cuda.synchronize()
                assert rc == 0 and abs(float(loss)) <= 1e-6 and float(ds.abs().max()) <= 1e-7, f"B={B} C={Cn} T={T}: t == s"
    # strided teacher and student views (row strides above C, padding full of large values)
    for B, Cn, T in ((16, 7, 4.0), (257, 64, 0.5), (3, 2, 1.0)):
        s = _logits(B, Cn, 20.0, 11 + B, ld=Cn + 9)
        t = _logits(B, Cn, 20.0, 12 + B, ld=3 * Cn + 5)
        assert s.stride(0) > Cn and t.stride(0) > Cn
        _check_kd(s, t, T, worst, f"strided B={B} C={Cn} T={T}")
    # |logits| up to 1e4 at T = 1 (the error model's bound only: the fixed bar is for |logits| <= 20)
    for B, Cn in ((16, 7), (257, 64)):
        s, t = _logits(B, Cn, 1e4, 21 + Cn), _logits(B, Cn, 1e4, 22 + Cn)
        s[0, 0], t[0, 1] = 1e4, -1e4
        _check_kd(s, t, 1.0, worst, f"large B={B} C={Cn}", bar=False)
    print(f"distill_kl: worst error / bound: loss {worst['loss']:.3e}, grad {worst['grad']:.3e}")


def test_fusion_loss_kd_equals_fusion_loss_plus_weighted_kd():
    worst = 0.0
    for B, Cn, T, w, ld in ((1, 2, 0.5, 0.5, None), (16, 7, 4.0, 0.5, None), (257, 64, 1.0, 2.0, 70), (1024, 7, 4.0, 0.5, 9)):
        s = _logits(B, Cn, 5.0, B + Cn, ld=ld)
        t = _logits(B, Cn, 5.0, 3 * B + Cn, ld=None if ld is None else ld + 4)
        y = torch.randint(0, Cn, (B,), generator=torch.Generator().manual_seed(B)).cuda()
        extras = [torch.rand((), device="cuda") for _ in range(3)]
        l_ce, d_ce = _fl(s, y, 0.1, extras, [0.1] * 3)
        _, l_kd, d_kd = _kl(s, t, T)
        rc, l_all, d_all = _flkd(s, y, 0.1, extras, [0.1] * 3, t, T, w)
        assert rc == 0
        torch.cuda.synchronize()
        want = float(l_ce) + w * float(l_kd)
        e = abs(float(l_all) - want)
        b = 1e-5 * max(1.0, abs(want))
        assert e <= b, f"B={B} C={Cn}: loss {float(l_all)} vs {want}"
        eg = float((d_all - (d_ce + w * d_kd)).abs().max())
        bg = 2e-6 * (1 + w * T) / B
        assert eg <= bg, f"B={B} C={Cn}: grad err {eg:.3e}"
        worst = max(worst, e / b, eg / bg)
        # and the KD part against float64 directly
        ref, gref = kd_value_grad(s, t, T)
        assert abs(float(l_all) - float(l_ce) - w * float(ref)) <= 1e-5 * max(1.0, abs(want))
    print(f"fusion_loss_kd vs fusion_loss + w * distill_kl: worst error / bar {worst:.3e}")


def test_kd_entry_points_refuse_bad_arguments():
    B, Cn = 4, 7
    s = torch.randn(B, 80, device="cuda")          # every buffer large enough that a wrongly accepted call stays in bounds
    t = torch.randn(B, 80, device="cuda")
    y = torch.zeros(B, dtype=torch.int64, device="cuda")
    L, st = hip_lib()
    bad_kl = [dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(teacher=None), dict(ldt=6),
              dict(lds=6), dict(C=0), dict(C=65), dict(B=0), dict(loss=None)]
    for case in bad_kl:
        a = dict(student=s.data_ptr(), lds=80, teacher=t.data_ptr(), ldt=80, B=B, C=Cn, T=4.0, loss=1)
        a.update(case)
        loss = torch.full((), float("nan"), device="cuda")
        ds = torch.full((B, 80), float("nan"), device="cuda")
        rc = L.mmf_distill_kl(a["student"], a["lds"], a["teacher"], a["ldt"], a["B"], a["C"], a["T"],
                              loss.data_ptr() if a["loss"] else None, ds.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == MMF_E_SHAPE, case
        assert bool(loss.isnan()) and bool(ds.isnan().all()), case
    sv, tv = s[:, :Cn], t[:, :Cn]
    bad_kd = [dict(T=0.0), dict(T=float("nan")), dict(T=-2.0), dict(w=float("nan")), dict(w=float("inf")), dict(t=None),
              dict(ldt=6), dict(eps=1.0), dict(eps=-0.1), dict(Cn=65), dict(B=0)]
    for case in bad_kd:
        a = dict(t=tv, T=4.0, w=0.5, eps=0.1, ldt=None, B=None, Cn=None)
        a.update(case)
        rc, loss, d = _flkd(sv, y, a["eps"], [], [], a["t"], a["T"], a["w"], ldt=a["ldt"], B=a["B"], Cn=a["Cn"])
        torch.cuda.synchronize()
        assert rc == MMF_E_SHAPE, case
        assert bool(loss.isnan()) and bool(d.isnan().all()), case
    # n_extra out of range, null targets, null loss
    pe, pw, _ = _ptrs([torch.zeros((), device="cuda")] * 9, [0.1] * 9)
    loss = torch.full((), float("nan"), device="cuda")
    d = torch.full((B, Cn), float("nan"), device="cuda")
    for n, tgt, lp in ((9, y.data_ptr(), loss.data_ptr()), (-1, y.data_ptr(), loss.data_ptr()), (0, None, loss.data_ptr()),
                       (0, y.data_ptr(), None)):
        rc = L.mmf_fusion_loss_kd(sv.data_ptr(), 80, tgt, B, Cn, 0.1, pe, pw, n, tv.data_ptr(), 80, 4.0, 0.5, lp, d.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == MMF_E_SHAPE, (n, tgt, lp)
        assert bool(loss.isnan()) and bool(d.isnan().all())


# ------------------------------------------------------------------------------------------------------------------------
# the wrapper and the training step
# ------------------------------------------------------------------------------------------------------------------------
def _cfg(d, heads, G, dropout=0.0, precision=None):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = True
    cfg.fusion_type = "hierarchical"
    cfg.fusion_hidden_size, cfg.fusion_num_heads = d, heads
    cfg.graph_hidden_size, cfg.graph_num_layers = G, 3
    cfg.fusion_dropout = cfg.graph_dropout = dropout
    if precision:
        cfg.fusion_precision = precision
    return cfg


PAIRS = {"meld": ((512, 8, 512), (256, 4, 256), 16), "small": ((256, 4, 256), (128, 2, 128), 4)}


def _pair(kind, dropout=0.0, precision=None, modality_dropout=0.0, seed=5):
    from models.multimodal_model import KnowledgeDistillationModel, MultimodalEmotionModel
    (td, th, tg), (sd, sh, sg), B = PAIRS[kind]
    tcfg, scfg = _cfg(td, th, tg, dropout, precision), _cfg(sd, sh, sg, dropout, precision)
    torch.manual_seed(seed)
    teacher = MultimodalEmotionModel(tcfg)
    kd = KnowledgeDistillationModel(teacher, scfg).cuda().train()
    kd.teacher.modality_dropout.dropout_rate = kd.student.modality_dropout.dropout_rate = modality_dropout
    return tcfg, scfg, kd, B


def _inputs(B, seed=1234):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, 9, 768, generator=g)
    audio = torch.randn(B, 21, 768, generator=g)
    video = torch.randn(B, 6, 768, generator=g)
    mask = torch.ones(B, 9, dtype=torch.long)
    labels = torch.randint(0, 7, (B,), generator=torch.Generator().manual_seed(7))
    return text, mask, audio, video, labels


def _cuda_inputs(B, seed=1234):
    text, mask, audio, video, labels = _inputs(B, seed)
    return {"input_ids": text.cuda(), "attention_mask": mask.cuda()}, audio.cuda(), video.cuda(), labels.cuda()


@pytest.mark.parametrize("kind", ["meld", "small"])
def test_wrapper_distillation_loss_matches_float64(kind):
    _, _, kd, B = _pair(kind)
    ti, au, vi, _ = _cuda_inputs(B)
    out = kd(ti, au, vi, compute_contrastive_loss=True)
    for k in ("distillation_loss", "teacher_logits", "emotion_logits", "contrastive_losses", "valence"):
        assert k in out, k
    ref, _ = kd_value_grad(out["emotion_logits"], out["teacher_logits"], kd.temperature)
    got = float(out["distillation_loss"].detach())
    assert abs(got - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), f"{kind}: {got} vs {float(ref)}"
    assert float(ref) > 0
    assert not out["teacher_logits"].requires_grad


def _torch_total(out, t_logits, labels, T):
    s = out["emotion_logits"].float()
    loss = F.cross_entropy(s, labels, label_smoothing=0.1)
    cl = out.get("contrastive_losses") or {}
    if cl:
        loss = loss + 0.1 * sum(cl.values())
    kd = F.kl_div(F.log_softmax(s / T, dim=-1), F.softmax(t_logits.float() / T, dim=-1), reduction="batchmean") * T ** 2
    return loss + 0.5 * kd


def _grad_sweep(kd, got_grads, want_grads, tol, label):
    params = dict(kd.student.named_parameters())
    scale = max(float(g.norm()) for g in want_grads.values())
    worst, checked = (0.0, ""), 0
    for n in params:
        want, got = want_grads[n], got_grads[n]
        if float(want.norm()) <= 1e-6 * scale:
            assert float(got.norm()) <= 1e-3 * scale, f"{label}: {n} should have a (near-)zero gradient"
            continue
        e = l2_rel(got, want)
        checked += 1
        if e > worst[0]:
            worst = (e, n)
    print(f"{label}: {checked} student parameter gradients, worst rel L2 {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= tol, f"{label}: grad {worst[1]} rel L2 {worst[0]:.3e} > {tol}"
    return checked


@pytest.mark.parametrize("kind,precision,tol", [("meld", "bf16", 2e-3), ("small", "bf16", 2e-3)])
def test_step_gradients_match_torch_formulation(kind, precision, tol):
    """DistillTrainStep.fwd_bwd (one fused loss launch) against the same HIP model backpropagated from torch's
    CE + 0.1 * contrastive + 0.5 * kl_div * T^2."""
    from mmfusion.train import DistillTrainStep
    _, _, kd, B = _pair(kind, precision=None if precision == "bf16" else precision)
    ti, au, vi, labels = _cuda_inputs(B)
    ts = DistillTrainStep(kd, lr=1e-3, weight_decay=1e-5, total_steps=10)
    loss = ts.fwd_bwd(ti, au, vi, labels)
    torch.cuda.synchronize()
    got = {n: p.grad.detach().float().cpu().clone() for n, p in kd.student.named_parameters()}
    ts.arena.zero_grad()
    out = kd.student(ti, au, vi, compute_contrastive_loss=True)
    t_logits = kd.teacher_forward(ti, au, vi, compute_contrastive_loss=True)["emotion_logits"]
    lt = _torch_total(out, t_logits, labels, kd.temperature)
    lt.backward()
    torch.cuda.synchronize()
    want = {n: p.grad.detach().float().cpu().clone() for n, p in kd.student.named_parameters()}
    lv, tv = float(loss.detach()), float(lt.detach())
    assert abs(lv - tv) <= 1e-4 * max(1.0, abs(tv)), (lv, tv)
    assert _grad_sweep(kd, got, want, tol, f"{kind}/{precision} step vs torch formulation") >= 30


def test_teacher_untouched_by_training_steps():
    from mmfusion.train import DistillTrainStep
    _, _, kd, B = _pair("small", dropout=0.1, modality_dropout=0.1)
    ti, au, vi, labels = _cuda_inputs(B)
    ts = DistillTrainStep(kd, lr=1e-2, weight_decay=1e-1, total_steps=10)
    t0 = {n: p.detach().clone() for n, p in kd.teacher.named_parameters()}
    s0 = {n: p.detach().clone() for n, p in kd.student.named_parameters()}
    for _ in range(3):
        ts(ti, au, vi, labels)
    torch.cuda.synchronize()
    for n, p in kd.teacher.named_parameters():
        assert torch.equal(p.detach(), t0[n]), f"teacher {n} moved"
        assert p.grad is None or not bool(p.grad.any()), f"teacher {n} has a gradient"
        assert not p.requires_grad
    moved = sum(not torch.equal(p.detach(), s0[n]) for n, p in kd.student.named_parameters())
    assert moved >= 0.9 * len(s0), f"only {moved} of {len(s0)} student parameters moved"
    assert ts.opt.arena.numel < sum(((p.numel() + 63) // 64) * 64 for p in kd.parameters())


def _ce_only_run(kd, inputs, teacher_mode, seed):
    """seeded dropout; kd forward (or the student alone when teacher_mode is None); loss = the student's CE only"""
    from mmfusion import arena as arena_mod, ops, small_ops
    ti, au, vi, labels = inputs
    ar = arena_mod.ensure(kd.student)
    ar.zero_grad()
    ops.seed_dropout(seed)
    if teacher_mode is None:
        out = kd.student(ti, au, vi)
    else:
        kd.teacher.train(teacher_mode == "train")
        out = kd(ti, au, vi)
    loss = small_ops.fusion_loss(out["emotion_logits"], labels, 0.1, [], [])
    small_ops.backward_from(loss)
    torch.cuda.synchronize()
    return out["emotion_logits"].detach().clone(), ar.grads.detach().clone()


def _same(a, b):
    """bitwise, or within 1e-6 relative (gradient kernels that accumulate with atomics may reorder additions)"""
    return torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6 * max(1e-30, float(b.abs().max()))


def test_teacher_forward_leaves_student_dropout_alone(monkeypatch):
    from mmfusion import ops
    _, _, kd, B = _pair("small", dropout=0.1, modality_dropout=0.1)
    kd.train()
    inputs = _cuda_inputs(B)
    kd.teacher_rng_state()
    lo_t, g_t = _ce_only_run(kd, inputs, "train", 77)
    lo_e, g_e = _ce_only_run(kd, inputs, "eval", 77)
    lo_s, g_s = _ce_only_run(kd, inputs, None, 77)
    assert torch.equal(lo_t, lo_e) and torch.equal(lo_t, lo_s), "student outputs depend on the teacher's mode"
    assert _same(g_t, g_e) and _same(g_t, g_s), "student gradients depend on the teacher's mode"
    assert float(g_s.abs().max()) > 0
    # the same test with the isolation removed (the teacher advances the student's state): it must notice
    class _NoIsolation:
        def __init__(self, state):
            pass

        def __enter__(self):
            return None

        def __exit__(self, *exc):
            return False
    monkeypatch.setattr(ops, "dropout_state", _NoIsolation)
    lo_m, g_m = _ce_only_run(kd, inputs, "train", 77)
    monkeypatch.undo()
    assert torch.equal(lo_m, lo_s)                    # the student's forward ran before the teacher's ...
    assert not _same(g_m, g_s), "a teacher that advances the student's dropout state went unnoticed"   # ... its backward did not


def test_distill_step_graph_replay_matches_eager():
    """Three DistillTrainStep steps captured as one single-chain graph (bench.single_stream) and replayed, against three
    eager steps from the same state — with dropout on in both models (teacher in train mode), so the teacher's isolated
    dropout state is exercised under capture too.  Compared per step: the loss, the whole student gradient arena and the
    student parameters.  The learning rate is small on purpose: the GAT backward accumulates with atomics (last-bit
    nondeterminism, ~1e-7 of a gradient) and Adam turns a sign flip of a near-zero gradient into a 2 x lr parameter step,
    so at lr = 1e-3 two EAGER runs drift apart by ~1e-3 within three steps; at lr = 1e-7 that stays under 1e-6."""
    from mmfusion.train import DistillTrainStep
    _, _, kd, B = _pair("small", dropout=0.1, modality_dropout=0.1)
    assert kd.teacher.training
    ti, au, vi, labels = _cuda_inputs(B)
    ts = DistillTrainStep(kd, lr=1e-7, weight_decay=1e-2, total_steps=10)
    eager, replay, worst_g, worst_p, moved = check_graph_replay_matches_eager(lambda: ts(ti, au, vi, labels), ts.arena, ts.opt,
                                                                              [kd.teacher_rng_state()])
    print(f"graph replay: losses {[r[0] for r in replay]} (eager {[e[0] for e in eager]}); worst gradient diff "
          f"{worst_g:.2e} of max, worst parameter diff {worst_p:.2e} (parameters moved up to {moved:.2e})")
