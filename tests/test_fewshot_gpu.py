"""FewShotModel on the MI355X: the episode-head kernels of csrc/fewshot.hip against the float64 restatement of
tests/fewshot_ref.py (per-element f32 error bounds, worst error reported as a fraction of its bound), zero distances,
determinism and refusals, the head in the fp32 parity mode, the wrapper in eval mode against the base model, and
``mmfusion.train.FewShotTrainStep`` (gradients against the torch formulation of the head, which parameters it steps and
which weight gradients it queues, graph replay, checkpoints)."""

import pytest
import torch

from fewshot_ref import dist_bwd_bound, dist_fwd, pred_bound, proto_bwd_bound, proto_fwd, query_features
from helpers import check_graph_replay_matches_eager, hip_lib, l2_rel, ptr3, within_bound

pytestmark = pytest.mark.gpu

MMF_E_SHAPE, MMF_E_ALIGN = -1, -3
NAN = float("nan")


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _nan(*s):
    return torch.full(s, NAN, device="cuda")


def _proto_fwd(s3, n_way, n_shot, d=None):
    L, st = hip_lib()
    S, d0 = s3[0].shape
    sf, mean = _nan(S, d0), _nan(n_way, d0)
    rc = L.mmf_fewshot_proto_fwd(ptr3(s3), sf.data_ptr(), mean.data_ptr(), n_way, n_shot, d0 if d is None else d, st)
    return rc, sf, mean


def _proto_bwd(dmean, dsf, n_way, n_shot, d=None):
    L, st = hip_lib()
    d0 = dmean.shape[1]
    ds = _nan(n_way * n_shot, d0)
    rc = L.mmf_fewshot_proto_bwd(dmean.data_ptr(), _ptr(dsf), ds.data_ptr(), n_way, n_shot, d0 if d is None else d, st)
    return rc, ds


def _dist_fwd(q3, P, Nq=None, n_way=None, d=None):
    L, st = hip_lib()
    Nq0, d0 = q3[0].shape
    nw = P.shape[0]
    qf, dist, pred = _nan(Nq0, d0), _nan(Nq0, nw), _nan(Nq0, nw)
    rc = L.mmf_fewshot_dist_fwd(ptr3(q3), _ptr(P), qf.data_ptr(), dist.data_ptr(), pred.data_ptr(), Nq0 if Nq is None else Nq,
                                nw if n_way is None else n_way, d0 if d is None else d, st)
    return rc, qf, dist, pred


def _dist_bwd(qf, P, dist, pred, gd, gp, want_q=True, want_p=True, Nq=None, n_way=None, d=None):
    L, st = hip_lib()
    Nq0, d0 = qf.shape
    nw = P.shape[0]
    dq = _nan(Nq0, d0) if want_q else None
    dP = _nan(nw, d0) if want_p else None
    rc = L.mmf_fewshot_dist_bwd(qf.data_ptr(), P.data_ptr(), dist.data_ptr(), pred.data_ptr(), _ptr(gd), _ptr(gp), _ptr(dq),
                                _ptr(dP), Nq0 if Nq is None else Nq, nw if n_way is None else n_way, d0 if d is None else d, st)
    return rc, dq, dP


def _episode(n_way, n_shot, Nq, d, seed):
    g = torch.Generator().manual_seed(seed)
    s3 = [torch.randn(n_way * n_shot, d, generator=g).cuda() for _ in range(3)]
    q3 = [torch.randn(Nq, d, generator=g).cuda() for _ in range(3)]
    P = (torch.randn(n_way, d, generator=g) * 1.5).cuda()
    return s3, q3, P, g


# ------------------------------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------------------------------
CASES = [(7, 1, 16, 512), (7, 5, 16, 512), (7, 50, 16, 512), (7, 5, 16, 768), (64, 3, 40, 512), (64, 64, 1024, 1024),
         (1, 1, 1, 4), (5, 10, 16, 256)]


def test_fewshot_kernels_against_float64():
    worst_f, worst_b = [0.0, ""], [0.0, ""]
    for n_way, n_shot, Nq, d in CASES:
        label = f"n_way={n_way} n_shot={n_shot} Nq={Nq} d={d}"
        s3, q3, P, g = _episode(n_way, n_shot, Nq, d, n_way * 1000 + n_shot * 10 + d)
        rc, sf, mean = _proto_fwd(s3, n_way, n_shot)
        torch.cuda.synchronize()
        assert rc == 0, label
        ref = proto_fwd(s3, n_way, n_shot)
        within_bound(sf, ref["sf"], ref["e_sf"], label + " support_features", worst_f)
        within_bound(mean, ref["mean"], ref["e_mean"], label + " mean", worst_f)
        rc, qf, dist, pred = _dist_fwd(q3, P)
        torch.cuda.synchronize()
        assert rc == 0, label
        rq, e_q = query_features(q3)
        within_bound(qf, rq, e_q, label + " query_features", worst_f)
        rd = dist_fwd(qf, P)
        within_bound(dist, rd["dist"], rd["e_dist"], label + " distances", worst_f)
        rp = torch.softmax(-dist.double().cpu(), dim=-1)            # from the kernel's own f32 distances
        within_bound(pred, rp, pred_bound(dist, rp), label + " predictions", worst_f)
        # backward, with each upstream gradient alone and both
        for which in ("pred", "dist", "both"):
            gd = torch.randn(Nq, n_way, generator=g).cuda() if which in ("dist", "both") else None
            gp = torch.randn(Nq, n_way, generator=g).cuda() if which in ("pred", "both") else None
            rc, dq, dP = _dist_bwd(qf, P, dist, pred, gd, gp)
            torch.cuda.synchronize()
            assert rc == 0, label
            rq_, rP_, e_dq, e_dP = dist_bwd_bound(qf, P, dist, pred, gd, gp)
            within_bound(dq, rq_, e_dq, f"{label} grads={which} dq", worst_b)
            within_bound(dP, rP_, e_dP, f"{label} grads={which} dP", worst_b)
        dmean = torch.randn(n_way, d, generator=g).cuda()
        for dsf in (None, torch.randn(n_way * n_shot, d, generator=g).cuda()):
            rc, ds = _proto_bwd(dmean, dsf, n_way, n_shot)
            torch.cuda.synchronize()
            assert rc == 0, label
            want, bound = proto_bwd_bound(dmean, dsf, n_shot)
            within_bound(ds, want, bound, f"{label} ds dsf={dsf is not None}", worst_b)
    print(f"fewshot head: {len(CASES)} episodes; worst error / bound: forward {worst_f[0]:.3e} ({worst_f[1]}), "
          f"backward {worst_b[0]:.3e} ({worst_b[1]})")


def test_zero_distance_is_exact_and_sends_no_gradient():
    n_way, d, Nq = 7, 512, 16
    _, q3, P, g = _episode(n_way, 1, Nq, d, 77)
    # query 3 is prototype 4 exactly: (t + a) + v = P[4] with t = P[4], a = v = 0
    q3 = [x.clone() for x in q3]
    q3[0][3], q3[1][3], q3[2][3] = P[4], 0.0, 0.0
    rc, qf, dist, pred = _dist_fwd(q3, P)
    torch.cuda.synchronize()
    assert rc == 0 and float(dist[3, 4]) == 0.0 and bool((dist.cpu() > 0).sum() == Nq * n_way - 1)
    gd, gp = torch.randn(Nq, n_way, generator=g).cuda(), torch.randn(Nq, n_way, generator=g).cuda()
    rc, dq, dP = _dist_bwd(qf, P, dist, pred, gd, gp)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dP).all())
    # the (3, 4) pair contributes nothing: the result equals the float64 sum over the other pairs
    rq, rP, e_dq, e_dP = dist_bwd_bound(qf, P, dist, pred, gd, gp)
    assert bool(((dq.double().cpu() - rq).abs() <= e_dq).all()) and bool(((dP.double().cpu() - rP).abs() <= e_dP).all())
    # ... and with only that pair's upstream gradient non-zero, both gradients are exactly zero
    gd1 = torch.zeros(Nq, n_way, device="cuda")
    gd1[3, 4] = 1.0
    rc, dq1, dP1 = _dist_bwd(qf, P, dist, pred, gd1, None)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(dq1.any()) and not bool(dP1.any())


def test_backward_is_bit_deterministic():
    s3, q3, P, g = _episode(7, 5, 64, 512, 5)
    _, qf, dist, pred = _dist_fwd(q3, P)
    gd, gp = torch.randn(64, 7, generator=g).cuda(), torch.randn(64, 7, generator=g).cuda()
    outs = [_dist_bwd(qf, P, dist, pred, gd, gp)[1:] for _ in range(3)]
    dm = torch.randn(7, 512, generator=g).cuda()
    dss = [_proto_bwd(dm, None, 7, 5)[1] for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    assert all(torch.equal(x, dss[0]) for x in dss[1:])


def test_every_limit_refuses():
    n_way, n_shot, Nq, d = 4, 2, 8, 256
    s3, q3, P, g = _episode(n_way, n_shot, Nq, d, 3)
    L, st = hip_lib()
    # every operand and output of a refused call lives in a buffer large enough for the largest size asked for, so a call
    # accepted by mistake would stay in bounds; the outputs keep their NaN sentinel
    big_n = 65 * 65 * 1028 + 64
    src = torch.randn(big_n, device="cuda")
    outs = [_nan(big_n) for _ in range(3)]
    for case in [dict(d=254), dict(d=0), dict(d=1028), dict(n_way=0), dict(n_way=65), dict(n_shot=0), dict(n_shot=65)]:
        nw, ns, dd = case.get("n_way", n_way), case.get("n_shot", n_shot), case.get("d", d)
        rc = L.mmf_fewshot_proto_fwd(ptr3([src] * 3), outs[0].data_ptr(), outs[1].data_ptr(), nw, ns, dd, st)
        rc2 = L.mmf_fewshot_proto_bwd(src.data_ptr(), None, outs[2].data_ptr(), nw, ns, dd, st)
        torch.cuda.synchronize()
        assert rc == MMF_E_SHAPE and rc2 == MMF_E_SHAPE, case
        assert all(bool(o.isnan().all()) for o in outs), case
    for case in [dict(d=254), dict(d=1028), dict(n_way=0), dict(n_way=65), dict(Nq=0), dict(Nq=1025)]:
        nq, nw, dd = case.get("Nq", Nq), case.get("n_way", n_way), case.get("d", d)
        rc = L.mmf_fewshot_dist_fwd(ptr3([src] * 3), src.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                    nq, nw, dd, st)
        rc2 = L.mmf_fewshot_dist_bwd(src.data_ptr(), src.data_ptr(), src.data_ptr(), src.data_ptr(), None, src.data_ptr(),
                                     outs[0].data_ptr(), outs[1].data_ptr(), nq, nw, dd, st)
        torch.cuda.synchronize()
        assert rc == MMF_E_SHAPE and rc2 == MMF_E_SHAPE, case
        assert all(bool(o.isnan().all()) for o in outs), case
    # null required pointers
    sf, mean = _nan(n_way * n_shot, d), _nan(n_way, d)
    assert L.mmf_fewshot_proto_fwd(ptr3([s3[0], None, s3[2]]), sf.data_ptr(), mean.data_ptr(), n_way, n_shot, d, st) == MMF_E_SHAPE
    assert L.mmf_fewshot_proto_fwd(None, sf.data_ptr(), mean.data_ptr(), n_way, n_shot, d, st) == MMF_E_SHAPE
    assert L.mmf_fewshot_proto_fwd(ptr3(s3), sf.data_ptr(), None, n_way, n_shot, d, st) == MMF_E_SHAPE
    assert L.mmf_fewshot_proto_bwd(None, None, sf.data_ptr(), n_way, n_shot, d, st) == MMF_E_SHAPE
    rc, qf, dist, pred = _dist_fwd(q3, P)
    assert rc == 0
    qf2, d2, p2 = _nan(Nq, d), _nan(Nq, n_way), _nan(Nq, n_way)
    assert L.mmf_fewshot_dist_fwd(ptr3(q3), None, qf2.data_ptr(), d2.data_ptr(), p2.data_ptr(), Nq, n_way, d, st) == MMF_E_SHAPE
    assert L.mmf_fewshot_dist_fwd(ptr3(q3), P.data_ptr(), qf2.data_ptr(), None, p2.data_ptr(), Nq, n_way, d, st) == MMF_E_SHAPE
    dq = _nan(Nq, d)
    assert L.mmf_fewshot_dist_bwd(qf.data_ptr(), P.data_ptr(), None, pred.data_ptr(), None, pred.data_ptr(), dq.data_ptr(),
                                  None, Nq, n_way, d, st) == MMF_E_SHAPE
    # misaligned feature rows
    assert L.mmf_fewshot_proto_fwd(ptr3([s3[0], src.data_ptr() + 4, s3[2]]), sf.data_ptr(), mean.data_ptr(), n_way, n_shot, d,
                                   st) == MMF_E_ALIGN
    torch.cuda.synchronize()
    assert all(bool(t.isnan().all()) for t in (sf, mean, qf2, d2, p2, dq))
    # the bindings refuse too, before any launch
    from mmfusion import small_ops
    with pytest.raises(ValueError):
        small_ops.fewshot_prototypes(*s3, n_way, n_shot + 1)
    with pytest.raises(ValueError):
        small_ops.fewshot_scores(*[torch.zeros(4, 254, device="cuda")] * 3, torch.zeros(3, 254, device="cuda"))
    with pytest.raises(RuntimeError):
        small_ops.fewshot_prototypes(*[x.cpu() for x in s3], n_way, n_shot)


# ------------------------------------------------------------------------------------------------------------------------
# the wrapper
# ------------------------------------------------------------------------------------------------------------------------
def _cfg(d=256, heads=4, dropout=0.0, precision=None):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = True
    cfg.fusion_type = "hierarchical"
    cfg.fusion_hidden_size, cfg.fusion_num_heads = d, heads
    cfg.graph_hidden_size, cfg.graph_num_layers = d, 3
    cfg.fusion_dropout = cfg.graph_dropout = dropout
    if precision:
        cfg.fusion_precision = precision
    return cfg


def _model(d=256, heads=4, dropout=0.0, modality_dropout=0.0, seed=5, **kw):
    from models.multimodal_model import FewShotModel, MultimodalEmotionModel
    torch.manual_seed(seed)
    cfg = _cfg(d, heads, dropout, **kw)
    m = FewShotModel(MultimodalEmotionModel(cfg), cfg).cuda().train()
    m.base_model.modality_dropout.dropout_rate = modality_dropout
    return m


def _data(B, seed):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, 9, 768, generator=g).cuda()
    audio = torch.randn(B, 21, 768, generator=g).cuda()
    video = torch.randn(B, 6, 768, generator=g).cuda()
    return {"text": {"input_ids": text, "attention_mask": torch.ones(B, 9, dtype=torch.long).cuda()}, "audio": audio,
            "video": video}


def _triple(x):
    return x["text"], x["audio"], x["video"]


def _episode_data(n_way=7, n_shot=5, Nq=16, seed=1):
    sup, qry = _data(n_way * n_shot, seed), _data(Nq, seed + 1)
    y = torch.randint(0, n_way, (Nq,), generator=torch.Generator().manual_seed(seed + 2)).cuda()
    return sup, qry, y


def _torch_head(self, support, query, n_way, n_shot):
    """FewShotModel.head with the fused kernels replaced by the reference's torch ops (sum, mean, cdist, softmax); the
    prototype MLP stays on the same row linear as in the model"""
    from mmfusion import ops
    from mmfusion.ops import W
    sf = support[0].float() + support[1].float() + support[2].float()
    mean = sf.view(n_way, n_shot, -1).mean(1)
    l0, l2 = self.prototype_network[0], self.prototype_network[2]
    h = ops.linear(mean, W(l0.weight), W(l0.bias), relu=True, out_f32=True)
    prototypes = ops.linear(h, W(l2.weight), W(l2.bias), out_f32=True)
    qf = query[0].float() + query[1].float() + query[2].float()
    distances = torch.cdist(qf, prototypes, p=2)
    return sf, prototypes, qf, distances, torch.softmax(-distances, dim=-1)


def test_head_fp32_mode_against_float64():
    """The head, prototype MLP included, in the fp32 parity mode on given features: outputs and every gradient (features
    and prototype_network) against float64 autograd of the reference formulation."""
    from mmfusion import arena as arena_mod, ops
    from fewshot_ref import torch_head
    for n_way, n_shot, d in ((7, 5, 256), (7, 1, 512), (3, 4, 256)):
        model = _model(d, 4, precision="fp32")
        ar = arena_mod.ensure(model)
        Nq = 16
        g = torch.Generator().manual_seed(d + n_shot)
        s3 = [torch.randn(n_way * n_shot, d, generator=g).cuda().requires_grad_(True) for _ in range(3)]
        q3 = [torch.randn(Nq, d, generator=g).cuda().requires_grad_(True) for _ in range(3)]
        gpred, gdist = torch.randn(Nq, n_way, generator=g).cuda(), torch.randn(Nq, n_way, generator=g).cuda()
        ar.zero_grad()
        old = ops.set_precision("fp32")
        try:
            sf, P, qf, dist, pred = model.head(s3, q3, n_way, n_shot)
        finally:
            ops.set_precision(old)
        ((gpred * pred).sum() + (gdist * dist).sum()).backward()
        torch.cuda.synchronize()
        pn = model.prototype_network
        params = [pn[0].weight, pn[0].bias, pn[2].weight, pn[2].bias]
        leaves = [x.detach().double().cpu().requires_grad_(True) for x in (*s3, *q3, *params)]
        r = torch_head(leaves[0:3], leaves[3:6], *leaves[6:10], n_way, n_shot)
        ((gpred.double().cpu() * r[4]).sum() + (gdist.double().cpu() * r[3]).sum()).backward()
        for name, got, want in zip(("sf", "P", "qf", "dist", "pred"), (sf, P, qf, dist, pred), r):
            e = float((got.detach().double().cpu() - want.detach()).abs().max()) / max(1.0, float(want.detach().abs().max()))
            assert e <= 1e-5, f"n_way={n_way} n_shot={n_shot} d={d}: {name} err {e:.3e}"
        for i, (got, leaf) in enumerate(zip([x.grad for x in (*s3, *q3)] + [p.grad for p in params], leaves)):
            e = l2_rel(got.detach().double().cpu(), leaf.grad)
            assert e <= 1e-5, f"n_way={n_way} n_shot={n_shot} d={d}: grad {i} rel L2 {e:.3e}"


@pytest.mark.parametrize("n_shot", [1, 5])
def test_eval_outputs_match_base_model_features(n_shot):
    from fewshot_ref import torch_head
    model = _model(512, 8).eval()
    n_way = 7
    sup, qry, _ = _episode_data(n_way, n_shot, 16, seed=n_shot)
    with torch.no_grad():
        out = model(sup, qry, n_way, n_shot)
        bs = model.base_model(sup["text"], sup["audio"], sup["video"], use_adapter=True, use_prompt=True)
        bq = model.base_model(qry["text"], qry["audio"], qry["video"], use_adapter=True, use_prompt=True)
    torch.cuda.synchronize()
    assert set(out) == {"predictions", "distances", "prototypes", "support_features", "query_features"}
    want_s = bs["text_features"] + bs["audio_features"] + bs["video_features"]
    want_q = bq["text_features"] + bq["audio_features"] + bq["video_features"]
    assert torch.equal(out["support_features"], want_s) and torch.equal(out["query_features"], want_q)
    pn = model.prototype_network
    cv = lambda t: t.detach().double().cpu()
    sf, P, qf, dist, pred = torch_head([cv(want_s), 0, 0], [cv(want_q), 0, 0], cv(pn[0].weight), cv(pn[0].bias),
                                       cv(pn[2].weight), cv(pn[2].bias), n_way, n_shot)
    # the prototype MLP runs on the bf16 row linear: bf16-level tolerance from there on
    assert l2_rel(cv(out["prototypes"]), P) <= 2e-2
    assert l2_rel(cv(out["distances"]), dist) <= 2e-2
    assert float((cv(out["predictions"]) - pred).abs().max()) <= 2e-2
    # ... and f32-tight from the kernel's own prototypes
    r2 = dist_fwd(out["query_features"], out["prototypes"])
    assert bool(((cv(out["distances"]) - r2["dist"]).abs() <= r2["e_dist"]).all())
    assert torch.allclose(out["predictions"].sum(-1).cpu(), torch.ones(16), atol=1e-6)


def _collect_grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


# The video adapter sits in front of the frozen BiLSTM: its gradient goes back through 30 recurrent steps whose dG is
# narrowed to bf16, which turns the f32 rounding differences of the head's input gradients into bf16-level ones (rel L2
# measured 7.7e-4 with dropout on, up to 3.4e-3 with it off).  It is held to 1e-2; every other reached gradient to 1e-3
# (measured: at most 5.5e-4; prototype_network 1e-7).
VIDEO_ADAPTER_TOL, STEP_GRAD_TOL = 1e-2, 1e-3


def test_step_gradients_match_torch_head(monkeypatch):
    from models.multimodal_model import FewShotModel
    from mmfusion.train import FewShotTrainStep
    model = _model(512, 8, dropout=0.1, modality_dropout=0.1)
    sup, qry, y = _episode_data(7, 5, 16)
    ts = FewShotTrainStep(model, 7, 5, lr=1e-3)
    from mmfusion import ops, small_ops

    def fwd_bwd():
        ts.arena.zero_grad()                                     # a full memset: torch accumulates into the arena views
        out = model(sup, qry, 7, 5)
        loss = small_ops.fusion_loss(out["predictions"], y, 0.0, [], [])
        small_ops.backward_from(loss)
        ts.arena.finalize_grads()
        return loss

    st0 = ops.rng_state().clone()
    loss = fwd_bwd()
    torch.cuda.synchronize()
    got = _collect_grads(model)
    ops.rng_state().copy_(st0)                                   # the same dropout masks for the torch-head run
    monkeypatch.setattr(FewShotModel, "head", _torch_head)
    lt = fwd_bwd()
    torch.cuda.synchronize()
    monkeypatch.undo()
    want = _collect_grads(model)
    assert abs(loss.item() - lt.item()) <= 1e-5 * max(1.0, abs(lt.item()))
    reached = {id(p) for p in ts.reached}
    worst, checked = (0.0, ""), 0
    for n, p in model.named_parameters():
        if id(p) not in reached:
            assert not bool(got[n].any()), f"{n}: gradient outside the reached set"
            continue
        assert float(want[n].norm()) > 0.0, f"{n}: reached but no gradient"
        e = l2_rel(got[n], want[n])
        checked += 1
        print(f"  {n}: rel L2 {e:.3e}")
        assert e <= (VIDEO_ADAPTER_TOL if n.startswith("base_model.video_encoder.adapter.") else STEP_GRAD_TOL), \
            f"{n}: rel L2 {e:.3e}"
        if e > worst[0]:
            worst = (e, n)
    print(f"few-shot step vs torch head: {checked} reached parameter gradients, worst rel L2 {worst[0]:.3e} ({worst[1]})")
    assert checked == len(ts.reached)


def test_step_updates_reached_parameters_only_and_queues_no_frozen_wgrad():
    from mmfusion import ops
    from mmfusion.train import FewShotTrainStep
    model = _model(256, 4, dropout=0.1, modality_dropout=0.1)
    sup, qry, y = _episode_data(7, 5, 16)
    ts = FewShotTrainStep(model, 7, 5, lr=1e-3)
    assert ts.opt.ranges is not None and ts.opt.max_grad_norm is None and ts.opt.weight_decay == 0.01
    assert abs(float(ts.opt.hparams[0]) - 1e-3) <= 1e-9 and abs(float(ts.opt.hparams[1]) - 0.9) <= 1e-7
    s0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    reached = {id(p) for p in ts.reached}
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and all(id(p) not in reached for n, p in model.named_parameters() if n in frozen)
    for _ in range(3):
        ts(_triple(sup), _triple(qry), y)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if id(p) in reached:
            assert not torch.equal(p.detach(), s0[n]), f"{n}: reached but did not move"
        else:
            assert torch.equal(p.detach(), s0[n]), f"{n}: not reached but moved"
            assert not bool(p.grad.any()), f"{n}: not reached but has an arena gradient"
    # which weight gradients the backward queues: the reached matrices only
    grad_of = {p.grad.data_ptr(): n for n, p in model.named_parameters() if p.grad is not None and p.dim() == 2}
    ops.set_manual_wgrad_flush(True)
    try:
        ts.fwd_bwd(_triple(sup), _triple(qry), y)
        pend = ops.take_pending_wgrad()
        ops.issue_wgrad(pend)
    finally:
        ops.set_manual_wgrad_flush(False)
    torch.cuda.synchronize()
    targets = {grad_of.get(q[2].data_ptr(), f"<unknown {q[2].data_ptr()}>") for q in pend}
    reached_names = {n for n, p in model.named_parameters() if id(p) in reached and p.dim() == 2}
    assert targets == reached_names, f"queued for frozen weights: {sorted(targets - reached_names)}"
    # the loss falls on a fixed episode (dropout off)
    model2 = _model(256, 4, seed=6)
    ts2 = FewShotTrainStep(model2, 7, 5, lr=1e-3)
    ls = [ts2(_triple(sup), _triple(qry), y).item() for _ in range(10)]
    assert ls[-1] < ls[0], ls


def test_fewshot_step_graph_replay_matches_eager():
    """Three FewShotTrainStep steps (dropout and ModalityDropout on) captured as one single-chain graph and replayed,
    against three eager steps from the same state: loss, gradient arena, parameters."""
    from mmfusion.train import FewShotTrainStep
    model = _model(256, 4, dropout=0.1, modality_dropout=0.1)
    sup, qry, y = _episode_data(7, 5, 16)
    ts = FewShotTrainStep(model, 7, 5, lr=1e-3)
    check_graph_replay_matches_eager(lambda: ts(_triple(sup), _triple(qry), y), ts.arena, ts.opt)


def test_checkpoint_round_trip(tmp_path):
    from models.multimodal_model import FewShotModel, MultimodalEmotionModel
    from mmfusion.train import FewShotTrainStep, load_checkpoint, save_checkpoint
    model = _model(256, 4)
    sup, qry, y = _episode_data(7, 5, 16)
    ts = FewShotTrainStep(model, 7, 5, lr=1e-3)
    for _ in range(2):
        ts(_triple(sup), _triple(qry), y)
    path = str(tmp_path / "fewshot.pt")
    save_checkpoint(path, model, ts.opt, epoch=1, config=model.config)
    torch.manual_seed(99)
    fresh = FewShotModel(MultimodalEmotionModel(model.config), model.config).cuda()
    ts2 = FewShotTrainStep(fresh, 7, 5, lr=1e-3)
    load_checkpoint(path, fresh, ts2.opt)
    model.eval(), fresh.eval()
    with torch.no_grad():
        a, b = model(sup, qry, 7, 5), fresh(sup, qry, 7, 5)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ts.opt.exp_avg, ts2.opt.exp_avg) and torch.equal(ts.opt.exp_avg_sq, ts2.opt.exp_avg_sq)
    assert ts2.opt.t == ts.opt.sync_step()


def test_base_model_with_its_own_arena_moves_into_the_wrapper():
    from models.multimodal_model import FewShotModel, MultimodalEmotionModel
    from mmfusion import arena as arena_mod
    cfg = _cfg(256, 4)
    torch.manual_seed(3)
    base = MultimodalEmotionModel(cfg).cuda().eval()
    own = arena_mod.ensure(base)
    sup, qry, _ = _episode_data(3, 2, 4)
    with torch.no_grad():
        want = base(sup["text"], sup["audio"], sup["video"], use_adapter=True, use_prompt=True)
    model = FewShotModel(base, cfg).cuda().eval()
    with torch.no_grad():
        out = model(sup, qry, 3, 2)
    ar = arena_mod.ensure(model)
    assert ar is not own and all(getattr(p, "_mmf_arena", None) is ar for p in model.parameters())
    assert torch.equal(out["support_features"], want["text_features"] + want["audio_features"] + want["video_features"])
