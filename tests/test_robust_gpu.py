"""RobustMultimodalModel on the MI355X: the robust head kernels of csrc/small.hip against the float64 restatement of
tests/robust_ref.py (per-element f32 error bounds, worst error reported as a fraction of its bound), their refusals, the
head in the fp32 parity mode, the wrapper in eval mode against the plain base model, and ``mmfusion.train.RobustTrainStep``
(gradients against the torch formulation of the head, which parameters it steps, graph replay, checkpoints)."""

import pytest
import torch

from helpers import check_graph_replay_matches_eager, hip_lib, l2_rel, ptr3, within_bound
from robust_ref import head_bwd, head_fwd, torch_head

pytestmark = pytest.mark.gpu

MMF_E_SHAPE, MMF_E_ALIGN = -1, -3
NAMES = ("text", "audio", "video")


def _operands(B, d, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    f = [torch.randn(B, d, generator=g).cuda() for _ in range(3)]
    h = torch.relu(torch.randn(B, d, generator=g)).cuda()
    W2 = (torch.randn(3, d, generator=g) * 2 / d ** 0.5).cuda()
    b2 = torch.randn(3, generator=g).cuda()
    Wm = [(torch.randn(Cn, d, generator=g) / d ** 0.5).cuda() for _ in range(3)]
    bm = [torch.randn(Cn, generator=g).cuda() for _ in range(3)]
    return f, h, W2, b2, Wm, bm


def _fwd(f, h, W2, b2, Wm, bm, avail, B=None, d=None, Cn=None):
    L, st = hip_lib()
    B0, d0 = h.shape
    C0 = Wm[0].shape[0]
    a = torch.full((B0, 3), float("nan"), device="cuda")
    p = [torch.full((B0, C0), float("nan"), device="cuda") for _ in range(3)]
    wn = torch.full((B0, 3), float("nan"), device="cuda")
    y = torch.full((B0, C0), float("nan"), device="cuda")
    rc = L.mmf_robust_head_fwd(ptr3(f), h.data_ptr() if h is not None else None, W2.data_ptr(), b2.data_ptr(), ptr3(Wm), ptr3(bm),
                               avail, a.data_ptr(), ptr3(p), wn.data_ptr(), y.data_ptr(),
                               B0 if B is None else B, d0 if d is None else d, C0 if Cn is None else Cn, st)
    return rc, a, p, wn, y


def _bwd(f, h, W2, Wm, a, p, wn, avail, g, dP, dA, dN, want_df, want_dh, init, B=None, Cn=None):
    L, st = hip_lib()
    B0, d = h.shape
    C0 = Wm[0].shape[0]
    df = [torch.full((B0, d), float("nan"), device="cuda") if want_df[m] else None for m in range(3)]
    dh = torch.full((B0, d), float("nan"), device="cuda") if want_dh else None
    dW2, db2 = init["dW2"].clone(), init["db2"].clone()
    dWm, dbm = [x.clone() for x in init["dWm"]], [x.clone() for x in init["dbm"]]
    rc = L.mmf_robust_head_bwd(ptr3(f), h.data_ptr(), W2.data_ptr(), ptr3(Wm), a.data_ptr(), ptr3(p), wn.data_ptr(), avail,
                               g.data_ptr() if g is not None else None, ptr3(dP) if dP is not None else None,
                               dA.data_ptr() if dA is not None else None, dN.data_ptr() if dN is not None else None,
                               ptr3(df), dh.data_ptr() if dh is not None else None, dW2.data_ptr(), db2.data_ptr(),
                               ptr3(dWm), ptr3(dbm), B0 if B is None else B, d, C0 if Cn is None else Cn, st)
    return rc, {"df": df, "dh": dh, "dW2": dW2, "db2": db2, "dWm": dWm, "dbm": dbm}


# ------------------------------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------------------------------
GRAD_SETS = {"y": ("y",), "all": ("y", "P", "A", "N"), "p_a": ("y", "P", "A"), "n_only": ("y", "N")}


def test_robust_head_kernels_against_float64():
    worst_f, worst_b = [0.0, ""], [0.0, ""]
    cases = 0
    for Cn in (3, 7, 16):
        for d in (256, 512, 768):
            for B in (1, 16, 256):
                seed = 100 * Cn + d + B
                f, h, W2, b2, Wm, bm = _operands(B, d, Cn, seed)
                for avail in (-1, 0b011, 0, 0b100, 0b111):
                    label = f"C={Cn} d={d} B={B} avail={avail}"
                    rc, a, p, wn, y = _fwd(f, h, W2, b2, Wm, bm, avail)
                    torch.cuda.synchronize()
                    assert rc == 0, label
                    ref = head_fwd(f, h, W2, b2, Wm, bm, avail)
                    within_bound(a, ref["a"], ref["ea"], label + " a", worst_f)
                    for m in range(3):
                        within_bound(p[m], ref["p"][m], ref["ep"][m], label + f" p{m}", worst_f)
                    within_bound(wn, ref["wn"], ref["ewn"], label + " wn", worst_f)
                    within_bound(y, ref["y"], ref["ey"], label + " y", worst_f)
                    if avail >= 0:
                        n = bin(avail).count("1")
                        want = torch.tensor([[((avail >> i) & 1) / n if n else 0.0 for i in range(3)]], dtype=torch.float32)
                        assert torch.equal(wn.cpu(), want.expand(B, 3)), f"{label}: given-mask weights not exactly 1/n"
                    gsets = GRAD_SETS if (d == 512 or B == 16) else {"all": GRAD_SETS["all"]}
                    for gname, gs in gsets.items():
                        gen = torch.Generator().manual_seed(seed + len(gname))
                        rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
                        g = rnd(B, Cn)
                        dP = [rnd(B, Cn), None, rnd(B, Cn)] if "P" in gs else None
                        dA = rnd(B, 3) if "A" in gs else None
                        dN = rnd(B, 3) if "N" in gs else None
                        want_df = (True, gname != "n_only", True)
                        init = {"dW2": rnd(3, d), "db2": rnd(3), "dWm": [rnd(Cn, d) for _ in range(3)],
                                "dbm": [rnd(Cn) for _ in range(3)]}
                        rc, out = _bwd(f, h, W2, Wm, a, p, wn, avail, g, dP, dA, dN, want_df, True, init)
                        torch.cuda.synchronize()
                        assert rc == 0, label
                        rb = head_bwd(f, h, W2, Wm, a, p, wn, g, dP, dA, dN if avail < 0 else None, avail)
                        lab = f"{label} grads={gname}"
                        U = 2.0 ** -24
                        for m in range(3):
                            if want_df[m]:
                                within_bound(out["df"][m], rb["df"][m], rb["e_df"][m], lab + f" df{m}", worst_b)
                            acc = init["dWm"][m].double().cpu() + rb["dWm"][m]
                            within_bound(out["dWm"][m], acc, rb["e_dWm"][m] + U * acc.abs(), lab + f" dW{m}", worst_b)
                            acc = init["dbm"][m].double().cpu() + rb["dbm"][m]
                            within_bound(out["dbm"][m], acc, rb["e_dbm"][m] + U * acc.abs(), lab + f" db{m}", worst_b)
                        within_bound(out["dh"], rb["dh"], rb["e_dh"], lab + " dh", worst_b)
                        acc = init["dW2"].double().cpu() + rb["dW2"]
                        within_bound(out["dW2"], acc, rb["e_dW2"] + U * acc.abs(), lab + " dW2", worst_b)
                        acc = init["db2"].double().cpu() + rb["db2"]
                        within_bound(out["db2"], acc, rb["e_db2"] + U * acc.abs(), lab + " db2", worst_b)
                        if avail >= 0 and dA is None:
                            assert not bool(out["dh"].any()), f"{lab}: a given mask sent gradient to the predictor"
                        cases += 1
    print(f"robust head: {cases} backward cases; worst error / bound: forward {worst_f[0]:.3e} ({worst_f[1]}), "
          f"backward {worst_b[0]:.3e} ({worst_b[1]})")


def test_robust_head_backward_is_deterministic():
    f, h, W2, b2, Wm, bm = _operands(64, 512, 7, 9)
    _, a, p, wn, _ = _fwd(f, h, W2, b2, Wm, bm, -1)
    g = torch.randn(64, 7, device="cuda")
    init = {"dW2": torch.zeros(3, 512, device="cuda"), "db2": torch.zeros(3, device="cuda"),
            "dWm": [torch.zeros(7, 512, device="cuda") for _ in range(3)], "dbm": [torch.zeros(7, device="cuda") for _ in range(3)]}
    outs = [_bwd(f, h, W2, Wm, a, p, wn, -1, g, None, None, None, (True,) * 3, True, init)[1] for _ in range(2)]
    torch.cuda.synchronize()
    for k in ("dh", "dW2", "db2"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    for k in ("df", "dWm", "dbm"):
        assert all(torch.equal(x, y) for x, y in zip(outs[0][k], outs[1][k])), k


def test_robust_head_refuses_bad_arguments():
    B, d, Cn = 4, 256, 7
    f, h, W2, b2, Wm, bm = _operands(B, d, Cn, 1)
    # forward: every output keeps its NaN sentinel
    bad_fwd = [dict(Cn=0, rc=MMF_E_SHAPE), dict(Cn=17, rc=MMF_E_SHAPE), dict(B=0, rc=MMF_E_SHAPE), dict(B=257, rc=MMF_E_SHAPE),
               dict(d=254, rc=MMF_E_SHAPE), dict(d=0, rc=MMF_E_SHAPE), dict(avail=8, rc=MMF_E_SHAPE),
               dict(avail=-2, rc=MMF_E_SHAPE), dict(h=None, rc=MMF_E_SHAPE), dict(f1=None, rc=MMF_E_SHAPE),
               dict(f1="mis", rc=MMF_E_ALIGN), dict(W="mis", rc=MMF_E_ALIGN)]
    big = torch.randn((B + Cn) * d + 64, device="cuda")          # large enough for a wrongly accepted call to stay in bounds
    for case in bad_fwd:
        ff = list(f)
        Ww = list(Wm)
        if case.get("f1", 0) is None:
            ff[1] = None
        elif case.get("f1") == "mis":
            ff[1] = big.data_ptr() + 4
        if case.get("W") == "mis":
            Ww = [Wm[0], big.data_ptr() + 8, Wm[2]]
        hh = None if "h" in case else h
        L, st = hip_lib()
        a = torch.full((B, 3), float("nan"), device="cuda")
        p = [torch.full((B, Cn), float("nan"), device="cuda") for _ in range(3)]
        wn = torch.full((B, 3), float("nan"), device="cuda")
        y = torch.full((B, Cn), float("nan"), device="cuda")
        rc = L.mmf_robust_head_fwd(ptr3(ff), hh.data_ptr() if hh is not None else None, W2.data_ptr(), b2.data_ptr(), ptr3(Ww),
                                   ptr3(bm), case.get("avail", -1), a.data_ptr(), ptr3(p), wn.data_ptr(), y.data_ptr(),
                                   case.get("B", B), case.get("d", d), case.get("Cn", Cn), st)
        torch.cuda.synchronize()
        assert rc == case["rc"], case
        assert all(bool(t.isnan().all()) for t in (a, *p, wn, y)), case
    # null outputs / biases in the forward
    L, st = hip_lib()
    for which in ("a", "y", "b2"):
        a, y = torch.full((B, 3), float("nan"), device="cuda"), torch.full((B, Cn), float("nan"), device="cuda")
        p = [torch.full((B, Cn), float("nan"), device="cuda") for _ in range(3)]
        wn = torch.full((B, 3), float("nan"), device="cuda")
        rc = L.mmf_robust_head_fwd(ptr3(f), h.data_ptr(), W2.data_ptr(), None if which == "b2" else b2.data_ptr(), ptr3(Wm), ptr3(bm),
                                   -1, None if which == "a" else a.data_ptr(), ptr3(p), wn.data_ptr(),
                                   None if which == "y" else y.data_ptr(), B, d, Cn, st)
        torch.cuda.synchronize()
        assert rc == MMF_E_SHAPE and all(bool(t.isnan().all()) for t in (a, *p, wn, y)), which
    # backward: refused calls leave every gradient output (sentinel-filled) untouched
    rc, a, p, wn, _ = _fwd(f, h, W2, b2, Wm, bm, -1)
    assert rc == 0
    g = torch.randn(B, Cn, device="cuda")
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    init = {"dW2": nan(3, d), "db2": nan(3), "dWm": [nan(Cn, d) for _ in range(3)], "dbm": [nan(Cn) for _ in range(3)]}
    for case in (dict(B=257), dict(B=0), dict(Cn=17), dict(avail=9), dict(g=None)):
        rc, out = _bwd(f, h, W2, Wm, a, p, wn, case.get("avail", -1), None if "g" in case else g, None, None, None,
                       (True,) * 3, True, init, B=case.get("B"), Cn=case.get("Cn"))
        torch.cuda.synchronize()
        assert rc == MMF_E_SHAPE, case
        for k, v in out.items():
            vs = v if isinstance(v, list) else [v]
            assert all(bool(t.isnan().all()) for t in vs), (case, k)
    # a null parameter gradient is refused too
    dW2 = nan(3, d)
    dh = nan(B, d)
    rc = L.mmf_robust_head_bwd(ptr3(f), h.data_ptr(), W2.data_ptr(), ptr3(Wm), a.data_ptr(), ptr3(p), wn.data_ptr(), -1,
                               g.data_ptr(), None, None, None, None, dh.data_ptr(), dW2.data_ptr(), None,
                               ptr3(init["dWm"]), ptr3(init["dbm"]), B, d, Cn, st)
    torch.cuda.synchronize()
    assert rc == MMF_E_SHAPE and bool(dh.isnan().all()) and bool(dW2.isnan().all())


# ------------------------------------------------------------------------------------------------------------------------
# the wrapper
# ------------------------------------------------------------------------------------------------------------------------
def _cfg(d=256, heads=4, G=256, dropout=0.0, precision=None, C=7):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = True
    cfg.fusion_type = "hierarchical"
    cfg.fusion_hidden_size, cfg.fusion_num_heads = d, heads
    cfg.graph_hidden_size, cfg.graph_num_layers = G, 3
    cfg.fusion_dropout = cfg.graph_dropout = dropout
    cfg.num_emotions = C
    if precision:
        cfg.fusion_precision = precision
    return cfg


def _model(d=256, heads=4, dropout=0.0, modality_dropout=0.0, seed=5, **kw):
    from models.multimodal_model import RobustMultimodalModel
    torch.manual_seed(seed)
    m = RobustMultimodalModel(_cfg(d, heads, d, dropout, **kw)).cuda().train()
    m.base_model.modality_dropout.dropout_rate = modality_dropout
    return m


def _cuda_inputs(B, seed=1234):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, 9, 768, generator=g).cuda()
    audio = torch.randn(B, 21, 768, generator=g).cuda()
    video = torch.randn(B, 6, 768, generator=g).cuda()
    mask = torch.ones(B, 9, dtype=torch.long).cuda()
    labels = torch.randint(0, 7, (B,), generator=torch.Generator().manual_seed(7)).cuda()
    return {"input_ids": text, "attention_mask": mask}, audio, video, labels


def _head_params(model, dtype=torch.float64):
    cv = lambda t: t.detach().to(dtype).cpu()
    l0, l2 = model.modality_predictor[0], model.modality_predictor[2]
    heads = (model.text_only_classifier, model.audio_only_classifier, model.video_only_classifier)
    return (cv(l0.weight), cv(l0.bias), cv(l2.weight), cv(l2.bias), [cv(l.weight) for l in heads], [cv(l.bias) for l in heads])


def test_head_fp32_mode_against_float64():
    """The whole head, hidden layer included, in the fp32 parity mode on given features: outputs and every gradient
    (features and head parameters) against float64 autograd of the reference formulation."""
    from mmfusion import arena as arena_mod, ops
    for d, avail in ((256, None), (512, ["text", "video"]), (256, ["audio"])):
        model = _model(d, 4, precision="fp32")
        ar = arena_mod.ensure(model)
        B = 16
        g = torch.Generator().manual_seed(d)
        f = [torch.randn(B, d, generator=g).cuda().requires_grad_(True) for _ in range(3)]
        gy = torch.randn(B, 7, generator=g).cuda()
        gp = torch.randn(B, 7, generator=g).cuda()
        ga = torch.randn(B, 3, generator=g).cuda()
        ar.zero_grad()
        old = ops.set_precision("fp32")
        try:
            a, pt, pa, pv, wn, y = model.head(*f, avail)
        finally:
            ops.set_precision(old)
        loss = (gy * y).sum() + (gp * pa).sum() + (ga * a).sum()
        loss.backward()
        torch.cuda.synchronize()
        W1, b1, W2, b2, Wm, bm = _head_params(model)
        leaves = [x.detach().double().cpu().requires_grad_(True) for x in (*f, W1, b1, W2, b2, *Wm, *bm)]
        lf = leaves[:3]
        h = torch.relu(torch.cat(lf, -1) @ leaves[3].T + leaves[4])
        ra, rp, rw, ry = torch_head(lf, h, leaves[5], leaves[6], leaves[7:10], leaves[10:13], avail)
        rl = (gy.double().cpu() * ry).sum() + (gp.double().cpu() * rp[1]).sum() + (ga.double().cpu() * ra).sum()
        rl.backward()
        for name, got, want in (("a", a, ra), ("p_t", pt, rp[0]), ("p_a", pa, rp[1]), ("p_v", pv, rp[2]), ("wn", wn, rw),
                                ("y", y, ry)):
            e = float((got.detach().double().cpu() - want.detach()).abs().max()) / max(1.0, float(want.detach().abs().max()))
            assert e <= 1e-5, f"d={d} avail={avail}: {name} err {e:.3e}"
        params = [model.modality_predictor[0].weight, model.modality_predictor[0].bias, model.modality_predictor[2].weight,
                  model.modality_predictor[2].bias, model.text_only_classifier.weight, model.audio_only_classifier.weight,
                  model.video_only_classifier.weight, model.text_only_classifier.bias, model.audio_only_classifier.bias,
                  model.video_only_classifier.bias]
        gots = [x.grad for x in f] + [p.grad for p in params]
        for i, (got, leaf) in enumerate(zip(gots, leaves)):
            want = leaf.grad
            if float(want.abs().max()) == 0.0:
                assert got is None or float(got.abs().max()) == 0.0, f"d={d} avail={avail}: grad {i} should be zero"
                continue
            e = l2_rel(got.detach().double().cpu(), want)
            assert e <= 1e-5, f"d={d} avail={avail}: grad {i} rel L2 {e:.3e}"


@pytest.mark.parametrize("missing", [[], ["text"], ["audio"], ["video"], ["text", "audio"], ["text", "video"],
                                     ["audio", "video"]], ids=lambda m: "all" if not m else "_".join(m) + "_missing")
def test_wrapper_eval_matches_base_model_and_float64(missing):
    from models.multimodal_model import MultimodalEmotionModel
    model = _model(512, 8).eval()
    plain = MultimodalEmotionModel(model.config).cuda().eval()
    plain.load_state_dict(model.base_model.state_dict())
    ti, au, vi, _ = _cuda_inputs(16)
    keep = [ti["input_ids"].clone(), ti["attention_mask"].clone(), au.clone(), vi.clone()]
    available = [m for m in NAMES if m not in missing]
    with torch.no_grad():
        out = model(ti, au, vi, missing_modalities=missing)
        out_given = model(ti, au, vi, available_modalities=available, missing_modalities=missing)
        base = plain(ti, au, vi, missing_modalities=missing)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(keep, [ti["input_ids"], ti["attention_mask"], au, vi])), "inputs modified"
    for k, v in base.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(out[k], v) and torch.equal(out_given[k], v), k
        elif isinstance(v, dict):
            assert all(torch.equal(out[k][j], v[j]) for j in v), k
    feats = [out[f"{m}_features"] for m in NAMES]
    W1, b1, W2, b2, Wm, bm = _head_params(model)
    mask = sum(1 << i for i, m in enumerate(NAMES) if m in available)
    # given weights: exact constants, robust_prediction from the f32 modality predictions
    ref = head_fwd(feats, torch.zeros(16, 512), W2, b2, Wm, bm, mask)
    assert torch.equal(out_given["modality_weights"].cpu().double(), ref["wn"].float().double())
    e = (out_given["robust_prediction"].double().cpu() - ref["y"]).abs()
    assert bool((e <= ref["ey"]).all()), f"{missing}: robust_prediction err {float(e.max()):.3e}"
    for i, m in enumerate(NAMES):
        e = (out_given["individual_predictions"][m].double().cpu() - ref["p"][i]).abs()
        assert bool((e <= ref["ep"][i]).all()), m
    # predicted weights: the hidden layer runs on the bf16 row linear, so the availability carries bf16-level error
    h = torch.relu(torch.cat([x.double().cpu() for x in feats], -1) @ W1.T + b1)
    ra, rp, rw, ry = torch_head([x.double().cpu() for x in feats], h, W2, b2, Wm, bm, None)
    assert float((out["modality_availability"].double().cpu() - ra).abs().max()) <= 2e-2
    assert float((out["modality_weights"].double().cpu() - rw).abs().max()) <= 2e-2
    assert l2_rel(out["robust_prediction"].double().cpu(), ry) <= 2e-2
    # ... and against float64 from the kernel's own availability: f32-exact
    rw2 = out["modality_availability"].double().cpu()
    rw2 = rw2 / (rw2.sum(dim=1, keepdim=True) + 1e-8)
    assert float((out["modality_weights"].double().cpu() - rw2).abs().max()) <= 1e-6
    ry2 = sum(rw2[:, i:i + 1] * rp[i] for i in range(3))
    assert float((out["robust_prediction"].double().cpu() - ry2).abs().max()) <= 1e-5 * max(1.0, float(ry2.abs().max()))


def _torch_robust_head(f_t, f_a, f_v, h, module, available=None):
    """the head in plain torch ops over the same parameters (what the reference runs after its hidden layer)"""
    heads = (module.text_only_classifier, module.audio_only_classifier, module.video_only_classifier)
    l2 = module.modality_predictor[2]
    if isinstance(available, int):
        available = None if available < 0 else [m for i, m in enumerate(NAMES) if (available >> i) & 1]
    a, p, w, y = torch_head([f_t.float(), f_a.float(), f_v.float()], h, l2.weight, l2.bias,
                            [l.weight for l in heads], [l.bias for l in heads], available)
    return a, p[0], p[1], p[2], w, y


@pytest.mark.parametrize("missing", [None, ["video"]], ids=["all", "video_missing"])
def test_step_gradients_match_torch_head(monkeypatch, missing):
    from mmfusion import small_ops
    from mmfusion.train import RobustTrainStep
    model = _model(512, 8)
    ti, au, vi, labels = _cuda_inputs(16)
    ts = RobustTrainStep(model, lr=1e-3)
    loss = ts.fwd_bwd(ti, au, vi, labels, missing_modalities=missing)
    torch.cuda.synchronize()
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    monkeypatch.setattr(small_ops, "robust_head", _torch_robust_head)
    lt = ts.fwd_bwd(ti, au, vi, labels, missing_modalities=missing)
    torch.cuda.synchronize()
    monkeypatch.undo()
    want = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    assert abs(float(loss) - float(lt)) <= 1e-6 * max(1.0, abs(float(lt)))
    reached = {id(p) for p in ts.reached}
    worst, checked = (0.0, ""), 0
    for n, p in model.named_parameters():
        if id(p) not in reached:
            assert not bool(got[n].any()) and not bool(want[n].any()), f"{n}: gradient outside the reached set"
            continue
        if float(want[n].norm()) == 0.0:                   # (a weight that only multiplies a zeroed input)
            assert missing and not bool(got[n].any()), f"{n}: reached but no gradient"
            continue
        e = l2_rel(got[n], want[n])
        checked += 1
        if e > worst[0]:
            worst = (e, n)
    print(f"step vs torch head: {checked} reached parameter gradients, worst rel L2 {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= 1e-4, f"{worst[1]}: rel L2 {worst[0]:.3e}"


def test_step_updates_reached_parameters_only():
    from mmfusion.train import RobustTrainStep
    model = _model(256, 4, dropout=0.1, modality_dropout=0.1)
    ti, au, vi, labels = _cuda_inputs(16)
    ts = RobustTrainStep(model, lr=2.5e-2, weight_decay=1e-2)
    assert ts.opt.ranges is not None and ts.opt.max_grad_norm is None
    assert abs(float(ts.opt.hparams[0]) - 1e-3) <= 1e-9 and abs(float(ts.opt.hparams[1]) - 0.95) <= 1e-7
    s0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    reached = {id(p) for p in ts.reached}
    losses = []
    for k in range(3):
        losses.append(float(ts(ti, au, vi, labels, missing_modalities=["audio"] if k == 1 else None)))
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if id(p) in reached:
            assert not torch.equal(p.detach(), s0[n]), f"{n}: reached but did not move"
        else:
            assert torch.equal(p.detach(), s0[n]), f"{n}: not reached but moved"
    # the loss falls on a fixed batch (dropout off)
    model2 = _model(256, 4, seed=6)
    ts2 = RobustTrainStep(model2, lr=2.5e-2)
    ls = [float(ts2(ti, au, vi, labels)) for _ in range(10)]
    assert ls[-1] < ls[0] - 0.05, ls


def test_robust_step_graph_replay_matches_eager():
    """Three RobustTrainStep steps (missing_modalities=["audio"], dropout and ModalityDropout on) captured as one
    single-chain graph and replayed, against three eager steps from the same state: loss, gradient arena, parameters."""
    from mmfusion.train import RobustTrainStep
    model = _model(256, 4, dropout=0.1, modality_dropout=0.1)
    ti, au, vi, labels = _cuda_inputs(16)
    ts = RobustTrainStep(model, lr=1e-5, weight_decay=1e-2)
    check_graph_replay_matches_eager(lambda: ts(ti, au, vi, labels, missing_modalities=["audio"]), ts.arena, ts.opt)


def test_checkpoint_round_trip(tmp_path):
    from models.multimodal_model import RobustMultimodalModel
    from mmfusion.train import RobustTrainStep, load_checkpoint, save_checkpoint
    model = _model(256, 4)
    ti, au, vi, labels = _cuda_inputs(16)
    ts = RobustTrainStep(model, lr=2.5e-2)
    for _ in range(2):
        ts(ti, au, vi, labels)
    path = str(tmp_path / "robust.pt")
    save_checkpoint(path, model, ts.opt, epoch=1, config=model.config)
    torch.manual_seed(99)
    fresh = RobustMultimodalModel(model.config).cuda()
    ts2 = RobustTrainStep(fresh, lr=2.5e-2)
    load_checkpoint(path, fresh, ts2.opt)
    model.eval(), fresh.eval()
    with torch.no_grad():
        for kw in ({}, {"available_modalities": ["text"], "missing_modalities": ["audio", "video"]}):
            a, b = model(ti, au, vi, **kw), fresh(ti, au, vi, **kw)
            for k in ("robust_prediction", "modality_availability", "modality_weights", "emotion_logits"):
                assert torch.equal(a[k], b[k]), (kw, k)
    assert torch.equal(ts.opt.exp_avg, ts2.opt.exp_avg) and ts2.opt.t == ts.opt.sync_step()
