"""Device-side evaluation on the MI355X: ``mmf_eval_accumulate`` (csrc/metrics.hip) against the float64 restatement of
tests/eval_ref.py over many batches (confusion counts, invalid count, predictions exact; loss and confidence sums to 1e-5
relative; probabilities to 1e-6 absolute), torch's argmax on ties and NaN rows, the refusals, bitwise reproducibility and
graph capture; then the evaluation passes of ``mmfusion.evaluate`` on MELD-shaped models against the reference's loops
written in torch + sklearn on the same logits."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_ref
from helpers import hip_lib
from mmfusion import evaluate as ev

pytestmark = pytest.mark.gpu

MMF_E_SHAPE = -1
NAMES7 = ["happy", "sad", "angry", "fear", "surprise", "disgust", "neutral"]


def _batch(B, Cn, seed, heads=1, ties=False, pad=5):
    """`heads` (B, Cn) f32 logit views (head 1 a strided column slice of a wider matrix), int64 targets"""
    g = torch.Generator().manual_seed(seed)
    mats = []
    for h in range(heads):
        x = torch.randn(B, Cn + (pad if h == 1 else 0), generator=g) * 3
        if ties:
            x = torch.round(x)                          # many equal maxima
        mats.append(x.cuda()[:, :Cn])
    y = torch.randint(0, Cn, (B,), generator=g).cuda()
    return mats, y


def _np(batches):
    return [([m.cpu().numpy() for m in mats], y.cpu().numpy()) for mats, y in batches]


def _check_against_ref(acc, batches, Cn, heads, label):
    ref = eval_ref.accumulate(_np(batches), Cn, heads)
    counts, sums = acc.state()
    assert np.array_equal(counts, ref["counts"]), f"{label}: counts"
    assert np.allclose(sums, ref["sums"], rtol=1e-5, atol=0), f"{label}: sums {sums} vs {ref['sums']}"
    preds, targets, probs = acc.collected()
    assert np.array_equal(preds, ref["preds"]) and np.array_equal(targets, ref["targets"]), f"{label}: preds / targets"
    assert np.abs(probs - ref["probs"]).max() <= 1e-6, f"{label}: probs"
    return ref


@pytest.mark.parametrize("Cn", [2, 7, 64])
def test_kernel_against_float64_over_many_batches(Cn):
    acc = ev.EvalAccumulator(Cn, heads=2, capacity=64)             # grows past 64 rows
    batches = []
    for i, B in enumerate((1, 16, 63, 64, 65, 1000, 16)):
        b = _batch(B, Cn, 100 * Cn + i, heads=2, ties=(i % 2 == 1))
        batches.append(b)
        acc.update(b[0][0], b[1], [b[0][1]])
    torch.cuda.synchronize()
    assert batches[0][0][1].stride(0) == Cn + 5
    _check_against_ref(acc, batches, Cn, 2, f"C={Cn}")
    # the kernel's argmax is torch's (ties: the lowest index)
    preds, _, _ = acc.collected()
    want = torch.cat([torch.argmax(m[0], dim=-1) for m, _ in batches]).cpu().numpy()
    assert np.array_equal(preds, want)


def test_nan_row_and_ties_follow_torch_argmax():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, -1.0, 2.0],              # tie: index 1
                      [0.0, 1.0, float("nan"), 5.0, float("nan"), 0.0, 0.0],   # first NaN: index 2
                      [float("-inf")] * 7,                                 # all -inf: index 0
                      [2.0] * 7], device="cuda")                           # all equal: index 0
    y = torch.tensor([1, 2, 0, 3], device="cuda")
    acc = ev.EvalAccumulator(7, capacity=4)
    acc.update(x, y)
    torch.cuda.synchronize()
    preds, _, probs = acc.collected()
    assert preds.tolist() == torch.argmax(x, dim=-1).tolist() == [1, 2, 0, 0]
    with np.errstate(invalid="ignore"):                                   # the NaN and all -inf rows
        ref = eval_ref.accumulate([([x.cpu().numpy()], y.cpu().numpy())], 7)
    counts, sums = acc.state()
    assert np.array_equal(counts, ref["counts"])
    assert np.isnan(probs[1]).all() and np.isnan(sums).all()             # NaN propagates as in torch's softmax


def test_refusals_launch_nothing():
    L, st = hip_lib()
    x = torch.randn(8, 65, device="cuda")
    y = torch.zeros(8, dtype=torch.int64, device="cuda")
    counts = torch.zeros(4 * 65 * 65 + 2, dtype=torch.int64, device="cuda")
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")

    def call(Cn, B, heads, ld=65, row0=0, cap=0, pred=None):
        ptrs = (C.c_void_p * 4)(*[x.data_ptr()] * 4)
        lds = (C.c_int * 4)(*[ld] * 4)
        return L.mmf_eval_accumulate(ptrs, lds, heads, y.data_ptr(), B, Cn, 0.1, counts.data_ptr(), sums.data_ptr(),
                                     pred, None, None, row0, cap, st)

    assert call(65, 8, 1) == MMF_E_SHAPE
    assert call(0, 8, 1) == MMF_E_SHAPE
    assert call(7, 0, 1) == MMF_E_SHAPE
    assert call(7, 8, 0) == MMF_E_SHAPE
    assert call(7, 8, 5) == MMF_E_SHAPE
    assert call(7, 8, 1, ld=6) == MMF_E_SHAPE
    pred = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert call(7, 8, 1, row0=1, cap=8, pred=pred.data_ptr()) == MMF_E_SHAPE       # rows 1..8 beyond capacity 8
    torch.cuda.synchronize()
    assert int(counts.abs().sum()) == 0 and float(sums.abs().sum()) == 0.0
    with pytest.raises(ValueError):
        ev.EvalAccumulator(65)


def test_invalid_targets_raise_from_compute():
    acc = ev.EvalAccumulator(7)
    x, y = _batch(16, 7, 3)
    y[3], y[9] = 7, -1
    acc.update(x[0], y)
    with pytest.raises(ValueError, match="2 target"):
        acc.compute()


def test_bitwise_reproducible():
    batches = [_batch(B, 7, 50 + i, heads=4) for i, B in enumerate((16, 1000, 33))]
    runs = []
    for _ in range(2):
        acc = ev.EvalAccumulator(7, heads=4, capacity=2048)
        for mats, y in batches:
            acc.update(mats[0], y, mats[1:])
        torch.cuda.synchronize()
        runs.append((acc.counts.clone(), acc.sums.clone(), acc.probs[:acc.rows].clone()))
    (c0, s0, p0), (c1, s1, p1) = runs
    assert torch.equal(c0, c1) and torch.equal(s0.view(torch.int64), s1.view(torch.int64))
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))


def test_update_captures_into_a_graph_and_replays_identically():
    import bench
    (x,), y = _batch(16, 7, 77)
    eager = ev.EvalAccumulator(7)
    for _ in range(3):
        eager.update(x, y)
    acc = ev.EvalAccumulator(7)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with bench.single_stream():
        with torch.cuda.stream(side):
            acc.update(x, y)                            # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        acc.reset()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                       # a host sync inside update() would fail the capture
            acc.update(x, y)
    torch.cuda.synchronize()
    assert int(acc.counts.sum()) == 0                   # captured, not run
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.counts, eager.counts)
    assert torch.equal(acc.sums.view(torch.int64), eager.sums.view(torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the evaluation passes on MELD-shaped models
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(fusion="hierarchical", d=256, heads=4):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = True
    cfg.fusion_type = fusion
    cfg.fusion_hidden_size, cfg.fusion_num_heads, cfg.graph_hidden_size = d, heads, d
    return cfg


def _batches(sizes, seed=1234, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    out = []
    for B in sizes:
        out.append({"text": {"input_ids": torch.randn(B, 9, 768, generator=g).to(device),
                             "attention_mask": torch.ones(B, 9, dtype=torch.long).to(device)},
                    "audio": torch.randn(B, 21, 768, generator=g).to(device),
                    "video": torch.randn(B, 6, 768, generator=g).to(device),
                    "emotion": torch.randint(0, 7, (B,), generator=g).to(device)})
    return out


def _record(model, key="emotion_logits"):
    rec = []
    h = model.register_forward_hook(lambda m, args, out: rec.append({k: (v.detach().clone() if torch.is_tensor(v) else
                                                                      {kk: vv.detach().clone() for kk, vv in v.items()})
                                                                     for k, v in out.items()
                                                                     if torch.is_tensor(v) or k == "individual_logits"}))
    return rec, h


def _sk():
    return pytest.importorskip("sklearn.metrics")


def test_validate_matches_the_reference_loop():
    skm = _sk()
    from models.multimodal_model import MultimodalEmotionModel
    torch.manual_seed(3)
    model = MultimodalEmotionModel(_cfg()).cuda()
    batches = _batches((16, 16, 16, 16, 16, 7), device="cpu")
    rec, h = _record(model)
    metrics, report, preds, targets, probs = ev.validate(model, batches, NAMES7)
    h.remove()
    assert not model.training and len(rec) == len(batches)
    # the reference loop (advanced_trainer.py:209-263) on the same logits
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    total, P, T, PR = 0.0, [], [], []
    for out, b in zip(rec, batches):
        lg, y = out["emotion_logits"], b["emotion"].cuda()
        total += crit(lg, y).item()
        P.extend(torch.argmax(lg, dim=-1).cpu().numpy()), T.extend(y.cpu().numpy())
        PR.extend(F.softmax(lg, dim=-1).cpu().numpy())
    val_loss = total / len(batches)
    assert metrics["val_loss"] == pytest.approx(val_loss, rel=1e-5)
    assert np.array_equal(preds, np.array(P)) and np.array_equal(targets, np.array(T))
    assert np.abs(probs - np.array(PR)).max() <= 1e-6
    assert metrics["val_accuracy"] == skm.accuracy_score(T, P)
    assert metrics["val_f1_macro"] == pytest.approx(skm.f1_score(T, P, average="macro"), rel=1e-12)
    assert metrics["val_f1_weighted"] == pytest.approx(skm.f1_score(T, P, average="weighted"), rel=1e-12)
    try:
        want = skm.classification_report(T, P, target_names=NAMES7, output_dict=True)
    except ValueError:
        want = None                                     # fewer present labels than names: the documented deviation
    if want is not None:
        eval_ref.assert_close_tree(report, want, rtol=1e-12, atol=1e-12)
    assert set(metrics) == {"val_loss", "val_accuracy", "val_f1_macro", "val_f1_weighted"}


def test_evaluate_dataset_late_fusion_individual_metrics():
    skm = _sk()
    from models.multimodal_model import MultimodalEmotionModel
    torch.manual_seed(4)
    model = MultimodalEmotionModel(_cfg("late")).cuda()
    batches = _batches((16, 16, 16, 16, 5), seed=99)
    rec, h = _record(model)
    res = ev.evaluate_dataset(model, batches, NAMES7)
    h.remove()
    assert set(res) == {"metrics", "individual_metrics", "predictions", "targets", "probabilities", "features"}
    T = torch.cat([b["emotion"] for b in batches]).cpu().numpy()
    lg = torch.cat([o["emotion_logits"] for o in rec])
    P = torch.argmax(lg, dim=-1).cpu().numpy()
    assert np.array_equal(res["predictions"], P) and np.array_equal(res["targets"], T)
    m = res["metrics"]
    assert m["accuracy"] == skm.accuracy_score(T, P)
    assert m["f1_macro"] == pytest.approx(skm.f1_score(T, P, average="macro"), rel=1e-12)
    assert set(res["individual_metrics"]) == {"text", "audio", "video"}
    for mod, got in res["individual_metrics"].items():
        pm = torch.cat([torch.argmax(o["individual_logits"][mod], dim=-1) for o in rec]).cpu().numpy()
        assert got["accuracy"] == skm.accuracy_score(T, pm), mod
        assert got["f1_macro"] == pytest.approx(skm.f1_score(T, pm, average="macro"), rel=1e-12), mod
        assert got["f1_weighted"] == pytest.approx(skm.f1_score(T, pm, average="weighted"), rel=1e-12), mod
    feats = torch.cat([(o["text_features"] + o["audio_features"] + o["video_features"]) / 3 for o in rec]).float()
    assert res["features"].shape == tuple(feats.shape) and np.array_equal(res["features"], feats.cpu().numpy())


def test_evaluate_dataset_standard_model_has_no_individual_metrics():
    from models.multimodal_model import MultimodalEmotionModel
    torch.manual_seed(5)
    model = MultimodalEmotionModel(_cfg()).cuda()
    res = ev.evaluate_dataset(model, _batches((16, 3), seed=5), NAMES7)
    assert res["individual_metrics"] == {} and res["probabilities"].shape == (19, 7)
    assert set(res["metrics"]) == set(ev._METRIC_KEYS)


def test_evaluate_robustness_seven_scenarios():
    skm = _sk()
    from models.multimodal_model import RobustMultimodalModel
    torch.manual_seed(6)
    model = RobustMultimodalModel(_cfg()).cuda()
    batches = _batches((16, 16, 16, 11), seed=7)
    rec, h = _record(model)
    res = ev.evaluate_robustness(model, batches)
    h.remove()
    assert list(res) == [ev.scenario_name(m) for m in ev.SCENARIOS]
    assert len(rec) == 7 * len(batches)
    T = torch.cat([b["emotion"] for b in batches]).cpu().numpy()
    for i, name in enumerate(res):
        outs = rec[i * len(batches):(i + 1) * len(batches)]
        P = torch.cat([torch.argmax(o["robust_prediction"], dim=-1) for o in outs]).cpu().numpy()
        assert res[name]["accuracy"] == skm.accuracy_score(T, P), name
        assert res[name]["f1_macro"] == pytest.approx(skm.f1_score(T, P, average="macro"), rel=1e-12), name
