"""Device-side evaluation without a GPU: the float64 oracle of tests/eval_ref.py and ``mmfusion.evaluate.finalize``
against sklearn (the reference's metric library) and against each other, the scenario names and key sets against the
reference's literals, a two-rank gloo ``all_reduce``, and the ABI entry point."""
import os
import tempfile

import numpy as np
import pytest
import torch

import eval_ref
from mmfusion import evaluate as ev, lib

NAMES7 = ["happy", "sad", "angry", "fear", "surprise", "disgust", "neutral"]


def _sklearn_metrics(t, p, P, names):
    """the reference's _calculate_metrics (evaluate_model.py:145-203), verbatim calls"""
    skm = pytest.importorskip("sklearn.metrics")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = {"accuracy": skm.accuracy_score(t, p), "f1_macro": skm.f1_score(t, p, average="macro"),
               "f1_weighted": skm.f1_score(t, p, average="weighted"), "f1_micro": skm.f1_score(t, p, average="micro"),
               "precision_macro": skm.precision_score(t, p, average="macro"),
               "precision_weighted": skm.precision_score(t, p, average="weighted"),
               "recall_macro": skm.recall_score(t, p, average="macro"),
               "recall_weighted": skm.recall_score(t, p, average="weighted"),
               "per_class_f1": skm.f1_score(t, p, average=None).tolist(),
               "per_class_precision": skm.precision_score(t, p, average=None).tolist(),
               "per_class_recall": skm.recall_score(t, p, average=None).tolist()}
        try:
            out["classification_report"] = skm.classification_report(t, p, target_names=names, output_dict=True)
        except ValueError:
            out["classification_report"] = None          # the documented deviation: compared separately
        try:
            out["roc_auc"] = skm.roc_auc_score(t, P, multi_class="ovr", average="macro")
        except Exception:
            out["roc_auc"] = None
        mp = np.max(P, axis=1)
        ok = p == t
        out["confidence_stats"] = {"mean_confidence": np.mean(mp), "mean_confidence_correct": np.mean(mp[ok]),
                                   "mean_confidence_incorrect": np.mean(mp[~ok]) if np.any(~ok) else 0,
                                   "confidence_std": np.std(mp)}
    return out


def _case(name, C=7, n=200, seed=0):
    """(targets, logits) of a named label situation"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, C)).astype(np.float32)
    t = rng.integers(0, C, n)
    if name == "random":
        pass
    elif name == "absent_class":                      # class 3 neither a target nor a prediction
        t[t == 3] = 4
        x[:, 3] = -10
    elif name == "never_predicted":                   # class 2 a target, never predicted
        x[:, 2] = -10
    elif name == "all_correct":
        x[np.arange(n), t] += 20
    elif name == "single_class":
        t[:] = 5
        x[:, 5] += 20
    elif name == "prob_ties":                         # coarse logits: many equal probabilities (AUC ties)
        x = np.round(x).astype(np.float32)
        x[:, 0] = x[:, 1]
    elif name == "only_two_targets":
        t = t % 2
    return t, x


CASES = ("random", "absent_class", "never_predicted", "all_correct", "single_class", "prob_ties", "only_two_targets")


def _through_finalize(t, x, C, names, batch=37):
    bs = [([x[i:i + batch]], t[i:i + batch]) for i in range(0, len(t), batch)]
    acc = eval_ref.accumulate(bs, C)
    return acc, ev.finalize(acc["counts"], acc["sums"], C, 1, names, acc["probs"].astype(np.float32), acc["targets"])


@pytest.mark.parametrize("case", CASES)
def test_eval_ref_and_finalize_match_sklearn(case):
    t, x = _case(case)
    acc, fin = _through_finalize(t, x, 7, NAMES7)
    p, P = acc["preds"], acc["probs"].astype(np.float32)
    assert np.array_equal(p, np.argmax(x, axis=1))
    sk = _sklearn_metrics(t, p, P, NAMES7)
    ref = eval_ref.metrics(t, p, P, NAMES7)
    skip = ("classification_report",) if sk["classification_report"] is None else ()
    # the oracle against sklearn: exact rules, f64 arithmetic (confidence: numpy reduces in f32 there)
    eval_ref.assert_close_tree(ref, sk, rtol=1e-10, atol=1e-10, skip=skip + ("confidence_stats",))
    eval_ref.assert_close_tree(ref["confidence_stats"], sk["confidence_stats"], rtol=1e-5, atol=1e-6)
    # finalize against sklearn and against the oracle
    eval_ref.assert_close_tree({k: fin[k] for k in sk}, sk, rtol=1e-10, atol=1e-10, skip=skip + ("confidence_stats",))
    eval_ref.assert_close_tree({k: fin[k] for k in ref}, ref, rtol=1e-9, atol=1e-12, skip=("confidence_stats",))
    ref64 = eval_ref.metrics(t, p, acc["probs"], NAMES7)          # the confidence sums are f64 in both
    # (the std comes from sum p and sum p^2: its absolute error is ~ sqrt(2^-52), visible where the spread is ~0)
    eval_ref.assert_close_tree(fin["confidence_stats"], ref64["confidence_stats"], rtol=1e-9, atol=1e-7)
    if skip:                                          # sklearn raised: the report is over the present labels' own names
        labels = np.union1d(t, p)
        assert [k for k in fin["classification_report"] if k not in ("accuracy", "macro avg", "weighted avg")] == \
            [NAMES7[c] for c in labels]
    assert fin["val_loss"] == pytest.approx(acc["sums"][0] / acc["counts"][-1])
    assert fin["num_samples"] == len(t)


def test_classification_report_layout_matches_sklearn_exactly():
    skm = pytest.importorskip("sklearn.metrics")
    t, x = _case("random", seed=3)
    acc, fin = _through_finalize(t, x, 7, NAMES7)
    want = skm.classification_report(t, acc["preds"], target_names=NAMES7, output_dict=True)
    got = fin["classification_report"]
    assert list(got) == list(want)
    for k in want:
        if isinstance(want[k], dict):
            assert list(got[k]) == list(want[k])
            assert all(type(got[k][kk]) is float for kk in got[k])


def test_roc_auc_ties_and_none():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(4)
    t = np.arange(60) % 4
    P = rng.integers(0, 3, (60, 4)).astype(np.float64) + 1.0
    P /= P.sum(1, keepdims=True)                      # heavy ties within every column
    want = skm.roc_auc_score(t, P, multi_class="ovr", average="macro")
    assert ev.roc_auc_ovr_macro(t, P) == pytest.approx(want, rel=1e-12)
    assert eval_ref.roc_auc(t, P) == pytest.approx(want, rel=1e-12)
    assert ev.roc_auc_ovr_macro(t % 3, P) is None     # a class of the columns absent from the targets
    P2 = P.copy()
    P2[0, 0] = np.nan
    assert ev.roc_auc_ovr_macro(t, P2) is None


def test_finalize_invalid_targets_raise():
    x = np.random.default_rng(0).standard_normal((8, 7)).astype(np.float32)
    acc = eval_ref.accumulate([([x], np.array([0, 1, 7, 2, -1, 3, 4, 5]))], 7)
    assert acc["counts"][-2] == 2
    with pytest.raises(ValueError, match="2 target"):
        ev.finalize(acc["counts"], acc["sums"], 7)


def test_finalize_individual_heads():
    rng = np.random.default_rng(5)
    bs = []
    for B in (16, 16, 5):
        bs.append(([rng.standard_normal((B, 7)).astype(np.float32) for _ in range(4)], rng.integers(0, 7, B)))
    acc = eval_ref.accumulate(bs, 7, heads=4)
    fin = ev.finalize(acc["counts"], acc["sums"], 7, 4)
    t = np.concatenate([y for _, y in bs])
    for h in range(1, 4):
        p = np.concatenate([np.argmax(l[h], 1) for l, _ in bs])
        ref = eval_ref.metrics(t, p)
        got = fin["individual_metrics"][h - 1]
        assert got == pytest.approx({k: ref[k] for k in ("accuracy", "f1_macro", "f1_weighted")}, rel=1e-12)


# the reference's literals: advanced_trainer.py:611-624 (scenarios), :250-255 (validate), evaluate_model.py:136-143, 187-202
REF_SCENARIO_NAMES = ["all", "text_missing", "audio_missing", "video_missing", "text_audio_missing", "text_video_missing",
                      "audio_video_missing"]
REF_VALIDATE_KEYS = {"val_loss", "val_accuracy", "val_f1_macro", "val_f1_weighted"}
REF_DATASET_KEYS = {"metrics", "individual_metrics", "predictions", "targets", "probabilities", "features"}
REF_METRIC_KEYS = {"accuracy", "f1_macro", "f1_weighted", "f1_micro", "precision_macro", "precision_weighted", "recall_macro",
                   "recall_weighted", "roc_auc", "per_class_f1", "per_class_precision", "per_class_recall",
                   "classification_report", "confidence_stats"}
REF_CONFIDENCE_KEYS = {"mean_confidence", "mean_confidence_correct", "mean_confidence_incorrect", "confidence_std"}


def test_scenario_names_and_key_sets_match_the_reference():
    assert [ev.scenario_name(m) for m in ev.SCENARIOS] == REF_SCENARIO_NAMES
    assert set(ev._METRIC_KEYS) == REF_METRIC_KEYS
    t, x = _case("random")
    _, fin = _through_finalize(t, x, 7, NAMES7)
    assert REF_METRIC_KEYS <= set(fin) and set(fin["confidence_stats"]) == REF_CONFIDENCE_KEYS
    import inspect
    src = inspect.getsource(ev.validate) + inspect.getsource(ev.evaluate_dataset)
    for k in REF_VALIDATE_KEYS | REF_DATASET_KEYS:
        assert f'"{k}"' in src, k


# ---- two ranks, gloo: all_reduce + finalize of two shards == one pass over the union ---------------------------------
def _shards():
    rng = np.random.default_rng(11)
    bs = [([rng.standard_normal((B, 7)).astype(np.float32) for _ in range(2)], rng.integers(0, 7, B))
          for B in (16, 16, 16, 9, 16, 3)]
    return bs[:4], bs[4:]


def _rank_main(rank, world, init_file, out_file):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        mine = _shards()[rank]
        acc = ev.EvalAccumulator(7, heads=2, device="cpu")
        ref = eval_ref.accumulate(mine, 7, heads=2)
        acc.counts.copy_(torch.from_numpy(ref["counts"]))
        acc.sums.copy_(torch.from_numpy(ref["sums"]))
        acc.all_reduce()
        fin = acc.compute(NAMES7)
        if rank == 0:
            np.save(out_file, np.array([fin], dtype=object), allow_pickle=True)
    finally:
        dist.destroy_process_group()


def test_all_reduce_two_ranks_equals_union():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        init, out = os.path.join(d, "init"), os.path.join(d, "out.npy")
        mp.start_processes(_rank_main, args=(2, init, out), nprocs=2, join=True, start_method="spawn")
        got = np.load(out, allow_pickle=True)[0]
    a, b = _shards()
    union = eval_ref.accumulate(a + b, 7, heads=2)
    want = ev.finalize(union["counts"], union["sums"], 7, 2, NAMES7)
    eval_ref.assert_close_tree({k: v for k, v in got.items()}, {k: v for k, v in want.items()}, rtol=1e-12, atol=1e-12)
    assert got["num_samples"] == 76 and np.array_equal(got["confusion_matrix"], want["confusion_matrix"])


def test_eval_accumulate_is_exported():
    assert "mmf_eval_accumulate" in lib.SYMBOLS
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = lib.load()
    assert L.mmf_eval_accumulate.argtypes is not None and len(L.mmf_eval_accumulate.argtypes) == 15


def test_accumulator_update_refuses_the_cpu():
    acc = ev.EvalAccumulator(7, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        acc.update(torch.zeros(4, 7), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        ev.EvalAccumulator(65, device="cpu")
    with pytest.raises(ValueError):
        ev.EvalAccumulator(7, heads=5, device="cpu")
