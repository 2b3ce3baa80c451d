"""Float64 numpy restatement of device-side evaluation (csrc/metrics.hip, mmfusion/evaluate.py), the oracle of
tests/test_eval_gpu.py and tests/test_eval_cpu.py.  No sklearn: ``metrics`` recomputes the reference's
``_calculate_metrics`` (evaluate_model.py:145-203) from the label arrays themselves, by sklearn's rules (labels = those
present in targets or predictions, zero_division 0.0), independently of the confusion-matrix route ``finalize`` takes."""
import numpy as np


def softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    return e / e.sum(axis=1, keepdims=True)


def ce_ls64(x, y, eps):
    """torch's CrossEntropyLoss(label_smoothing=eps) per row, float64"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    logp_y = x[np.arange(len(y)), y] - lse
    return (1 - eps) * (-logp_y) + eps * (lse - x.mean(axis=1))


def accumulate(batches, C, heads=1, eps=0.1):
    """mmf_eval_accumulate over a list of batches [(logits: list of `heads` (B, C) arrays, targets (B,))].
    -> dict(counts int64 (heads C C + 2), sums float64 (4), preds, targets, probs) — the kernel's accumulators and its
    collected outputs.  Predictions: numpy's argmax (first maximum; the first NaN if a row holds one), torch's rule."""
    counts = np.zeros(heads * C * C + 2, dtype=np.int64)
    conf = counts[:heads * C * C].reshape(heads, C, C)
    sums = np.zeros(4, dtype=np.float64)
    preds, tgts, probs = [], [], []
    for logits, y in batches:
        y = np.asarray(y, dtype=np.int64)
        valid = (y >= 0) & (y < C)
        for h in range(heads):
            p = np.argmax(np.asarray(logits[h]), axis=1)
            np.add.at(conf[h], (y[valid], p[valid]), 1)
        x = np.asarray(logits[0], dtype=np.float64)
        p = np.argmax(np.asarray(logits[0]), axis=1)
        P = softmax64(x)
        pmax = 1.0 / np.exp(x - x.max(axis=1, keepdims=True)).sum(axis=1)
        loss = np.zeros(len(y))
        loss[valid] = ce_ls64(x[valid], y[valid], eps)
        sums[0] += loss.sum() / len(y)
        sums[1] += pmax.sum()
        sums[2] += (pmax * pmax).sum()
        sums[3] += pmax[valid & (p == y)].sum()
        counts[-2] += int((~valid).sum())
        counts[-1] += 1
        preds.append(p), tgts.append(y), probs.append(P)
    return {"counts": counts, "sums": sums, "preds": np.concatenate(preds), "targets": np.concatenate(tgts),
            "probs": np.concatenate(probs)}


def _prf(t, p):
    labels = np.union1d(t, p)
    prec, rec, f1, sup = [], [], [], []
    for c in labels:
        tp = np.sum((t == c) & (p == c))
        fp = np.sum((t != c) & (p == c))
        fn = np.sum((t == c) & (p != c))
        prec.append(tp / (tp + fp) if tp + fp else 0.0)
        rec.append(tp / (tp + fn) if tp + fn else 0.0)
        f1.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
        sup.append(float(tp + fn))
    return labels, np.array(prec), np.array(rec), np.array(f1), np.array(sup)


def roc_auc(t, P):
    """one-vs-rest macro AUC as the probability that a positive outscores a negative (ties count half), or None where
    sklearn's roc_auc_score raises"""
    t, P = np.asarray(t), np.asarray(P, dtype=np.float64)
    C = P.shape[1]
    if C < 3 or sorted(set(t.tolist())) != list(range(C)) or not np.isfinite(P).all() or not np.allclose(1, P.sum(1)):
        return None
    aucs = []
    for c in range(C):
        pos, neg = P[t == c, c], P[t != c, c]
        gt = (pos[:, None] > neg[None, :]).sum()
        eq = (pos[:, None] == neg[None, :]).sum()
        aucs.append((gt + 0.5 * eq) / (len(pos) * len(neg)))
    return float(np.mean(aucs))


def metrics(t, p, P=None, names=None):
    """the reference's _calculate_metrics from targets, predictions and (optionally) probabilities, float64"""
    t, p = np.asarray(t), np.asarray(p)
    labels, prec, rec, f1, sup = _prf(t, p)
    n = len(t)
    acc = float(np.mean(t == p))
    w = sup / sup.sum()
    out = {"accuracy": acc, "f1_macro": f1.mean(), "f1_weighted": (f1 * w).sum(), "f1_micro": acc,
           "precision_macro": prec.mean(), "precision_weighted": (prec * w).sum(),
           "recall_macro": rec.mean(), "recall_weighted": (rec * w).sum(),
           "per_class_f1": f1.tolist(), "per_class_precision": prec.tolist(), "per_class_recall": rec.tolist(),
           "roc_auc": roc_auc(t, P) if P is not None else None}
    keys = list(names) if names is not None and len(names) == len(labels) else \
        [names[c] for c in labels] if names is not None else [str(c) for c in labels]
    rep = {k: {"precision": prec[i], "recall": rec[i], "f1-score": f1[i], "support": sup[i]} for i, k in enumerate(keys)}
    rep["accuracy"] = acc
    rep["macro avg"] = {"precision": prec.mean(), "recall": rec.mean(), "f1-score": f1.mean(), "support": float(n)}
    rep["weighted avg"] = {"precision": (prec * w).sum(), "recall": (rec * w).sum(), "f1-score": (f1 * w).sum(),
                           "support": float(n)}
    out["classification_report"] = rep
    if P is not None:
        mp = np.asarray(P, dtype=np.float64).max(axis=1)
        ok = p == t
        out["confidence_stats"] = {"mean_confidence": mp.mean(),
                                   "mean_confidence_correct": mp[ok].mean() if ok.any() else float("nan"),
                                   "mean_confidence_incorrect": mp[~ok].mean() if (~ok).any() else 0,
                                   "confidence_std": mp.std()}
    return out


def assert_close_tree(got, want, rtol=1e-12, atol=1e-12, path="", skip=()):
    """nested dicts / lists / numbers equal up to rtol / atol (None == None, nan == nan, the same keys)"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) - set(skip) == set(want) - set(skip), \
            f"{path}: keys {sorted(got) if isinstance(got, dict) else got} != {sorted(want)}"
        for k in want:
            if k not in skip:
                assert_close_tree(got[k], want[k], rtol, atol, f"{path}/{k}", skip)
    elif isinstance(want, list) and want and isinstance(want[0], dict):
        assert isinstance(got, list) and len(got) == len(want), f"{path}: {got} != {want}"
        for i, (g, w) in enumerate(zip(got, want)):
            assert_close_tree(g, w, rtol, atol, f"{path}[{i}]", skip)
    elif want is None or got is None:
        assert got is None and want is None, f"{path}: {got} != {want}"
    else:
        g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert g.shape == w.shape, f"{path}: shape {g.shape} != {w.shape}"
        assert np.allclose(g, w, rtol=rtol, atol=atol, equal_nan=True), f"{path}: {got} != {want}"
