"""Device-side evaluation: the metrics tail of the reference's evaluation loops as one HIP launch per batch.

Reference (paths relative to its root): ``training/advanced_trainer.py:209-263`` (``validate``), ``:607-660``
(``evaluate_robustness``) and ``evaluate_model.py:55-203`` (``evaluate_dataset``, ``_calculate_metrics``) run softmax,
argmax and ``CrossEntropyLoss(label_smoothing=0.1)`` per batch in torch, sync the host on ``.item()`` and three ``.cpu()``
copies, and hand the collected lists to sklearn.  Here:

  * ``EvalAccumulator.update`` adds a batch to device-resident accumulators with ONE launch of ``mmf_eval_accumulate``
    (``csrc/metrics.hip``): per head the C x C confusion counts, for the main head the sum of batch-mean losses and the
    confidence sums, optionally the predictions, targets and probabilities.  It never syncs the host, so it can be
    captured into a graph.
  * ``EvalAccumulator.compute`` copies the accumulators once and ``finalize`` turns them into the reference's metrics in
    float64 numpy (no sklearn).
  * ``validate``, ``evaluate_dataset`` and ``evaluate_robustness`` are the reference's three loops on top of it, returning
    what the reference methods return, with the same keys.

``finalize`` follows sklearn's rules: the labels are those present in targets or predictions (absent classes are left
out of the macro averages and the per-class lists), ``zero_division`` gives 0.0, ``roc_auc`` is None where
``roc_auc_score`` would raise (the reference catches that).  The one deviation: where ``classification_report`` would
raise because the number of present labels differs from the number of target names, the report is built over the present
labels under their own names (``names[label]``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib

MODALITIES = ("text", "audio", "video")
# the reference's missing-modality scenarios (advanced_trainer.py:611-619) and their names (:624)
SCENARIOS = ([], ["text"], ["audio"], ["video"], ["text", "audio"], ["text", "video"], ["audio", "video"])


def scenario_name(missing: Sequence[str]) -> str:
    return "all" if not missing else "_".join(missing) + "_missing"


# ---------------------------------------------------------------------------------------------------------------------
# the accumulator
# ---------------------------------------------------------------------------------------------------------------------
class EvalAccumulator:
    """Device accumulators of ``mmf_eval_accumulate`` for ``heads`` logit matrices of ``num_classes`` columns.

    ``counts`` (int64): ``heads`` C x C confusion matrices (row = target, column = prediction), then the number of
    invalid targets, then the number of batches.  ``sums`` (float64): the sum of batch-mean cross-entropies (label
    smoothing ``label_smoothing``), of the max-probabilities, of their squares, and of the max-probabilities of the
    rows predicted correctly, all of head 0.  With ``capacity`` (rows), head 0's predictions, the targets and head 0's
    softmax probabilities are also kept on the device; the buffers double when a batch would overflow them (a torch
    copy, no host sync)."""

    def __init__(self, num_classes: int, heads: int = 1, label_smoothing: float = 0.1, capacity: Optional[int] = None,
                 device="cuda"):
        if not 1 <= num_classes <= 64:
            raise ValueError(f"num_classes must be in 1..64, got {num_classes}")
        if not 1 <= heads <= lib.EVAL_MAX_HEADS:
            raise ValueError(f"heads must be in 1..{lib.EVAL_MAX_HEADS}, got {heads}")
        self.num_classes, self.heads, self.label_smoothing = num_classes, heads, float(label_smoothing)
        self.device = torch.device(device)
        C_ = num_classes
        self.counts = torch.zeros(heads * C_ * C_ + 2, dtype=torch.int64, device=self.device)
        self.sums = torch.zeros(lib.EVAL_NSUMS, dtype=torch.float64, device=self.device)
        self.collect = capacity is not None
        self.rows = 0
        self.reduced = False
        if self.collect:
            cap = max(int(capacity), 1)
            self.preds = torch.empty(cap, dtype=torch.int64, device=self.device)
            self.targets = torch.empty(cap, dtype=torch.int64, device=self.device)
            self.probs = torch.empty(cap, C_, dtype=torch.float32, device=self.device)

    def reset(self) -> None:
        self.counts.zero_()
        self.sums.zero_()
        self.rows = 0
        self.reduced = False

    def _grow(self, need: int) -> None:
        cap = self.preds.shape[0]
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        preds = torch.empty(cap, dtype=torch.int64, device=self.device)
        targets = torch.empty(cap, dtype=torch.int64, device=self.device)
        probs = torch.empty(cap, self.num_classes, dtype=torch.float32, device=self.device)
        n = self.rows
        preds[:n].copy_(self.preds[:n])
        targets[:n].copy_(self.targets[:n])
        probs[:n].copy_(self.probs[:n])
        self.preds, self.targets, self.probs = preds, targets, probs

    def update(self, logits: torch.Tensor, targets: torch.Tensor, individual_logits=None) -> None:
        """Add one batch: ``logits`` (B, C) f32 (rows may be strided), ``targets`` (B,) int64, ``individual_logits`` the
        other heads' (B, C) logits (a sequence, or a dict in ``MODALITIES`` order).  One launch, no host sync."""
        if self.device.type != "cuda" or not logits.is_cuda:
            raise RuntimeError("mmfusion: EvalAccumulator.update runs on the GPU only (no CPU fallback)")
        if isinstance(individual_logits, dict):
            individual_logits = [individual_logits[m] for m in MODALITIES if m in individual_logits]
        heads = [logits] + list(individual_logits or [])
        if len(heads) != self.heads:
            raise ValueError(f"update got {len(heads)} logit matrices, the accumulator has {self.heads} heads")
        B = logits.shape[0]
        ptrs, lds = (C.c_void_p * lib.EVAL_MAX_HEADS)(), (C.c_int * lib.EVAL_MAX_HEADS)()
        keep = []
        for h, x in enumerate(heads):
            if x.dim() != 2 or x.shape != (B, self.num_classes):
                raise ValueError(f"head {h}: logits of shape {tuple(x.shape)}, expected ({B}, {self.num_classes})")
            if x.dtype != torch.float32:
                x = x.float()
            if x.stride(1) != 1:
                x = x.contiguous()
            keep.append(x)
            ptrs[h], lds[h] = x.data_ptr(), x.stride(0) if B > 1 else self.num_classes
        if targets.dtype != torch.int64 or not targets.is_contiguous() or targets.shape != (B,):
            targets = targets.reshape(B).to(torch.int64).contiguous()
        outs = (None, None, None)
        row0, cap = 0, 0
        if self.collect:
            self._grow(self.rows + B)
            outs = (self.preds.data_ptr(), self.targets.data_ptr(), self.probs.data_ptr())
            row0, cap = self.rows, self.preds.shape[0]
        lib.check(lib.load().mmf_eval_accumulate(ptrs, lds, len(heads), targets.data_ptr(), B, self.num_classes,
                                                 self.label_smoothing, self.counts.data_ptr(), self.sums.data_ptr(),
                                                 *outs, row0, cap, lib.stream_ptr()))
        if self.collect:
            self.rows += B

    def all_reduce(self, group=None) -> None:
        """With ``torch.distributed`` initialised: one SUM of the counts and one of the sums over the ranks, so that every
        rank's ``compute()`` gives the metrics of the union of the ranks' shards.  The collected predictions and
        probabilities stay per rank: after a reduction over more than one rank ``compute()`` reports ``roc_auc`` None."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=group)
        self.reduced = dist.get_world_size(group) > 1

    def state(self) -> Tuple[np.ndarray, np.ndarray]:
        """(counts, sums) as host numpy arrays: the one copy of a pass"""
        return self.counts.cpu().numpy(), self.sums.cpu().numpy()

    def collected(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(predictions, targets, probabilities) of the rows added so far, host numpy"""
        if not self.collect:
            raise RuntimeError("EvalAccumulator was built without capacity: nothing collected")
        n = self.rows
        return self.preds[:n].cpu().numpy(), self.targets[:n].cpu().numpy(), self.probs[:n].cpu().numpy()

    def compute(self, names: Optional[Sequence[str]] = None, probabilities: Optional[np.ndarray] = None,
                targets: Optional[np.ndarray] = None) -> Dict:
        """finalize() of the accumulated state; raises ValueError if any target was outside 0..C-1.  ``roc_auc`` uses
        ``probabilities`` / ``targets`` if given, else the collected ones (if any, and not after a multi-rank reduce)."""
        counts, sums = self.state()
        if probabilities is None and self.collect and not self.reduced:
            _, targets, probabilities = self.collected()
        return finalize(counts, sums, self.num_classes, self.heads, names, probabilities, targets)


# ---------------------------------------------------------------------------------------------------------------------
# finalize: accumulators -> the reference's metrics (float64 numpy)
# ---------------------------------------------------------------------------------------------------------------------
def split_counts(counts: np.ndarray, num_classes: int, heads: int):
    """-> (confusion (heads, C, C), invalid, batches)"""
    counts = np.asarray(counts, dtype=np.int64)
    CC = num_classes * num_classes
    if counts.shape != (heads * CC + 2,):
        raise ValueError(f"counts of shape {counts.shape}, expected ({heads * CC + 2},)")
    return counts[:heads * CC].reshape(heads, num_classes, num_classes), int(counts[-2]), int(counts[-1])


def prf_from_confusion(conf: np.ndarray):
    """sklearn's precision / recall / F1 per label and their averages from a confusion matrix (row = target, column =
    prediction) over the labels present in targets or predictions; zero_division = 0.0.
    -> (labels, precision, recall, f1, support, averages {macro, weighted, micro: (p, r, f)})"""
    conf = np.asarray(conf, dtype=np.float64)
    support, predicted, tp = conf.sum(1), conf.sum(0), np.diag(conf).copy()
    labels = np.nonzero((support > 0) | (predicted > 0))[0]
    s, pr, t = support[labels], predicted[labels], tp[labels]
    div = lambda a, b: np.divide(a, b, out=np.zeros_like(a), where=b > 0)
    p, r, f = div(t, pr), div(t, s), div(2.0 * t, s + pr)
    n = float(s.sum())
    avg = {
        "macro": tuple(float(x.mean()) if len(labels) else 0.0 for x in (p, r, f)),
        "weighted": tuple(float((x * s).sum() / n) if n > 0 else 0.0 for x in (p, r, f)),
    }
    micro = float(t.sum() / n) if n > 0 else 0.0
    avg["micro"] = (micro, micro, micro)
    return labels, p, r, f, s, avg


def _average_ranks(x: np.ndarray) -> np.ndarray:
    """1-based ranks with ties given their average rank"""
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    end = np.cumsum(cnt).astype(np.float64)
    return (end - (cnt - 1) / 2.0)[inv.reshape(-1)]


def roc_auc_ovr_macro(targets: np.ndarray, probabilities: np.ndarray) -> Optional[float]:
    """sklearn's roc_auc_score(targets, probabilities, multi_class='ovr', average='macro'), rank-based (Mann-Whitney with
    ties counted half), or None where sklearn raises: fewer than three classes, a class of the columns absent from the
    targets, a non-finite score, rows that do not sum to 1."""
    y = np.asarray(targets).reshape(-1)
    P = np.asarray(probabilities)
    if P.ndim != 2 or P.shape[0] != y.shape[0] or P.shape[0] == 0:
        return None
    C_ = P.shape[1]
    if C_ < 3 or not np.array_equal(np.unique(y), np.arange(C_)):
        return None
    if not np.isfinite(P).all() or not np.allclose(1, P.sum(axis=1)):
        return None
    aucs = []
    for c in range(C_):
        pos = y == c
        n_pos, n_neg = int(pos.sum()), int((~pos).sum())
        ranks = _average_ranks(P[:, c].astype(np.float64))
        aucs.append((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))
    return float(np.mean(aucs))


def _report(labels, p, r, f, s, avg, names, accuracy) -> Dict:
    names = list(names) if names is not None else None
    if names is not None and len(names) == len(labels):
        keys = names                                                     # sklearn: names taken in order of the labels
    elif names is not None:
        keys = [names[l] if l < len(names) else str(l) for l in labels]  # the documented deviation (sklearn raises)
    else:
        keys = [str(l) for l in labels]
    out = {k: {"precision": float(p[i]), "recall": float(r[i]), "f1-score": float(f[i]), "support": float(s[i])}
           for i, k in enumerate(keys)}
    n = float(s.sum())
    out["accuracy"] = accuracy
    for kind in ("macro", "weighted"):
        ap, ar, af = avg[kind]
        out[f"{kind} avg"] = {"precision": ap, "recall": ar, "f1-score": af, "support": n}
    return out


def head_metrics(conf: np.ndarray) -> Dict[str, float]:
    """accuracy, f1_macro and f1_weighted of one confusion matrix (the reference's individual / scenario metrics)"""
    labels, p, r, f, s, avg = prf_from_confusion(conf)
    n = float(np.asarray(conf).sum())
    acc = float(np.trace(conf) / n) if n > 0 else 0.0
    return {"accuracy": acc, "f1_macro": avg["macro"][2], "f1_weighted": avg["weighted"][2]}


def finalize(counts: np.ndarray, sums: np.ndarray, num_classes: int, heads: int = 1,
             names: Optional[Sequence[str]] = None, probabilities: Optional[np.ndarray] = None,
             targets: Optional[np.ndarray] = None) -> Dict:
    """The accumulators of ``mmf_eval_accumulate`` -> the keys of the reference's ``_calculate_metrics``
    (evaluate_model.py:145-203), plus ``val_loss`` (the mean of the batch-mean losses, advanced_trainer.py:247),
    ``confusion_matrix`` (head 0), ``num_samples`` and, with ``heads`` > 1, ``individual_metrics`` (one dict per extra
    head).  ``roc_auc`` needs ``probabilities`` and ``targets`` (None otherwise).  Raises ValueError if a target was
    outside 0..C-1 (the kernel counted it and used it nowhere)."""
    conf, invalid, batches = split_counts(counts, num_classes, heads)
    if invalid:
        raise ValueError(f"{invalid} target(s) outside 0..{num_classes - 1}: no metric is computed")
    sums = np.asarray(sums, dtype=np.float64)
    main = conf[0]
    n = int(main.sum())
    labels, p, r, f, s, avg = prf_from_confusion(main)
    n_correct = int(np.trace(main))
    accuracy = n_correct / n if n else 0.0
    loss_sum, sp, sp2, spc = (float(x) for x in sums[:4])
    mean_p = sp / n if n else float("nan")
    confidence_stats = {
        "mean_confidence": mean_p,
        "mean_confidence_correct": spc / n_correct if n_correct else float("nan"),       # np.mean([]) is nan
        "mean_confidence_incorrect": (sp - spc) / (n - n_correct) if n > n_correct else 0,
        "confidence_std": float(np.sqrt(max(sp2 / n - mean_p * mean_p, 0.0))) if n else float("nan"),
    }
    roc_auc = roc_auc_ovr_macro(targets, probabilities) if probabilities is not None and targets is not None else None
    out = {
        "accuracy": accuracy,
        "f1_macro": avg["macro"][2], "f1_weighted": avg["weighted"][2], "f1_micro": avg["micro"][2],
        "precision_macro": avg["macro"][0], "precision_weighted": avg["weighted"][0],
        "recall_macro": avg["macro"][1], "recall_weighted": avg["weighted"][1],
        "roc_auc": roc_auc,
        "per_class_f1": f.tolist(), "per_class_precision": p.tolist(), "per_class_recall": r.tolist(),
        "classification_report": _report(labels, p, r, f, s, avg, names, accuracy),
        "confidence_stats": confidence_stats,
        "val_loss": loss_sum / batches if batches else float("nan"),
        "confusion_matrix": main.copy(),
        "num_samples": n,
    }
    if heads > 1:
        out["individual_metrics"] = [head_metrics(conf[h]) for h in range(1, heads)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the evaluation passes
# ---------------------------------------------------------------------------------------------------------------------
def _to_device(batch: Dict, device) -> Dict:
    out = {}
    for k, v in batch.items():
        if isinstance(v, dict):
            out[k] = {kk: vv.to(device, non_blocking=True) if torch.is_tensor(vv) else vv for kk, vv in v.items()}
        else:
            out[k] = v.to(device, non_blocking=True) if torch.is_tensor(v) else v
    return out


def _model_device(model) -> torch.device:
    return next(model.parameters()).device


def _capacity_hint(batches) -> int:
    try:
        return max(len(batches) * 16, 16)
    except TypeError:
        return 1024


def validate(model, batches: Iterable[Dict], labels: Optional[Sequence[str]] = None, label_smoothing: float = 0.1):
    """``AdvancedTrainer.validate`` (advanced_trainer.py:209-263) -> (metrics, class_report, predictions, targets,
    probabilities): ``metrics`` = {val_loss, val_accuracy, val_f1_macro, val_f1_weighted}, ``class_report`` in
    classification_report's output_dict layout (names ``labels``), predictions / targets (N,) int64 and probabilities
    (N, C) f32 numpy arrays.  ``val_loss`` is the mean of the batch means of CrossEntropyLoss(label_smoothing)."""
    model.eval()
    dev = _model_device(model)
    acc = None
    with torch.no_grad():
        for batch in batches:
            batch = _to_device(batch, dev)
            out = model(text_input=batch["text"], audio_input=batch["audio"], video_input=batch["video"])
            logits = out["emotion_logits"]
            if acc is None:
                acc = EvalAccumulator(logits.shape[-1], 1, label_smoothing, _capacity_hint(batches), dev)
            acc.update(logits, batch["emotion"])
    if acc is None:
        raise ValueError("validate: no batches")
    preds, targets, probs = acc.collected()
    m = acc.compute(labels, probs, targets)
    metrics = {"val_loss": m["val_loss"], "val_accuracy": m["accuracy"], "val_f1_macro": m["f1_macro"],
               "val_f1_weighted": m["f1_weighted"]}
    return metrics, m["classification_report"], preds, targets, probs


_METRIC_KEYS = ("accuracy", "f1_macro", "f1_weighted", "f1_micro", "precision_macro", "precision_weighted", "recall_macro",
                "recall_weighted", "roc_auc", "per_class_f1", "per_class_precision", "per_class_recall",
                "classification_report", "confidence_stats")


def evaluate_dataset(model, batches: Iterable[Dict], labels: Optional[Sequence[str]] = None,
                     label_smoothing: float = 0.1) -> Dict:
    """``ModelEvaluator.evaluate_dataset`` (evaluate_model.py:55-143) -> {metrics, individual_metrics, predictions,
    targets, probabilities, features}: ``metrics`` with the keys of ``_calculate_metrics``, ``individual_metrics``
    {text, audio, video: {accuracy, f1_macro, f1_weighted}} when the model emits ``individual_logits`` (late fusion,
    else {}), ``features`` = (text + audio + video features) / 3 (N, d) or None."""
    model.eval()
    dev = _model_device(model)
    acc, feats, mods = None, [], []
    with torch.no_grad():
        for batch in batches:
            batch = _to_device(batch, dev)
            out = model(text_input=batch["text"], audio_input=batch["audio"], video_input=batch["video"])
            logits = out["emotion_logits"]
            ind = out.get("individual_logits")
            if acc is None:
                mods = [m for m in MODALITIES if ind and m in ind]
                acc = EvalAccumulator(logits.shape[-1], 1 + len(mods), label_smoothing, _capacity_hint(batches), dev)
            acc.update(logits, batch["emotion"], [ind[m] for m in mods] if mods else None)
            if "text_features" in out:
                feats.append((out["text_features"] + out["audio_features"] + out["video_features"]) / 3)
    if acc is None:
        raise ValueError("evaluate_dataset: no batches")
    preds, targets, probs = acc.collected()
    m = acc.compute(labels, probs, targets)
    features = None
    if feats:
        buf = torch.cat(feats, dim=0)                                   # (N, d) on the device, one copy to the host
        features = buf.float().cpu().numpy()
    individual = {mod: m["individual_metrics"][i] for i, mod in enumerate(mods)} if mods else {}
    return {"metrics": {k: m[k] for k in _METRIC_KEYS}, "individual_metrics": individual, "predictions": preds,
            "targets": targets, "probabilities": probs, "features": features}


def evaluate_robustness(model, batches: Iterable[Dict]) -> Dict[str, Dict[str, float]]:
    """``RobustnessTrainer.evaluate_robustness`` (advanced_trainer.py:607-660): for each of the seven missing-modality
    scenarios {accuracy, f1_macro}, keyed 'all', 'text_missing', ..., 'audio_video_missing'.  The logits are
    ``robust_prediction`` for a RobustMultimodalModel and ``emotion_logits`` otherwise.  ``batches`` is iterated once
    per scenario (a list or a DataLoader)."""
    from models.multimodal_model import RobustMultimodalModel
    key = "robust_prediction" if isinstance(model, RobustMultimodalModel) else "emotion_logits"
    dev = _model_device(model)
    results = {}
    for missing in SCENARIOS:
        model.eval()
        acc = None
        with torch.no_grad():
            for batch in batches:
                batch = _to_device(batch, dev)
                out = model(text_input=batch["text"], audio_input=batch["audio"], video_input=batch["video"],
                            missing_modalities=missing)
                logits = out[key]
                if acc is None:
                    acc = EvalAccumulator(logits.shape[-1], 1, device=dev)
                acc.update(logits, batch["emotion"])
        if acc is None:
            raise ValueError("evaluate_robustness: no batches")
        m = acc.compute()
        results[scenario_name(missing)] = {"accuracy": m["accuracy"], "f1_macro": m["f1_macro"]}
    return results
