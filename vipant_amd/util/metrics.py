"""Multi-label tagging metrics of BCELossHead.report (cvap/module/decoder/loss_more.py:86-131) in numpy.

The reference calls scikit-learn (`average_precision_score` with its three averages, `roc_auc_score`, `precision_recall_curve`);
the package does not depend on it at run time, so the four quantities are restated here with scikit-learn's definitions
(tests/test_cls_cpu.py compares them with scikit-learn where it is installed):

  * thresholds are the DISTINCT score values, in decreasing order; tied scores enter a threshold together;
  * precision = tp / (tp + fp), recall = tp / #positives, with the closing point (precision 1, recall 0) appended;
  * average precision = sum over thresholds of (recall step) x precision -- no interpolation;
  * ROC-AUC = trapezoidal area under (fp / #negatives, tp / #positives), starting from (0, 0): ties count one half;
  * a class without a positive has recall 1 at every threshold and average precision 0; ROC-AUC is undefined for a class
    without a positive or without a negative -- the reference counts it 0 and prints `Err(True)`.
"""
from __future__ import annotations

import numpy as np

__all__ = ["binary_curve", "precision_recall_curve", "average_precision", "roc_auc", "average_precision_score",
           "multilabel_report"]


def binary_curve(y_true, y_score):
    """(fps, tps, thresholds) at every distinct score, decreasing: the counts of negatives / positives scored >= threshold."""
    y_true = np.asarray(y_true).ravel() != 0
    y_score = np.asarray(y_score).ravel()
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    idx = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    return fps, tps, y_score[idx]


def precision_recall_curve(y_true, y_score):
    """(precision, recall, thresholds) with recall decreasing and the closing point (1, 0) appended."""
    fps, tps, thr = binary_curve(y_true, y_score)
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=(ps != 0))
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    return np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0)), thr[::-1]


def average_precision(y_true, y_score) -> float:
    precision, recall, _ = precision_recall_curve(y_true, y_score)
    return max(0.0, float(-np.sum(np.diff(recall) * precision[:-1])))


def roc_auc(y_true, y_score) -> float:
    """ROC-AUC of one class; ValueError when only one class is present (as scikit-learn raises)."""
    fps, tps, _ = binary_curve(y_true, y_score)
    if tps[-1] == 0 or fps[-1] == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    fpr, tpr = np.r_[0.0, fps] / fps[-1], np.r_[0.0, tps] / tps[-1]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) * 0.5))


def average_precision_score(y_true, y_score, average="macro"):
    """y_true, y_score [n, c].  average: "micro" (all entries as one problem), "macro" (mean over classes), "weighted" (classes
    weighted by their positives; 0 without any positive), None (per class)."""
    y_true, y_score = np.asarray(y_true), np.asarray(y_score)
    if average == "micro":
        return average_precision(y_true.ravel(), y_score.ravel())
    per_class = np.array([average_precision(y_true[:, k], y_score[:, k]) for k in range(y_true.shape[1])])
    if average is None:
        return per_class
    if average == "weighted":
        weight = (y_true != 0).sum(0).astype(np.float64)
        if np.isclose(weight.sum(), 0.0):
            return 0
        return float(np.average(per_class, weights=weight))
    return float(np.mean(per_class))


def multilabel_report(x2s, x1s) -> str:
    """The report string of loss_more.py:94-131: x2s targets [n, c], x1s scores [n, c]."""
    x2s, x1s = np.asarray(x2s), np.asarray(x1s)
    nsample, nlabel = x1s.shape[:2]
    ap_list = average_precision_score(x2s, x1s, average=None)
    ap_micro = average_precision_score(x2s, x1s, average="micro")
    ap_macro = float(np.mean(ap_list))
    weight = (x2s != 0).sum(0).astype(np.float64)
    ap_weighted = 0 if np.isclose(weight.sum(), 0.0) else float(np.average(ap_list, weights=weight))
    has_err = False
    auc_list, precisions, recalls = [], [], []
    for k in range(nlabel):
        y_true, y_score = x2s[:, k], x1s[:, k]
        try:
            auc = roc_auc(y_true, y_score)
        except ValueError:
            auc = 0.
            has_err = True
        p, r, _ = precision_recall_curve(y_true, y_score)
        mid = len(p) // 2
        auc_list.append(auc)
        precisions.append(p[mid])
        recalls.append(r[mid])
    mean_ap, mean_auc = np.mean(ap_list) * 100., np.mean(auc_list) * 100.
    mean_p, mean_r = np.mean(precisions) * 100., np.mean(recalls) * 100.
    text = f"Err({has_err}) mAP = {mean_ap:2.2f} mAUC = {mean_auc:2.2f} mP = {mean_p:2.2f} mR = {mean_r:2.2f}"
    common = f"Mac-AP = {ap_macro:2.2f} Mic-AP = {ap_micro:2.2f} wAP = {ap_weighted:2.2f}"
    return f"{common} {text} @ {nsample}"
