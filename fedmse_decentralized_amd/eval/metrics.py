"""Detection metrics (reference `src/Evaluator/evaluator.py:21-48`).

* ROC-AUC with sklearn ``roc_curve`` + ``auc`` semantics (positives = label 1,
  ties count one half, non-finite scores replaced by ``nan_to_num``).  The
  trapezoid area under sklearn's ROC is exactly the Mann-Whitney statistic
  with mid-ranks, which is what the host library and the device kernel
  compute; parity against sklearn is pinned in ``tests/test_metrics.py``.
* classification metrics at a fixed score threshold (F1 / precision / recall,
  ``score > 0.5`` -> anomaly, `evaluator.py:30-48`), sklearn zero-division
  conventions (0.0 with a warning there).
* calibrated thresholds (not in the reference; README "Detection thresholds"):
  the rank of the calibration value used as threshold, and the per-client
  report formed from ``Engine.detect_metrics``' rows.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

from ..ops import _host

# metrics taken at a calibrated threshold (README "Detection thresholds"):
# "detection" calibrates on the client's own validation scores (all normal)
# and reports F1, "tpr_at_fpr" on the test set's normal scores and reports recall
DETECT_METRICS = ("detection", "tpr_at_fpr")
# rows of Engine.detect_metrics' [8, k] result
DETECT_ROWS = ("value", "threshold", "tp", "fp", "fn", "tn", "precision", "recall")
# what a round reports per client (RoundResult.detection, EvalResult.extra)
DETECT_FIELDS = ("threshold", "tp", "fp", "fn", "tn", "precision", "recall", "f1", "fpr")


def calibration_rank(n_c: int, q: float) -> int:
    """0-based rank of the calibration value used as threshold: the smallest
    rank with at least a share ``q`` of the ``n_c`` values at or below it;
    -1 (no threshold) without calibration values."""
    n_c = int(n_c)
    if n_c == 0:
        return -1
    return min(n_c - 1, max(0, math.ceil(q * n_c) - 1))


def detect_value_is_recall(metric_or_value: str) -> bool:
    if metric_or_value in ("f1", "detection"):
        return False
    if metric_or_value in ("recall", "tpr_at_fpr"):
        return True
    raise ValueError(f"detect_metrics value must be 'f1' or 'recall', got {metric_or_value!r}")


def detection_fields(rows: np.ndarray) -> Dict[str, np.ndarray]:
    """The per-client report of a ``[8, k]`` detect_metrics result: its rows
    1..7 by name, plus F1 and the false-positive rate formed from the exact
    counts (one f64 division each; NaN wherever precision is undefined)."""
    rows = np.asarray(rows, dtype=np.float64)
    out = {name: rows[i].copy() for i, name in enumerate(DETECT_ROWS) if i}
    tp, fp, fn, tn = out["tp"], out["fp"], out["fn"], out["tn"]
    undefined = np.isnan(out["precision"])
    f1 = np.zeros(rows.shape[1], dtype=np.float64)
    fpr = np.zeros(rows.shape[1], dtype=np.float64)
    for i in range(rows.shape[1]):
        den = 2 * tp[i] + fp[i] + fn[i]
        f1[i] = np.nan if undefined[i] else (2 * tp[i] / den if den else 0.0)
        den = fp[i] + tn[i]
        fpr[i] = np.nan if undefined[i] else (fp[i] / den if den else 0.0)
    out["f1"], out["fpr"] = f1, fpr
    return out


def detection_rows(value: np.ndarray, fields: Dict[str, np.ndarray]) -> np.ndarray:
    """Back to ``[8, k]`` rows (the form that travels through an all-reduce)."""
    return np.stack([np.asarray(value, dtype=np.float64)] + [np.asarray(fields[n], dtype=np.float64)
                                                             for n in DETECT_ROWS[1:]])


def roc_auc(labels, scores) -> float:
    s = np.asarray(scores, dtype=np.float64)
    if not np.all(np.isfinite(s)):
        s = np.nan_to_num(s)
    return _host.roc_auc(s, np.asarray(labels))


def read_scores(scores, f32_scale: float = 1.0) -> np.ndarray:
    """Scores as the AUC kernels read them: a float32 score times
    ``f32_scale`` in float32, then widened; a float64 score as is; then
    NaN -> 0 and +-inf -> +-DBL_MAX (``numpy.nan_to_num``)."""
    s = np.asarray(scores)
    if s.dtype == np.float32:
        s = (s * np.float32(f32_scale)).astype(np.float64)
    else:
        s = s.astype(np.float64)
    return np.nan_to_num(s)


def auc_chunked_numpy(scores, labels, chunk_keys: int, f32_scale: float = 1.0) -> float:
    """The rule of the multi-workgroup device AUC (README "Exact AUC at any
    size", fedmx_auc_large.hip) written out: the smaller class (the positives
    on a tie) is cut into chunks of ``chunk_keys`` values, each chunk is
    sorted, every value of the other class is searched in it, and the counts
    of smaller and of equal values are summed as integers.  Equal to
    ``_host.roc_auc`` of the read scores to the bit while P*N < 2^52."""
    s = read_scores(scores, f32_scale)
    pos = np.asarray(labels) != 0
    P = int(pos.sum())
    N = int(s.shape[0]) - P
    if P == 0 or N == 0:
        return float("nan")
    sort_pos = P <= N
    keys, probe = (s[pos], s[~pos]) if sort_pos else (s[~pos], s[pos])
    less = eq = 0
    for k0 in range(0, keys.shape[0], int(chunk_keys)):
        chunk = np.sort(keys[k0:k0 + int(chunk_keys)])
        lb = np.searchsorted(chunk, probe, side="left")
        ub = np.searchsorted(chunk, probe, side="right")
        less += int(lb.sum(dtype=np.int64))
        eq += int((ub - lb).sum(dtype=np.int64))
    pairs = float(P) * float(N)
    if sort_pos:
        return (pairs - float(less) - 0.5 * float(eq)) / pairs
    return (float(less) + 0.5 * float(eq)) / pairs


def classification_metrics(labels, scores, threshold: float = 0.5):
    y = np.asarray(labels).astype(np.int64)
    pred = (np.asarray(scores) > threshold).astype(np.int64)
    tp = int(np.sum((pred == 1) & (y == 1)))
    fp = int(np.sum((pred == 1) & (y == 0)))
    fn = int(np.sum((pred == 0) & (y == 1)))
    precision = tp / (tp + fp) if (tp + fp) else 0.0
    recall = tp / (tp + fn) if (tp + fn) else 0.0
    f1 = 2 * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) else 0.0
    return f1, precision, recall
