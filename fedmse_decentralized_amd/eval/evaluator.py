"""Batched evaluation of many clients (reference ``Evaluator.evaluate``,
`src/Evaluator/evaluator.py:50-127`).

The reference evaluates the N clients one after another, 12 rows per
forward, and moves every score/latent to the host for sklearn/scipy.  Here
all hosted clients are evaluated with a handful of launches:

* ``autoencoder``: one ``forward_rows`` over every client's test set
  (per-row SSE); anomaly score = SSE / D (``MSELoss(reduction='none')
  .mean(1)``); AUC on the device.
* ``hybrid`` (SAE-CEN): one ``forward_rows`` returning latents for every
  client's train and test sets; CEN scaler + distance and AUC on the device
  (`src/Model/Centroid.py:15-35`).  With ``engine.latent_scorer == "knn"``
  (not in the reference) the distance is to the ``engine.knn_k``-th nearest
  train latent instead of the centroid (``Engine.latent_scores``).

``metric="detection"`` / ``"tpr_at_fpr"`` (not in the reference) return F1 /
recall at a threshold calibrated per client (README "Detection thresholds");
``detection`` adds every client's validation rows to the forward.
``metric="classification"`` returns F1 at threshold 0.5 (plus P/R),
``metric="time"`` the wall time of the scoring pass (the reference's
``"time"`` branch is broken).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .metrics import DETECT_METRICS, calibration_rank, classification_metrics, detection_fields


@dataclass
class EvalResult:
    metrics: np.ndarray                       # [k] per evaluated client
    extra: Dict[str, np.ndarray] = field(default_factory=dict)
    latents: Optional[List[Tuple[np.ndarray, np.ndarray]]] = None  # (test_latent, labels) per client


def detection_ranks(engine, local_ids: Sequence[int], metric: str) -> List[int]:
    """The calibration rank of each client (host side; the kernel takes it as
    an int32): ``detection`` ranks the client's validation rows at
    ``engine.detect_quantile``, ``tpr_at_fpr`` its normal test rows at
    ``1 - engine.target_fpr``."""
    st = engine.store
    if metric == "detection":
        return [calibration_rank(int(st.valid_off[c + 1] - st.valid_off[c]), engine.detect_quantile)
                for c in local_ids]
    return [calibration_rank(int(np.count_nonzero(st.labels(c) == 0)), 1.0 - engine.target_fpr) for c in local_ids]


def detection_result(rows: np.ndarray, latents=None) -> "EvalResult":
    """EvalResult of a ``[8, k]`` detect_metrics result: row 0 is the metric."""
    rows = np.asarray(rows, dtype=np.float64)
    return EvalResult(rows[0].copy(), detection_fields(rows), latents)


def _evaluate_detection(engine, local_ids, model_type, metric, keep_latents) -> "EvalResult":
    """``detection`` / ``tpr_at_fpr``: the scores of ``evaluate_clients``
    (for the AE the raw fp32 SSE, scaled by 1/D where it is read), the
    calibration vector, then ``engine.detect_metrics``."""
    st = engine.store
    with_valid = metric == "detection"
    splits = (["train"] if model_type == "hybrid" else []) + ["test"] + (["valid"] if with_valid else [])
    items = [(c, st.rows(s, c)) for c in local_ids for s in splits]
    m = len(splits)
    test_lat = None
    if model_type == "autoencoder":
        sse, _ = engine.forward_rows(st.params, items, want_sse=True, want_latent=False)
        scores = sse[0::m]
        calib = sse[1::m] if with_valid else scores
        scale = 1.0 / engine.dims.d_in
    else:
        _, lat = engine.forward_rows(st.params, items, want_sse=False, want_latent=True)
        tr, test_lat = lat[0::m], lat[1::m]
        scores = engine.latent_scores(tr, test_lat)
        # validation latents under the scaler fitted on the train latents
        calib = engine.latent_scores(tr, lat[2::m]) if with_valid else scores
        scale = 1.0
    labels = [st.test_label[int(st.test_off[c]):int(st.test_off[c + 1])] for c in local_ids]
    rows = engine.detect_metrics(calib, scores, labels, detection_ranks(engine, local_ids, metric),
                                 calib_labels=None if with_valid else labels, score_scale=scale,
                                 value="f1" if with_valid else "recall")
    latents = None
    if keep_latents and test_lat is not None:
        latents = [(l.detach().cpu().numpy().astype(np.float32), st.labels(c).astype(np.float32))
                   for l, c in zip(test_lat, local_ids)]
    return detection_result(rows, latents)


def evaluate_clients(engine, local_ids: Sequence[int], model_type: str, metric: str = "AUC",
                     keep_latents: bool = False) -> EvalResult:
    st = engine.store
    D = engine.dims.d_in
    t0 = time.perf_counter()
    if metric in DETECT_METRICS:
        if model_type not in ("autoencoder", "hybrid"):
            raise ValueError(f"unknown model_type {model_type!r}")
        return _evaluate_detection(engine, local_ids, model_type, metric, keep_latents)
    if model_type == "autoencoder":
        items = [(c, st.rows("test", c)) for c in local_ids]
        sse, _ = engine.forward_rows(st.params, items, want_sse=True, want_latent=False)
        scores = [s / D for s in sse]
        test_lat = None
    elif model_type == "hybrid":
        items = []
        for c in local_ids:
            items.append((c, st.rows("train", c)))
            items.append((c, st.rows("test", c)))
        _, lat = engine.forward_rows(st.params, items, want_sse=False, want_latent=True)
        tr = lat[0::2]
        test_lat = lat[1::2]
        scores = engine.latent_scores(tr, test_lat)
    else:
        raise ValueError(f"unknown model_type {model_type!r}")
    labels = [st.test_label[int(st.test_off[c]):int(st.test_off[c + 1])] for c in local_ids]
    extra = {}
    if metric == "AUC":
        vals = engine.auc(scores, labels)
    elif metric == "classification":
        f1s, ps, rs = [], [], []
        for s, c in zip(scores, local_ids):
            f1, p, r = classification_metrics(st.labels(c), s.detach().cpu().numpy())
            f1s.append(f1)
            ps.append(p)
            rs.append(r)
        vals = np.asarray(f1s)
        extra = {"precision": np.asarray(ps), "recall": np.asarray(rs)}
    elif metric == "time":
        engine.synchronize()
        vals = np.full(len(local_ids), time.perf_counter() - t0)
    else:
        raise ValueError(f"unknown metric {metric!r}")
    latents = None
    if keep_latents and test_lat is not None:
        latents = [(l.detach().cpu().numpy().astype(np.float32), st.labels(c).astype(np.float32))
                   for l, c in zip(test_lat, local_ids)]
    return EvalResult(np.asarray(vals, dtype=np.float64), extra, latents)
