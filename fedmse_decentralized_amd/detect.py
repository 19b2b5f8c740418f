"""Score raw traffic with an exported detector (README "Deploying a detector").

    python -m fedmse_decentralized_amd.detect --detector PATH/detector.npz \\
        --input traffic.csv [--output alarms.npz] [--backend auto|hip|torch] [--explain K]
        [--monitor [--monitor-top N]]
        [--incidents [--incident-window W] [--incident-min M|auto] [--incident-tail P] [--incident-hold H]
         [--signatures N [--signature-top K]]]

``--input`` is one headerless CSV of raw feature rows (one column per model
input) or a directory of them, read in sorted file-name order by the
package's reader.  ``--output`` receives ``scores`` (float64, cleaned),
``flags`` (uint8, 1 = alarm), ``alarms`` and ``threshold``.  One line with the
row count, the alarm count and the scoring rate goes to stdout.

``--explain K`` (README "Explaining an alarm") also ranks, for every flagged
row, the K features the model reconstructed worst and adds to ``--output``:
``explain_rows`` (the flagged rows' indices), ``explain_idx`` (feature indices,
worst first; -1 unused), ``explain_resid`` (reconstruction minus observation in
standardised units), ``explain_share`` (the feature's part of the row's squared
error), ``explain_observed`` and ``explain_expected`` (the raw value and what
the model expected, in raw units).

``--monitor`` (README "Monitoring a deployed detector") also compares the rows
with the baseline the bundle was exported with (``--export-baseline``): a second
line ``monitor: alarm_rate ... expected ... psi ... worst features d:out_share
...`` names the ``--monitor-top`` (default 5) features with the largest share of
values outside the train band, and ``--output`` gains one ``monitor_*`` array per
``DriftReport`` field.  A bundle without a baseline is monitored without band and
histogram (``baseline none``).

``--incidents`` (README "Incidents") also groups the flagged rows into
incidents: a row is hot when at least ``--incident-min`` of the last
``--incident-window`` (default 64) rows are flagged, and hot rows with at most
``--incident-hold`` (default: the window) other rows between them form one
incident.  ``--incident-min auto`` (the default) takes the smallest count whose
chance under independent benign flags at rate ``1 - detect_quantile`` is at
most ``--incident-tail`` (default 1e-6).  A line ``incidents: count K
rows_covered R longest L hot_rows H window W min M hold H`` follows, and
``--output`` gains ``incident_start``, ``incident_end``, ``incident_alarms``,
``incident_peak_row``, ``incident_peak_score`` and ``incident_params`` (window,
min, hold).  Rows are in time order: a directory's files are concatenated in
sorted name order and a window runs across file boundaries.

``--signatures N`` (README "Incident signatures"; needs ``--incidents``) also
says what the N incidents with the most alarms (equal counts: the smaller
index; reported in rising index order) are about: per incident the
``--signature-top`` (default 5) features with the largest summed squared
residual over the incident's flagged rows, their share of it and their mean
residual.  A line ``# signatures: incidents S top_k K incident k rows R
d:share:mean_resid ...`` follows, and ``--output`` gains ``signature_incident``,
``signature_rows``, ``signature_idx``, ``signature_share``,
``signature_mean_resid``, ``signature_err_sum``, ``signature_resid_sum``,
``signature_bad`` and ``signature_similarity`` (the cosines between the
incidents' ``err_sum`` rows).
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys
import time

import numpy as np
import torch

from .data.csv import load_data
from .deploy.detector import (EXPLAIN_MAX_K, INCIDENT_MAX_HOLD, INCIDENT_MAX_WINDOW, SIGNATURE_MAX_INCIDENTS, Detector,
                              expected_raw, incident_min_alarms)
from .engine import make_engine
from .ops import _host


def read_rows(path: str) -> np.ndarray:
    if os.path.isdir(path):
        return np.asarray(load_data(path, cache=False), dtype=np.float64)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"input not found: {path}")
    return np.asarray(_host.read_csv(path), dtype=np.float64)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m fedmse_decentralized_amd.detect", description=__doc__.split("\n")[0])
    ap.add_argument("--detector", required=True, help="detector.npz written by a run with --export-detectors")
    ap.add_argument("--input", required=True, help="headerless CSV of raw rows, or a directory of them")
    ap.add_argument("--output", default=None, help="write scores and flags to this .npz")
    ap.add_argument("--backend", default="auto", choices=("auto", "hip", "torch"))
    ap.add_argument("--explain", type=int, default=None, metavar="K",
                    help=f"rank the K (1..{EXPLAIN_MAX_K}) worst-reconstructed features of every flagged row")
    ap.add_argument("--monitor", action="store_true",
                    help="compare the rows with the bundle's baseline: per-feature drift and score histogram")
    ap.add_argument("--monitor-top", type=int, default=5, metavar="N",
                    help="features named on the monitor line, by falling share outside the train band (default 5)")
    ap.add_argument("--incidents", action="store_true",
                    help="group the flagged rows into incidents: m of the last w rows, runs joined across short gaps")
    ap.add_argument("--incident-window", type=int, default=64, metavar="W",
                    help=f"rows the alarm count looks back over (1..{INCIDENT_MAX_WINDOW}; default 64)")
    ap.add_argument("--incident-min", default="auto", metavar="M|auto",
                    help="flagged rows in the window that make a row hot (1..W), or auto: from --incident-tail")
    ap.add_argument("--incident-tail", type=float, default=1e-6, metavar="P",
                    help="auto: the chance of a hot row under independent benign flags stays at or below P")
    ap.add_argument("--incident-hold", type=int, default=None, metavar="H",
                    help=f"hot rows at most H other rows apart share an incident (0..{INCIDENT_MAX_HOLD}; default W)")
    ap.add_argument("--signatures", type=int, default=None, metavar="N",
                    help="with --incidents: per-feature residual profile of the N incidents with the most alarms")
    ap.add_argument("--signature-top", type=int, default=5, metavar="K",
                    help=f"features named per incident, by falling summed squared residual (1..{EXPLAIN_MAX_K}; "
                         "default 5)")
    ns = ap.parse_args(argv)
    if ns.signatures is not None:
        if not ns.incidents:
            ap.error("--signatures needs --incidents")
        if not 1 <= ns.signatures <= SIGNATURE_MAX_INCIDENTS:
            ap.error(f"--signatures takes 1..{SIGNATURE_MAX_INCIDENTS}")
        if not 1 <= ns.signature_top <= EXPLAIN_MAX_K:
            ap.error(f"--signature-top takes 1..{EXPLAIN_MAX_K}")
    if not 1 <= ns.incident_window <= INCIDENT_MAX_WINDOW:
        ap.error(f"--incident-window takes 1..{INCIDENT_MAX_WINDOW}")
    hold = ns.incident_window if ns.incident_hold is None else ns.incident_hold
    if not 0 <= hold <= INCIDENT_MAX_HOLD:
        ap.error(f"--incident-hold takes 0..{INCIDENT_MAX_HOLD}")
    if not 0.0 < ns.incident_tail < 1.0:
        ap.error("--incident-tail takes a probability between 0 and 1")
    if ns.incident_min != "auto":
        try:
            ns.incident_min = int(ns.incident_min)
        except ValueError:
            ap.error("--incident-min takes a count or auto")
        if not 1 <= ns.incident_min <= ns.incident_window:
            ap.error("--incident-min takes 1..W (the window) or auto")
    if ns.monitor_top < 0:
        ap.error("--monitor-top takes a count >= 0")
    if ns.explain is not None and not 1 <= ns.explain <= EXPLAIN_MAX_K:
        ap.error(f"--explain takes 1..{EXPLAIN_MAX_K}")
    det = Detector.load(ns.detector)
    rows = read_rows(ns.input)
    if rows.ndim != 2 or rows.shape[1] != det.dims.d_in:
        raise SystemExit(f"{ns.input}: rows have {rows.shape[1] if rows.ndim == 2 else '?'} columns, the detector "
                         f"takes {det.dims.d_in}")
    device = "cuda" if ns.backend == "hip" or (ns.backend == "auto" and torch.cuda.is_available()) else "cpu"
    eng = make_engine(ns.backend, det.dims, device)
    # with --monitor two calls read the rows: on a GPU engine they are uploaded once, ahead of both
    shared = torch.from_numpy(rows).to(eng.device) if (ns.monitor or ns.signatures is not None) \
        and eng.device.type == "cuda" else rows
    min_alarms = ns.incident_min
    if ns.incidents and min_alarms == "auto":
        if not 0.0 <= det.detect_quantile <= 1.0:
            ap.error("--incident-min auto needs the detector's detect_quantile; give a count")
        min_alarms = incident_min_alarms(ns.incident_window, 1.0 - det.detect_quantile, ns.incident_tail)
    inc = None
    t0 = time.perf_counter()
    if ns.incidents:
        scores, flags, alarms, inc = eng.score_incidents([det], [shared], ns.incident_window, min_alarms, hold)[0]
    else:
        scores, flags, alarms = eng.score_rows([det], [shared])[0]
    dt = time.perf_counter() - t0
    extra, tail = {}, ""
    if ns.explain is not None:
        extra = explain_flagged(eng, det, rows, flags, ns.explain)
        tail = f" explained {extra['explain_rows'].shape[0]} top_k {ns.explain}"
    monitor_line = None
    if ns.monitor:
        rep = eng.monitor_rows([det], [shared])[0]
        extra.update({"monitor_" + k: np.asarray(v) for k, v in dataclasses.asdict(rep).items() if v is not None})
        monitor_line = monitor_summary(det, rep, ns.monitor_top)
    if inc is not None:
        extra.update({"incident_" + k: getattr(inc, k) for k in ("start", "end", "alarms", "peak_row", "peak_score")})
        extra["incident_params"] = np.array([inc.window, inc.min_alarms, inc.hold], dtype=np.int64)
    signature_line = None
    if ns.signatures is not None:
        sig = eng.incident_signatures([det], [shared], [flags], [inc], top_k=ns.signature_top,
                                      which=[largest_incidents(inc, ns.signatures)])[0]
        extra.update({"signature_incident": sig.incidents, "signature_rows": sig.rows, "signature_idx": sig.idx,
                      "signature_share": sig.share, "signature_mean_resid": sig.mean_resid,
                      "signature_err_sum": sig.err_sum, "signature_resid_sum": sig.resid_sum,
                      "signature_bad": sig.bad, "signature_similarity": sig.similarity()})
        signature_line = signature_summary(sig, ns.signature_top)
    if ns.output:
        with open(ns.output, "wb") as f:
            np.savez(f, scores=scores, flags=flags, alarms=np.array(alarms, dtype=np.int64),
                     threshold=np.array(det.threshold, dtype=np.float64), **extra)
    n = int(scores.shape[0])
    rate = n / dt if dt > 0 else float("inf")
    print(f"detect: rows {n} alarms {alarms} threshold {det.threshold:.9g} backend {eng.name} "
          f"rows_per_s {rate:.1f}{tail}")
    if monitor_line is not None:
        print(monitor_line)
    if inc is not None:
        print(f"incidents: count {inc.count} rows_covered {inc.rows_covered} longest {inc.longest} "
              f"hot_rows {inc.hot_rows} window {inc.window} min {inc.min_alarms} hold {inc.hold}")
    if signature_line is not None:
        print(signature_line)
    return 0


def largest_incidents(inc, count: int) -> np.ndarray:
    """The ``count`` incidents with the most alarms (equal counts: the smaller
    index), as rising indices."""
    order = np.argsort(-inc.alarms, kind="stable")[:max(0, int(count))]
    return np.sort(order).astype(np.int64)


def signature_summary(sig, top_k: int) -> str:
    """The ``# signatures:`` line: per summarised incident its index, its
    flagged rows and ``feature:share:mean_resid`` of its leading features."""
    parts = [f"# signatures: incidents {sig.incidents.shape[0]} top_k {int(top_k)}"]
    for j, k in enumerate(sig.incidents):
        feats = " ".join(f"{int(d)}:{sig.share[j, i]:.4g}:{sig.mean_resid[j, i]:.4g}"
                         for i, d in enumerate(sig.idx[j]) if d >= 0)
        parts.append(f"incident {int(k)} rows {int(sig.rows[j])} {feats}")
    return " ".join(parts)


def monitor_summary(det: Detector, rep, top: int) -> str:
    """The ``monitor:`` line: the ``top`` features with the largest
    ``out_share``, equal shares by rising feature index."""
    order = np.argsort(-rep.out_share, kind="stable")[:max(0, min(int(top), det.dims.d_in))]
    worst = " ".join(f"{int(d)}:{rep.out_share[d]:.4g}" for d in order)
    base = "" if det.baseline is not None else " baseline none"
    return (f"monitor: alarm_rate {rep.alarm_rate:.6g} expected {rep.expected_alarm_rate:.6g} psi {rep.psi:.6g} "
            f"worst features {worst}{base}")


def explain_flagged(eng, det: Detector, rows: np.ndarray, flags: np.ndarray, top_k: int) -> dict:
    """The ``explain_*`` arrays of ``--output`` for the flagged rows."""
    which = np.flatnonzero(flags).astype(np.int64)
    ex = eng.explain_rows([det], [rows], top_k=top_k, which=[which])[0]
    used = ex.idx >= 0
    col = np.where(used, ex.idx, 0)
    picked = rows[which]
    with np.errstate(all="ignore"):
        e = (ex.resid * ex.resid).astype(np.float64)   # fp32 product, as the ranking key
        share = np.where(used, e / ex.sse.astype(np.float64)[:, None], 0.0)
    observed = np.where(used, np.take_along_axis(picked, col, axis=1), np.nan)
    x_std = np.take_along_axis(det.standardise(picked), col, axis=1)
    return {"explain_rows": ex.rows, "explain_idx": ex.idx, "explain_resid": ex.resid, "explain_share": share,
            "explain_observed": observed, "explain_expected": expected_raw(det, x_std, ex.resid, ex.idx)}


if __name__ == "__main__":
    sys.exit(main())
