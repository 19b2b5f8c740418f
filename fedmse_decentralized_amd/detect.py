"""Score raw traffic with an exported detector (README "Deploying a detector").

    python -m fedmse_decentralized_amd.detect --detector PATH/detector.npz \\
        --input traffic.csv [--output alarms.npz] [--backend auto|hip|torch]

``--input`` is one headerless CSV of raw feature rows (one column per model
input) or a directory of them, read in sorted file-name order by the
package's reader.  ``--output`` receives ``scores`` (float64, cleaned),
``flags`` (uint8, 1 = alarm), ``alarms`` and ``threshold``.  One line with the
row count, the alarm count and the scoring rate goes to stdout.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

from .data.csv import load_data
from .deploy.detector import Detector
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
    ns = ap.parse_args(argv)
    det = Detector.load(ns.detector)
    rows = read_rows(ns.input)
    if rows.ndim != 2 or rows.shape[1] != det.dims.d_in:
        raise SystemExit(f"{ns.input}: rows have {rows.shape[1] if rows.ndim == 2 else '?'} columns, the detector "
                         f"takes {det.dims.d_in}")
    device = "cuda" if ns.backend == "hip" or (ns.backend == "auto" and torch.cuda.is_available()) else "cpu"
    eng = make_engine(ns.backend, det.dims, device)
    t0 = time.perf_counter()
    scores, flags, alarms = eng.score_rows([det], [rows])[0]
    dt = time.perf_counter() - t0
    if ns.output:
        with open(ns.output, "wb") as f:
            np.savez(f, scores=scores, flags=flags, alarms=np.array(alarms, dtype=np.int64),
                     threshold=np.array(det.threshold, dtype=np.float64))
    n = int(scores.shape[0])
    rate = n / dt if dt > 0 else float("inf")
    print(f"detect: rows {n} alarms {alarms} threshold {det.threshold:.9g} backend {eng.name} "
          f"rows_per_s {rate:.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
