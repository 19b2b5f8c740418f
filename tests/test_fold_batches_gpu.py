"""Second-stage kernels past their first batch, on the GPU, bit for bit:

* ``monitor_fold_kernel`` (fedmx_monitor.hip) alone through
  ``fedmx_monitor_fold`` on synthetic block partials: it loads 128 partials per
  batch, so 1, 127, 128, 129, 255, 256, 257 and 300 blocks, as eight detectors
  of one launch, against a plain numpy fold in block order;
* ``monitor_rows`` end to end over 130 blocks;
* the incident kernels (fedmx_incident.hip) past the 64 spans one step of
  ``incident_scan_kernel`` scans: 64, 64 and a row, 65 and 130 spans, with the
  edge patterns of tests/test_incidents_gpu.py at the 64-span edge.

(``incident_sig_fold_kernel`` past its four-block unroll:
tests/test_incident_signatures_gpu.py.)"""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.deploy.detector import incident_bound, incidents_numpy
from fedmse_decentralized_amd.models.layout import ModelDims

import test_incidents_gpu as inc
import test_monitor_rows_gpu as mon

DEV = torch.device("cuda", 0)
NBLOCKS = [1, 127, 128, 129, 255, 256, 257, 300]
BATCH = 128
COLS = 128
NEG_ZERO_COL, NAN_COL = 5, 9
FULL = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# monitor_fold_kernel
def make_partials():
    """One MONITOR_PARTIAL_DTYPE array per detector."""
    from fedmse_decentralized_amd.ops import _hip

    assert _hip.MONITOR_COLS == COLS
    rng = np.random.default_rng(2718)
    out = []
    for nb in NBLOCKS:
        p = np.zeros(nb, dtype=_hip.MONITOR_PARTIAL_DTYPE)
        for k in ("sum", "sq"):   # mixed signs over 1e-8 .. 1e8
            p[k] = rng.choice([-1.0, 1.0], size=(nb, COLS)) * 10.0 ** rng.uniform(-8, 8, size=(nb, COLS))
        p["mn"] = rng.normal(size=(nb, COLS)).astype(np.float32)
        p["mx"] = p["mn"] + np.abs(rng.normal(size=(nb, COLS))).astype(np.float32)
        p["mn"][:, 7] = np.float32(1.25)   # ties: the first one stays
        for k in ("cnt", "bad", "out"):
            p[k] = rng.integers(0, 1 << 20, size=(nb, COLS), dtype=np.uint32)
            for b in sorted({0, nb // 2, nb - 1}):   # three blocks (fewer in the shortest folds): totals pass 2^32
                p[k][b] = FULL
        p["pad"] = 0xDEADBEEF   # (not read)
        # empty blocks at the batch edges and at the end
        for b in (0, BATCH - 1, BATCH, 2 * BATCH - 1, 2 * BATCH, nb - 1):
            if b < nb and nb > 1:
                p["sum"][b], p["sq"][b], p["mn"][b], p["mx"][b] = 0.0, 0.0, np.inf, -np.inf
        p["sum"][:, NEG_ZERO_COL] = -0.0
        p["mn"][nb // 3, NAN_COL] = p["mx"][nb // 3, NAN_COL] = np.nan   # (no kernel writes one; a strict compare skips it)
        out.append(p)
    return out


def fold(p, order=None, batch=None):
    """The rule: from +0.0, one float64 add per block in block order, strict
    compares, int64 counters.  ``order``: another block order.  ``batch``: fold
    each batch of that many blocks from zero, then add the batch totals."""
    from fedmse_decentralized_amd.ops import _hip

    t = np.zeros((), dtype=_hip.MONITOR_TOTAL_DTYPE)
    order = range(p.shape[0]) if order is None else order
    for k in ("sum", "sq"):
        if batch is None:
            acc = np.zeros(COLS)
            for b in order:
                acc = acc + p[k][b]
        else:
            acc = np.zeros(COLS)
            for b0 in range(0, p.shape[0], batch):
                sub = np.zeros(COLS)
                for b in range(b0, min(b0 + batch, p.shape[0])):
                    sub = sub + p[k][b]
                acc = acc + sub
        t[k] = acc
    mn, mx = np.full(COLS, np.inf, np.float32), np.full(COLS, -np.inf, np.float32)
    for b in order:
        mn = np.where(p["mn"][b] < mn, p["mn"][b], mn)
        mx = np.where(p["mx"][b] > mx, p["mx"][b], mx)
    t["mn"], t["mx"] = mn, mx
    for k in ("cnt", "bad", "out"):
        t[k] = p[k].astype(np.int64).sum(axis=0)
    return t


@pytest.fixture(scope="module")
def partials():
    parts = make_partials()
    want = [fold(p) for p in parts]
    for p in parts:
        p.setflags(write=False)
    return parts, want


def test_wrong_folds_differ_from_the_reference(partials):
    """On the CPU: a fold in reverse block order and a fold that sums each
    128-block batch from zero both change some column's bits, so the
    comparison below tells them from the kernel's order."""
    parts, want = partials
    for p, w in zip(parts, want):
        nb = p.shape[0]
        assert w["sum"][NEG_ZERO_COL] == 0.0 and not np.signbit(w["sum"][NEG_ZERO_COL])
        if nb >= 3:
            assert all(np.all(w[k] > 1 << 32) for k in ("cnt", "bad", "out"))
        if nb > 2:
            r = fold(p, order=range(nb - 1, -1, -1))
            assert any(r[k].tobytes() != w[k].tobytes() for k in ("sum", "sq")), nb
        b = fold(p, batch=BATCH)
        if nb > BATCH + 1:
            assert any(b[k].tobytes() != w[k].tobytes() for k in ("sum", "sq")), nb
        else:
            assert b.tobytes() == w.tobytes()


def test_monitor_fold_kernel_matches_a_fold_in_block_order(partials):
    from fedmse_decentralized_amd.ops import _hip

    parts, want = partials
    P, T = _hip.MONITOR_PARTIAL_DTYPE, _hip.MONITOR_TOTAL_DTYPE
    rt = _hip.runtime(DEV)
    part = torch.from_numpy(np.concatenate(parts).view(np.uint8).copy()).to(DEV)
    total = torch.full(((len(parts) + 1) * T.itemsize,), 0xAB, dtype=torch.uint8, device=DEV)
    f = np.zeros(len(parts), dtype=_hip.MONITOR_FOLD_DTYPE)
    first = np.cumsum([0] + [p.shape[0] for p in parts[:-1]])
    f["part"] = part.data_ptr() + P.itemsize * first
    f["total"] = total.data_ptr() + T.itemsize * np.arange(len(parts))
    f["nblocks"] = [p.shape[0] for p in parts]
    (fptr,) = rt.desc.put(f)
    _hip._check(_hip.lib().fedmx_monitor_fold(fptr, len(parts), rt.stream), "fedmx_monitor_fold")
    rt.sync()
    host = total.cpu().numpy()
    assert np.all(host[len(parts) * T.itemsize:] == 0xAB), "bytes beyond the launch's totals were written"
    got = host[:len(parts) * T.itemsize].view(T)
    for nb, g, w in zip(NBLOCKS, got, want):
        for k in T.names:
            assert g[k].tobytes() == w[k].tobytes(), \
                f"nblocks={nb} {k}: columns {np.flatnonzero(g[k] != w[k])[:8].tolist()} differ: {g[k][:8]} vs {w[k][:8]}"


def test_monitor_rows_over_130_blocks():
    dims = ModelDims(5, 3, 2)
    det, train_raw = mon.make_detector(dims, "autoencoder", None, "standard")
    n = 64 * 129 + 5
    x = mon.raw_rows(np.random.default_rng(88), n, dims.d_in)
    x[3, 0], x[64 * 128 + 1, 4], x[n - 1, 2] = np.nan, np.inf, -np.inf
    s = mon.score_rows_numpy(det, x, engine=mon.engine(dims))[0]
    det = dataclasses.replace(det, baseline=mon.baseline_for(det, train_raw, 10), threshold=float(np.sort(s)[(7 * n) // 10]))
    (g,) = mon.engine(dims).monitor_rows([det], [x], block_rows=64)
    mon.check(det, x, g, 64, f"5/3/2 n={n} in 130 blocks")
    assert np.all(g.cnt + g.bad == n) and g.bad[0] >= 1 and g.bad[4] >= 1 and g.bad[2] >= 1
    assert 0 < g.alarms < n and int(g.hist.sum()) == n


# ---------------------------------------------------------------------------
# incidents past 64 spans
EDGE_PATTERNS = ("run from the edge", "run up to the edge", "merged across the edge", "split across the edge",
                 "evidence from the span before", "equal peaks either side of the edge")
LONG_PATTERNS = ("alternating", "random 0.05", "one")


@pytest.mark.parametrize("w,m,h", [(1, 1, 0), (64, 15, 64), (4096, 4096, 4096)])
def test_incidents_past_64_spans(w, m, h):
    S = inc.span_rows()
    E = 64 * S
    names, flags, scores, edges = [], [], [], []
    for i, n in enumerate((64 * S, 64 * S + 1, 65 * S + 3, 129 * S + 7)):
        keep = LONG_PATTERNS if n > 2 * E else EDGE_PATTERNS
        got = [(name, f, s) for name, f, s in inc.patterns(n, E, w, m, h, seed=7 * w + i) if name in keep]
        assert len(got) == len(keep)
        for name, f, s in got:
            names.append(f"w={w} m={m} h={h} n={n} {name}")
            flags.append(f)
            scores.append(s)
            edges.append(E if n > E else n // 2)   # (the edge `patterns` used: a span edge either way)
    got = inc.engine().incidents(flags, scores, w, m, h)
    assert len(got) == len(names) == 3 * len(EDGE_PATTERNS) + len(LONG_PATTERNS)
    seen = 0
    for what, f, s, e, g in zip(names, flags, scores, edges, got):
        inc.same(g, incidents_numpy(f, s, w, m, h), what)
        assert g.count <= incident_bound(g.n, h), what
        seen += g.count
        room = g.n - e > S   # both runs lie inside the rows (they end within 3 * 4096 + 4 rows of the edge)
        if what.endswith(" one"):
            assert (g.start.tolist(), g.end.tolist()) == ([m - 1], [g.n - 1]), what
        if what.endswith("alternating") and (w, m, h) == (1, 1, 0):
            assert g.count == incident_bound(g.n, h), what
        if what.endswith("either side of the edge") and g.n > e + 5:
            assert g.count == 1 and g.peak_row[0] == e - 3 and g.peak_score[0] == 5.0, what
        if "merged across" in what and room:
            assert g.count == 1 and g.start[0] < e <= g.end[0], what
        if "split across" in what and room:
            assert g.count == 2 and g.end[0] < e <= g.start[1], what
        if "evidence from" in what and g.n > e:
            assert g.count == 1 and g.start[0] == e, what
    assert seen > 0
