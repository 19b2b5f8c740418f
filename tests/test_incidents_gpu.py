"""The incident kernels (fedmx_incident.hip), ``HipEngine.incidents`` and
``HipEngine.score_incidents`` on the GPU against the oracle ``incidents_numpy``.
Every field is an integer or a copied score, so every field must match bit
for bit.

Grid, with S the rows of one span: n in {0, 1, S-1, S, S+1, 2S+3}; (window,
min_alarms, hold) in {(1,1,0), (2,2,1), (64,15,64), (4096,1,0),
(4096,4096,4096)}; per pair the thirteen patterns of ``patterns``.  All items
of one parameter triple go through a single call (78 items of different
lengths, some without rows)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.data.prepare import fitted_scaler_arrays
from fedmse_decentralized_amd.data.scaler import IoTDataProcessor, StandardScaler
from fedmse_decentralized_amd.deploy.detector import Detector, Incidents, incident_bound, incidents_numpy
from fedmse_decentralized_amd.engine.base import pad_features
from fedmse_decentralized_amd.models.layout import ModelDims

DEV = torch.device("cuda", 0)
DBL_MAX = np.finfo(np.float64).max
PARAMS = [(1, 1, 0), (2, 2, 1), (64, 15, 64), (4096, 1, 0), (4096, 4096, 4096)]
ARRAYS = ("start", "end", "alarms", "peak_row", "peak_score")
SCALARS = ("n", "window", "min_alarms", "hold", "hot_rows", "count", "rows_covered", "longest")
_ENGINES = {}


def engine(dims=ModelDims(115, 27, 7)):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    if dims not in _ENGINES:
        _ENGINES[dims] = HipEngine(dims, DEV)
    return _ENGINES[dims]


def span_rows():
    from fedmse_decentralized_amd.ops import _hip

    return _hip.incident_span_rows()


def same(got, want, what):
    assert isinstance(got, Incidents), what
    for k in SCALARS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))
    for k in ARRAYS:
        g, w = np.ascontiguousarray(getattr(got, k)), np.ascontiguousarray(getattr(want, k))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
            raise AssertionError(f"{what} {k}: {bad.size} of {g.size} differ, first at {bad[:5].tolist()}: "
                                 f"{g[bad[:5]]} vs {w[bad[:5]]}")


def put(a, lo, hi, v=1):
    """a[lo:hi] = v, clipped to the array."""
    lo, hi = max(lo, 0), min(hi, a.shape[0])
    if hi > lo:
        a[lo:hi] = v


@functools.lru_cache(maxsize=None)
def split_gap(w, m, h):
    """The smallest distance between two full-window runs of flags at which
    they are two incidents (one less: they merge), by bisection on the oracle."""
    def count(c):
        f = np.zeros(2 * w + c + w + h + 8, np.uint8)
        f[w:2 * w] = 1
        f[2 * w + c:3 * w + c] = 1
        return incidents_numpy(f, np.zeros(f.shape[0]), w, m, h).count

    lo, hi = 0, w + h + 4        # count(lo) == 1: one joined run; count(hi) == 2
    assert count(hi) == 2
    if count(lo) == 2:
        return 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if count(mid) == 1 else (lo, mid)
    return hi


def patterns(n, S, w, m, h, seed):
    """[(name, flags, scores)] for one row count."""
    rng = np.random.default_rng(seed)

    def plain():
        return np.round(rng.normal(size=n), 1)   # (rounded: equal scores are common)

    z = lambda: np.zeros(n, np.uint8)   # noqa: E731
    edge = S if n > S else n // 2
    out = [("zero", z(), plain()), ("one", np.ones(n, np.uint8), plain()),
           ("alternating", (np.arange(n) % 2 == 0).astype(np.uint8), plain()),
           ("random 0.05", (rng.random(n) < 0.05).astype(np.uint8), plain()),
           ("random 0.5", (rng.random(n) < 0.5).astype(np.int32) * 7, plain())]   # (non-zero counts as 1; another type)
    f = z()
    put(f, edge, edge + w + 3)
    out.append(("run from the edge", f, plain()))
    f = z()
    put(f, edge - w - 3, edge)
    out.append(("run up to the edge", f, plain()))
    c = split_gap(w, m, h)
    for name, gap in (("merged across the edge", c - 1), ("split across the edge", c)):
        f = z()
        a = edge - (w - m) - max(0, gap + 2 * m - w - 1) // 2   # the cold rows between the runs straddle the edge
        put(f, a - w, a)
        put(f, a + gap, a + gap + w)
        out.append((name, f, plain()))
    f = z()
    put(f, edge - (m - 1), edge + 1)          # row `edge` is hot only with the m - 1 flags before it
    out.append(("evidence from the span before", f, plain()))
    s = np.ones(n)
    for r in (edge - 3, edge + 5, n - 1):
        put(s, r, r + 1, 5.0)
    out.append(("equal peaks either side of the edge", np.ones(n, np.uint8), s))
    s = np.full(n, -0.0)
    put(s, edge + 1, edge + 2, 0.0)
    put(s, n // 3, n // 3 + 1, 0.0)
    out.append(("zeros of both signs", np.ones(n, np.uint8), s))
    s = rng.choice(np.array([-DBL_MAX, DBL_MAX, 0.0, 1.5, np.nan, np.inf, -np.inf]), size=n)
    out.append(("+-DBL_MAX and unclean scores", (rng.random(n) < 0.5).astype(np.uint8), s))
    return out


@pytest.mark.parametrize("w,m,h", PARAMS)
def test_every_field_matches_the_oracle(w, m, h):
    S = span_rows()
    assert S >= 8192 + 4098
    names, flags, scores = [], [], []
    for i, n in enumerate((0, 1, S - 1, S, S + 1, 2 * S + 3)):
        for name, f, s in patterns(n, S, w, m, h, seed=100 * w + i):
            names.append(f"w={w} m={m} h={h} n={n} {name}")
            flags.append(f)
            scores.append(s)
    # inputs as numpy, host tensors and device tensors in turn
    fin = [f if i % 3 == 0 else torch.from_numpy(f).to(DEV if i % 3 == 2 else "cpu") for i, f in enumerate(flags)]
    sin = [s if i % 3 == 0 else torch.from_numpy(s).to(DEV if i % 3 == 1 else "cpu") for i, s in enumerate(scores)]
    got = engine().incidents(fin, sin, w, m, h)
    assert len(got) == len(names)
    seen = 0
    for what, f, s, g in zip(names, flags, scores, got):
        want = incidents_numpy(f, s, w, m, h)
        same(g, want, what)
        assert g.count <= incident_bound(g.n, h), what
        seen += g.count
        if what.endswith(" one") and g.n >= m:
            assert (g.start.tolist(), g.end.tolist()) == ([m - 1], [g.n - 1]), what
        if what.endswith("alternating") and (w, m, h) == (1, 1, 0):
            assert g.count == incident_bound(g.n, h), what
        if what.endswith("zeros of both signs") and g.count:
            assert g.peak_row[0] == g.start[0] and np.signbit(g.peak_score[0]) == np.signbit(s[g.start[0]]), what
        if what.endswith("either side of the edge") and g.count and g.n > S + 5 and m - 1 <= S - 3:
            assert g.peak_row[0] == S - 3 and g.peak_score[0] == 5.0, what
        if "merged across" in what and g.n > 2 * S:
            assert g.count == 1 and g.start[0] < S <= g.end[0], what
        if "split across" in what and g.n > 2 * S:
            assert g.count == 2 and g.end[0] < S <= g.start[1], what
        if "evidence from" in what and g.n > S and S >= m:
            assert g.start[0] == S, what
    assert seen > 0


def test_a_call_without_rows_launches_nothing(monkeypatch):
    from fedmse_decentralized_amd.ops import _hip

    calls = []
    real = _hip.lib().fedmx_incidents
    monkeypatch.setattr(_hip.lib(), "fedmx_incidents", lambda *a: calls.append(a[1:6]) or real(*a))
    eng = engine()
    got = eng.incidents([np.zeros(0, np.uint8), torch.zeros(0, dtype=torch.uint8, device=DEV)],
                        [np.zeros(0), np.zeros(0)], 4, 2, 1)
    assert calls == [] and [g.count for g in got] == [0, 0] and got[0].start.dtype == np.int64
    assert eng.incidents([], [], 4, 2, 1) == []
    f = np.array([0, 1, 1, 0, 0, 0, 1, 1], np.uint8)
    got = eng.incidents([f[:0], f], [np.zeros(0), np.arange(8.0)], 2, 2, 1)
    assert calls == [(1, calls[0][1], 1, incident_bound(8, 1), 31)]      # one item with rows, one span
    same(got[1], incidents_numpy(f, np.arange(8.0), 2, 2, 1), "after an empty item")
    assert got[0].n == 0 and got[0].count == 0
    for bad in ((0, 1, 0), (4097, 1, 0), (4, 5, 0), (4, 0, 0), (4, 2, -1), (4, 2, 4097)):
        with pytest.raises(ValueError):
            eng.incidents([f], [np.arange(8.0)], *bad)
    with pytest.raises(ValueError):
        eng.incidents([f], [np.arange(7.0)], 2, 2, 1)
    with pytest.raises(ValueError):
        eng.incidents([f.reshape(2, 4)], [np.arange(8.0).reshape(2, 4)], 2, 2, 1)


# ---------------------------------------------------------------------------
# score_incidents
def raw_rows(rng, n, D):
    mag = 10.0 ** np.linspace(-2, 6, D)
    x = rng.normal(size=(n, D)) * mag + mag
    x[:, D // 2] = 3.5
    return x


def make_detector(dims, model_type, scorer):
    rng = np.random.default_rng(1000 * dims.d_in)
    proc = IoTDataProcessor("standard")
    train_raw = raw_rows(rng, 120, dims.d_in)
    proc.fit_transform(train_raw)
    sc = fitted_scaler_arrays(proc, "standard")
    sc.pop("kind")
    params = (rng.normal(size=dims.num_params) * 0.4 / np.sqrt(dims.hidden)).astype(np.float32)
    det = Detector(dims=dims, model_type="autoencoder", params=params, scaler_kind="standard", scaler=sc,
                   detect_quantile=0.9)
    if model_type == "autoencoder":
        return det
    eng = engine(dims)
    xt = torch.from_numpy(pad_features(det.standardise(train_raw))).to(DEV)
    _, lat = eng.forward_rows(det.padded_params().unsqueeze(0).to(DEV), [(0, xt)], want_sse=False, want_latent=True)
    train_lat = eng.fetch([lat[0]])[0].astype(np.float32)
    zs = StandardScaler().fit(train_lat)
    kw = dict(knn_k=3, train_latents=train_lat) if scorer == "knn" else {}
    return dataclasses.replace(det, model_type="hybrid", latent_scorer=scorer, latent_mean=zs.mean_,
                               latent_scale=zs.scale_, **kw)


def widest_gap_threshold(scores):
    """Midway across the widest gap between adjacent sorted scores in the
    sixth and seventh tenth: no row lies near the threshold."""
    s = np.sort(scores)
    lo, hi = (5 * s.size) // 10, (7 * s.size) // 10
    i = lo + int(np.argmax(np.diff(s[lo:hi + 1])))
    return float(0.5 * (s[i] + s[i + 1]))


@pytest.mark.parametrize("dims", [ModelDims(115, 27, 7), ModelDims(5, 3, 2)], ids=lambda d: f"{d.d_in}-{d.hidden}-{d.latent}")
def test_score_incidents_matches_score_rows_and_the_torch_engine(dims):
    """The three kinds in one call.  Against ``score_rows`` of the same engine
    and the oracle on its scores: every bit.  Against ``TorchEngine`` on the
    CPU, whose fp32 forward rounds differently: the thresholds lie in the
    widest gap of its scores around the 60th percentile, so the flags and with
    them every field the flags decide agree exactly; a peak score differs by no
    more than some row's score does (a maximum is 1-Lipschitz), and the peak
    row's CPU score is within twice that of the CPU peak."""
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine

    w, m, h = 8, 4, 3
    cpu = TorchEngine(dims, torch.device("cpu"))
    eng = engine(dims)
    rng = np.random.default_rng(9)
    dets, rows = [], []
    for i, (mt, sc) in enumerate((("autoencoder", None), ("hybrid", "cen"), ("hybrid", "knn"))):
        det = make_detector(dims, mt, sc)
        x = raw_rows(rng, 300 + 17 * i, dims.d_in)
        det = dataclasses.replace(det, threshold=widest_gap_threshold(cpu.score_rows([det], [x])[0][0]))
        dets.append(det)
        rows.append(x)
    dets.append(dets[0])
    rows.append(rows[0][:0])                     # an item without rows
    got = eng.score_incidents(dets, rows, w, m, h)
    plain = eng.score_rows(dets, rows)
    ref = cpu.score_incidents(dets, rows, w, m, h)
    assert len(got) == 4 and got[3][3].count == 0 and got[3][0].shape == (0,)
    for i, (g, p, r) in enumerate(zip(got, plain, ref)):
        what = f"{dims.d_in} item {i}"
        assert g[0].dtype == p[0].dtype and g[0].tobytes() == p[0].tobytes(), what
        assert g[1].dtype == p[1].dtype and g[1].tobytes() == p[1].tobytes() and g[2] == p[2], what
        same(g[3], incidents_numpy(p[1], p[0], w, m, h), what + " against the oracle on score_rows' results")
        np.testing.assert_array_equal(g[1], r[1], err_msg=what + " flags against TorchEngine")
        assert g[2] == r[2], what
        for k in SCALARS + ("start", "end", "alarms"):
            np.testing.assert_array_equal(getattr(g[3], k), getattr(r[3], k), err_msg=f"{what} {k}")
        if i < 3:
            assert g[3].count >= 1, what
            d = float(np.max(np.abs(g[0] - r[0])))
            assert np.all(np.abs(g[3].peak_score - r[3].peak_score) <= d), what
            assert np.all(r[0][g[3].peak_row] >= r[3].peak_score - 2 * d), what
