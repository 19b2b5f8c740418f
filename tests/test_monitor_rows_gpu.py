"""``monitor_rows_kernel`` + ``monitor_fold_kernel`` (fedmx_monitor.hip) and
``HipEngine.monitor_rows`` on the GPU against the oracle
``monitor_rows_numpy`` with the same ``block_rows``; the oracle's forward (and
kNN scores) go through the HIP engine's own ``forward_rows`` / ``knn_scores``,
as tests/test_score_rows_gpu.py does for scores.

Every field must match bit for bit: ``cnt``, ``bad``, ``out``, ``sum``, ``sq``,
``mn``, ``mx``, ``alarms`` and, for autoencoder and CEN detectors, ``hist``; a
kNN detector's ``hist`` is the host binning of the engine's own kNN scores.

Shapes: 115/27/7 (compact forward order), 5/3/2, 1/1/1 and 127/31/15 (identity
order; the lane's second column in and out of range) and 64/16/4 (second
column all padding); row counts bracketing the 16-row tile and the 64-row
pass, and 200 rows in blocks of 64 (four blocks, the last of 8 rows: empty
streams)."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.data.prepare import fitted_scaler_arrays
from fedmse_decentralized_amd.data.scaler import IoTDataProcessor, StandardScaler
from fedmse_decentralized_amd.deploy.detector import (Baseline, Detector, DriftReport, make_baseline,
                                                      monitor_rows_numpy, score_bins, score_rows_numpy)
from fedmse_decentralized_amd.engine.base import pad_features
from fedmse_decentralized_amd.models.layout import ModelDims

DEV = torch.device("cuda", 0)
DIMS = [ModelDims(115, 27, 7), ModelDims(5, 3, 2), ModelDims(1, 1, 1), ModelDims(127, 31, 15), ModelDims(64, 16, 4)]
ROW_COUNTS = [1, 15, 16, 17, 63, 64, 65, 200]
KINDS = [("autoencoder", None), ("hybrid", "cen"), ("hybrid", "knn")]
BINS = [None, 1, 2, 10, 16, None, 10, 16]   # per row count: no baseline, B = 0, 1, 9, 15
N_TRAIN = 120
EXACT = ("cnt", "bad", "out", "sum", "sq", "mn", "mx")
_ENGINES = {}


def engine(dims):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    if dims not in _ENGINES:
        _ENGINES[dims] = HipEngine(dims, DEV)
    return _ENGINES[dims]


def raw_rows(rng, n, D, dtype=np.float64):
    mag = 10.0 ** np.linspace(-2, 6, D)
    x = rng.normal(size=(n, D)) * mag + mag
    x[:, D // 2] = 3.5
    return x.astype(dtype)


def make_detector(dims, model_type, scorer, scaler, seed=0):
    rng = np.random.default_rng(1000 * dims.d_in + seed)
    proc = IoTDataProcessor(scaler)
    train_raw = raw_rows(rng, N_TRAIN, dims.d_in)
    proc.fit_transform(train_raw)
    sc = fitted_scaler_arrays(proc, scaler)
    sc.pop("kind")
    params = (rng.normal(size=dims.num_params) * 0.4 / np.sqrt(dims.hidden)).astype(np.float32)
    det = Detector(dims=dims, model_type="autoencoder", params=params, scaler_kind=scaler, scaler=sc,
                   detect_quantile=0.9)
    if model_type == "autoencoder":
        return det, train_raw
    eng = engine(dims)
    xt = torch.from_numpy(pad_features(det.standardise(train_raw))).to(DEV)
    _, lat = eng.forward_rows(det.padded_params().unsqueeze(0).to(DEV), [(0, xt)], want_sse=False, want_latent=True)
    train_lat = eng.fetch([lat[0]])[0].astype(np.float32)
    zs = StandardScaler().fit(train_lat)
    kw = dict(knn_k=3, train_latents=train_lat) if scorer == "knn" else {}
    return dataclasses.replace(det, model_type="hybrid", latent_scorer=scorer, latent_mean=zs.mean_,
                               latent_scale=zs.scale_, **kw), train_raw


def baseline_for(det, train_raw, bins):
    """bins None: no baseline; 1: a band and no edges (B = 0); else bins - 1 edges."""
    if bins is None:
        return None
    x = det.standardise(train_raw)
    s = np.sort(score_rows_numpy(det, train_raw, engine=engine(det.dims))[0])
    if bins == 1:
        b = make_baseline(x, s, 2)
        return Baseline(b.feat_lo, b.feat_hi, b.score_edges[:0], np.array([s.shape[0]], np.int64))
    return make_baseline(x, s, bins)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {got} vs {want}"


def check(det, rows, got, block_rows, what, scores=None):
    """One report against the oracle's; ``scores``: the kernel's own scores of
    these rows, which then decide the expected histogram and alarm count."""
    want = monitor_rows_numpy(det, rows, block_rows, engine=engine(det.dims))
    assert isinstance(got, DriftReport) and got.n == rows.shape[0] and got.block_rows == block_rows, what
    for k in EXACT:
        same_bits(getattr(got, k), getattr(want, k), f"{what} {k}")
    if scores is not None:
        with np.errstate(invalid="ignore"):
            assert got.alarms == int(np.sum(scores > det.threshold)), what
    else:
        assert got.alarms == want.alarms, (what, got.alarms, want.alarms)
    if det.baseline is None:
        assert got.hist is None and want.hist is None, what
    elif det.latent_scorer == "knn" or scores is not None:
        s = scores if scores is not None else engine(det.dims).score_rows([det], [rows])[0][0]
        same_bits(got.hist, score_bins(s, det.baseline.score_edges), what + " hist (the engine's own scores)")
    else:
        same_bits(got.hist, want.hist, what + " hist")
    for k in ("mean", "var", "out_share", "bad_share"):
        same_bits(getattr(got, k), getattr(want, k), f"{what} {k}")
    return want


@pytest.mark.parametrize("scaler", ["standard", "minmax"])
@pytest.mark.parametrize("model_type,scorer", KINDS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d.d_in}-{d.hidden}-{d.latent}")
def test_every_field_matches_the_oracle(dims, model_type, scorer, scaler):
    """Every row count as one detector of a single call (the same weights;
    different row blocks, input types, baselines and thresholds)."""
    base, train_raw = make_detector(dims, model_type, scorer, scaler)
    D = dims.d_in
    rng = np.random.default_rng(77)
    dets, rows = [], []
    for i, (n, bins) in enumerate(zip(ROW_COUNTS, BINS)):
        x = raw_rows(rng, n, D, np.float32 if i % 2 else np.float64)
        if n >= 17:   # NaN, +inf and -inf in some features; rows of other tiles stay clean
            x[1, 0] = np.nan
            x[3, D - 1] = np.inf
            x[n - 1, D // 3] = -np.inf
        if n == 65:   # a feature without one finite value
            x[:, D - 1] = np.nan
        b = baseline_for(base, train_raw, bins)
        if b is not None and n in (16, 200):   # the band of these very rows: its ends are attained, none is out
            xs = base.standardise(x)
            fin = np.isfinite(xs)
            b = Baseline(np.where(fin, xs, np.float32(np.inf)).min(axis=0),
                         np.where(fin, xs, np.float32(-np.inf)).max(axis=0), b.score_edges, b.score_base)
        s = score_rows_numpy(base, x, engine=engine(dims))[0]
        tau = float("nan") if n == 63 else float(np.sort(s)[(7 * n) // 10])   # (a tie with a score: normal)
        dets.append(dataclasses.replace(base, baseline=b, threshold=tau))
        rows.append(x)
    got = engine(dims).monitor_rows(dets, rows, block_rows=64)
    assert len(got) == len(dets)
    for det, x, g in zip(dets, rows, got):
        n = x.shape[0]
        what = f"{D}/{dims.hidden}/{dims.latent} {model_type}/{scorer} {scaler} {x.dtype} n={n}"
        want = check(det, x, g, 64, what)
        assert np.all(g.cnt + g.bad == n), what
        if n >= 17:
            assert g.bad[0] >= 1 and g.bad[D - 1] >= 1, what
        if n == 65:
            assert g.cnt[D - 1] == 0 and g.bad[D - 1] == 65 and g.mn[D - 1] == np.inf and g.mx[D - 1] == -np.inf \
                and g.sum[D - 1] == 0.0, what
        if n == 63:
            assert g.alarms == 0, what
        elif n > 1 and n != 65 and model_type != "hybrid" and D >= 5:   # (n = 65: every score is NaN, cleaned to 0)
            assert 0 < g.alarms < n, what
        if det.baseline is not None:
            assert g.hist.shape == (det.baseline.score_edges.shape[0] + 1,) and int(g.hist.sum()) == n, what
            if n in (16, 200):
                assert not g.out.any(), what
            elif n >= 64 and D >= 64:
                assert g.out.any(), what   # other rows than the band's: some value leaves it
        assert want.psi == g.psi or (want.psi != want.psi and g.psi != g.psi) or scorer == "knn", what


@pytest.mark.parametrize("model_type,scorer", KINDS)
def test_scores_equal_to_an_edge_fall_in_the_lower_bin(model_type, scorer):
    """Edges taken from the kernel's own scores of a few rows."""
    dims = DIMS[0]
    det, _ = make_detector(dims, model_type, scorer, "standard")
    x = raw_rows(np.random.default_rng(21), 150, dims.d_in)
    eng = engine(dims)
    s = eng.score_rows([det], [x])[0][0]
    picked = np.sort(s[[3, 40, 40, 77, 149]])   # (a repeated edge: an empty bin)
    xs = det.standardise(x)
    det = dataclasses.replace(det, threshold=float(picked[2]), baseline=Baseline(
        xs.min(axis=0), xs.max(axis=0), picked, np.zeros(6, np.int64)))
    g = eng.monitor_rows([det], [x], block_rows=128)[0]
    want_hist = np.array([np.sum(s <= picked[0])] + [np.sum((s > picked[i]) & (s <= picked[i + 1])) for i in range(4)]
                         + [np.sum(s > picked[4])], np.int64)
    same_bits(g.hist, want_hist, "hist against the kernel's scores")
    dup = int(np.flatnonzero(np.diff(picked) == 0)[0])   # the bin between the two equal edges holds nothing
    assert g.hist[0] >= 1 and g.hist[dup + 1] == 0 and int(g.hist.sum()) == 150
    assert g.alarms == int(np.sum(s > picked[2])) and not g.out.any()
    check(det, x, g, 128, f"edge ties {model_type}/{scorer}", scores=s)


def test_three_detectors_in_one_call_and_empty_items(monkeypatch):
    """Different dimensions, kinds, scalers and input types in one call with
    the default block size; the item without rows gets no workgroup, and a call
    with only empty items launches nothing."""
    from fedmse_decentralized_amd.ops import _hip

    rng = np.random.default_rng(5)
    specs = [(DIMS[0], "autoencoder", None, "standard", np.float64, 333, 10),
             (DIMS[1], "hybrid", "knn", "minmax", np.float32, 0, 10),
             (DIMS[3], "hybrid", "cen", "minmax", np.float32, 70, 16),
             (DIMS[1], "hybrid", "knn", "standard", np.float64, 129, 2)]
    dets, rows = [], []
    for dims, mt, sc, scaler, dtype, n, bins in specs:
        d, train_raw = make_detector(dims, mt, sc, scaler, seed=n)
        x = raw_rows(rng, n, dims.d_in, dtype)
        s = score_rows_numpy(d, train_raw, engine=engine(dims))[0]
        dets.append(dataclasses.replace(d, baseline=baseline_for(d, train_raw, bins), threshold=float(np.median(s))))
        rows.append(x)
    launches = []
    real = _hip.lib().fedmx_monitor_rows
    monkeypatch.setattr(_hip.lib(), "fedmx_monitor_rows", lambda d, nb, f, nf, st: launches.append((nb, nf)) or
                        real(d, nb, f, nf, st))
    eng = engine(DIMS[0])
    got = eng.monitor_rows(dets, rows)
    rpb = _hip.score_rows_per_block(333 + 70 + 129)
    assert launches == [(sum(-(-n // rpb) for n in (333, 70, 129)), 3)]
    for i, (d, x, g) in enumerate(zip(dets, rows, got)):
        check(d, x, g, rpb, f"mixed item {i}")
    e = got[1]
    assert e.n == 0 and not e.cnt.any() and not e.sum.any() and np.all(e.mn == np.inf) and np.all(e.mx == -np.inf) \
        and e.alarms == 0 and e.hist.tolist() == [0] * 10
    del launches[:]
    none = eng.monitor_rows([dets[1], dets[0]], [rows[1], rows[0][:0]])
    assert launches == [] and [r.n for r in none] == [0, 0] and none[1].hist.tolist() == [0] * 10
    with pytest.raises(ValueError):
        eng.monitor_rows(dets, rows, block_rows=100)
    with pytest.raises(ValueError):
        eng.monitor_rows(dets[:1], [rows[2]])


def test_score_rows_is_undisturbed():
    dims = DIMS[0]
    det, train_raw = make_detector(dims, "hybrid", "cen", "standard")
    det = dataclasses.replace(det, baseline=baseline_for(det, train_raw, 10), threshold=1.0)
    x = raw_rows(np.random.default_rng(31), 500, dims.d_in)
    eng = engine(dims)
    before = eng.score_rows([det], [x], want_latents=True)[0]
    eng.monitor_rows([det], [x])
    after = eng.score_rows([det], [x], want_latents=True)[0]
    for a, b, k in zip(before, after, ("scores", "flags", "alarms", "latents")):
        if isinstance(a, np.ndarray):
            same_bits(b, a, k)
        else:
            assert a == b, k
