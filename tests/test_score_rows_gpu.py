"""``score_rows_kernel`` (fedmx_score.hip) and ``HipEngine.score_rows`` on the
GPU against an oracle that never runs the kernel: ``Detector.standardise``
(numpy, bit-equal to ``IoTDataProcessor``) gives the fp32 rows,
``HipEngine.forward_rows`` (``fwd_rows_kernel``) their SSE and latents, the
numpy CEN loop / ``knn_score_numpy`` the latent scores.

Autoencoder scores and emitted latents must equal the oracle's bit for bit;
CEN and kNN scores lie within the relative 1e-12 that
tests/test_knn_scorer_gpu.py holds ``cen_score_kernel``'s arithmetic and
``knn_score_kernel`` to (the kernels take their float64 square root and, for
kNN, refit the latent scaler on the device).  Thresholds are taken midway
between two adjacent distinct oracle scores, so no row sits within that
tolerance of the threshold; flags must equal ``returned score > threshold``
and the alarm counter their sum.

Shapes: the 16-row tile and the 64-row workgroup pass (four waves, one tile
each) bracketed from both sides, about 1,000 rows over several workgroups with
a ragged tail, and blocks of three passes; 115/27/7 (compact forward order),
120/30/10 (identity order) and 5/3/2."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.data.prepare import fitted_scaler_arrays
from fedmse_decentralized_amd.data.scaler import IoTDataProcessor, StandardScaler
from fedmse_decentralized_amd.deploy.detector import Detector, _ae_scores, cen_scores_stored
from fedmse_decentralized_amd.engine.base import pad_features
from fedmse_decentralized_amd.engine.torch_engine import knn_score_numpy
from fedmse_decentralized_amd.models.layout import ModelDims

DEV = torch.device("cuda", 0)
TOL = 1e-12            # CEN / kNN scores, relative (tests/test_knn_scorer.py GPU_TOL)
GAP = 1e-6             # relative gap between the two scores a threshold is put between
DIMS = [ModelDims(115, 27, 7), ModelDims(120, 30, 10), ModelDims(5, 3, 2)]
ROW_COUNTS = [1, 15, 16, 17, 63, 64, 65, 1000]   # tile 16, workgroup pass 64
KINDS = [("autoencoder", None, 0), ("hybrid", "cen", 0), ("hybrid", "knn", 1), ("hybrid", "knn", 5)]
N_TRAIN = 300
_ENGINES = {}
_WORST = {}


def engine(dims):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    if dims not in _ENGINES:
        _ENGINES[dims] = HipEngine(dims, DEV)
    return _ENGINES[dims]


def raw_rows(rng, n, D, dtype=np.float64):
    """Raw traffic-like rows: columns of very different magnitudes, one constant."""
    mag = 10.0 ** np.linspace(-2, 6, D)
    x = rng.normal(size=(n, D)) * mag + mag
    x[:, D // 2] = 3.5
    return x.astype(dtype)


def forward_oracle(det, std_rows, want_sse, want_lat):
    """fwd_rows_kernel on already standardised fp32 rows -> (sse, latents) as numpy."""
    eng = engine(det.dims)
    params = det.padded_params().unsqueeze(0).to(DEV)
    xt = torch.from_numpy(pad_features(std_rows)).to(DEV)
    sse, lat = eng.forward_rows(params, [(0, xt)], want_sse=want_sse, want_latent=want_lat)
    eng.synchronize()
    return (sse[0].cpu().numpy() if want_sse else None), (lat[0].cpu().numpy() if want_lat else None)


def make_detector(dims, model_type, scorer, k, scaler, seed=0):
    rng = np.random.default_rng(1000 * dims.d_in + seed)
    D = dims.d_in
    proc = IoTDataProcessor(scaler)
    train_raw = raw_rows(rng, N_TRAIN, D)
    proc.fit_transform(train_raw)
    sc = fitted_scaler_arrays(proc, scaler)
    sc.pop("kind")
    params = (rng.normal(size=dims.num_params) * 0.4 / np.sqrt(dims.hidden)).astype(np.float32)
    det = Detector(dims=dims, model_type="autoencoder", params=params, scaler_kind=scaler, scaler=sc)
    if model_type == "autoencoder":
        return det
    _, train_lat = forward_oracle(det, det.standardise(train_raw), False, True)
    zs = StandardScaler().fit(train_lat)
    kw = dict(knn_k=k, train_latents=train_lat) if scorer == "knn" else {}
    return dataclasses.replace(det, model_type="hybrid", latent_scorer=scorer, latent_mean=zs.mean_,
                               latent_scale=zs.scale_, **kw)


def oracle(det, raw):
    """(cleaned float64 scores, fp32 latents or None) without score_rows_kernel."""
    hybrid = det.model_type == "hybrid"
    sse, lat = forward_oracle(det, det.standardise(raw), not hybrid, hybrid)
    if not hybrid:
        s = _ae_scores(sse, det.dims.d_in)
    elif det.latent_scorer == "cen":
        s = cen_scores_stored(lat, det.latent_mean, det.latent_scale)
    else:
        s = knn_score_numpy(det.train_latents, lat, det.knn_k)
    return np.nan_to_num(s), lat


def threshold_between(scores, q):
    """Midway between two adjacent distinct sorted scores near quantile q,
    at least GAP (relative) apart; NaN when there is no such pair."""
    s = np.unique(scores[np.isfinite(scores)])
    if s.size < 2:
        return float("nan")
    order = np.argsort(np.abs(np.arange(s.size - 1) - q * (s.size - 1)))
    for i in order:
        if s[i + 1] - s[i] > GAP * max(abs(s[i]), abs(s[i + 1]), 1e-300):
            return float(0.5 * (s[i] + s[i + 1]))
    return float("nan")


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind != "f":
        np.testing.assert_array_equal(got, want, err_msg=what)
        return
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero((got.view(u) != want.view(u)).reshape(-1) & ~(np.isnan(got) & np.isnan(want)).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first {bad[:6].tolist()}: " \
                          f"{got.reshape(-1)[bad[:6]]} vs {want.reshape(-1)[bad[:6]]}"


def check(det, got, want_scores, want_lat, what):
    """One detector's result against its oracle; returns the relative score error."""
    s, f, a = got[:3]
    n = want_scores.shape[0]
    assert s.shape == (n,) and s.dtype == np.float64 and f.shape == (n,) and f.dtype == np.uint8, what
    err = 0.0
    if det.model_type == "autoencoder":
        same_bits(s, want_scores, what + " AE scores")
    else:
        if n:
            err = float(np.max(np.abs(s - want_scores) / np.maximum(np.abs(want_scores), 1e-300)))
        np.testing.assert_allclose(s, want_scores, rtol=TOL, atol=0.0, err_msg=what)
    if len(got) > 3 and want_lat is not None:
        same_bits(got[3], want_lat, what + " latents")
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(f, (s > det.threshold).astype(np.uint8), err_msg=what + " flags")
        if np.isfinite(det.threshold):   # no row within the tolerance of the threshold: the oracle's flags too
            np.testing.assert_array_equal(f, (want_scores > det.threshold).astype(np.uint8), err_msg=what)
    assert a == int(f.sum()), (what, a, int(f.sum()))
    key = (det.model_type, det.latent_scorer)
    _WORST[key] = max(_WORST.get(key, 0.0), err)
    return err


@pytest.mark.parametrize("scaler,dtype", [("standard", np.float64), ("standard", np.float32),
                                          ("minmax", np.float64), ("minmax", np.float32)])
@pytest.mark.parametrize("model_type,scorer,k", KINDS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d.d_in}-{d.hidden}-{d.latent}")
def test_scores_flags_and_alarms(dims, model_type, scorer, k, scaler, dtype):
    """Every row count as one detector of a single launch (the same weights,
    different row blocks and thresholds)."""
    base = make_detector(dims, model_type, scorer, k, scaler)
    rng = np.random.default_rng(77)
    rows = [raw_rows(rng, n, dims.d_in, dtype) for n in ROW_COUNTS] + [np.zeros((0, dims.d_in), dtype)]
    want = [oracle(base, x) if x.shape[0] else (np.zeros(0), np.zeros((0, dims.latent), np.float32)) for x in rows]
    dets = []
    for i, (ws, _) in enumerate(want):
        # thresholds at different quantiles; one NaN; one equal to a score
        if i == 2:
            tau = float("nan")
        elif i == 4:
            tau = float(np.sort(ws)[ws.size // 2])
        else:
            tau = threshold_between(ws, (0.1, 0.5, 0.9)[i % 3]) if ws.size > 1 else (float(ws[0]) * 0.5 if ws.size else 1.0)
        dets.append(dataclasses.replace(base, threshold=tau))
    got = engine(dims).score_rows(dets, rows, want_latents=True)
    worst = 0.0
    for i, (d, g, (ws, wl)) in enumerate(zip(dets, got, want)):
        what = f"{dims} {model_type}/{scorer}/{k} {scaler} {np.dtype(dtype).name} n={rows[i].shape[0]}"
        if i == 4 and model_type != "autoencoder":
            # (a threshold equal to an oracle score may sit 1e-12 off the kernel's: re-tune it to the returned one)
            d.threshold = float(np.sort(g[0])[g[0].size // 2])
            g = engine(dims).score_rows([d], [rows[i]], want_latents=True)[0]
            f = g[1]
            np.testing.assert_array_equal(f, (g[0] > d.threshold).astype(np.uint8), err_msg=what + " tie")
            assert g[2] == int(f.sum()) and f[np.argsort(g[0])[g[0].size // 2]] == 0
            worst = max(worst, float(np.max(np.abs(g[0] - ws) / np.maximum(np.abs(ws), 1e-300))))
            np.testing.assert_allclose(g[0], ws, rtol=TOL, atol=0.0, err_msg=what)
            same_bits(g[3], wl, what + " latents")
            continue
        worst = max(worst, check(d, g, ws, wl if model_type == "hybrid" else None, what))
        if i == 4:   # autoencoder: the tie row itself is normal
            assert g[1][np.argsort(ws)[ws.size // 2]] == 0 and 0 < g[2] < ws.size
        if i == 2:
            assert g[2] == 0 and not g[1].any()
        if model_type == "autoencoder":
            assert g[3] is None
    assert got[-1][0].shape == (0,) and got[-1][1].shape == (0,) and got[-1][2] == 0
    assert any(g[2] > 0 for g in got)
    print(f"score_rows {dims.d_in}/{dims.hidden}/{dims.latent} {model_type}/{scorer}/k={k} {scaler} "
          f"{np.dtype(dtype).name}: max relative score error {worst:.3e}")


def test_mixed_detectors_in_one_call():
    """Detectors of different dimensions, types, scalers, input types and row counts in one call."""
    rng = np.random.default_rng(5)
    specs = [(DIMS[0], "autoencoder", None, 0, "standard", np.float64, 333),
             (DIMS[1], "hybrid", "cen", 0, "minmax", np.float32, 70),
             (DIMS[2], "hybrid", "knn", 5, "standard", np.float64, 129),
             (DIMS[0], "hybrid", "knn", 1, "minmax", np.float32, 17),
             (DIMS[0], "hybrid", "cen", 0, "standard", np.float64, 1),
             (DIMS[2], "autoencoder", None, 0, "minmax", np.float32, 64)]
    dets, rows, want = [], [], []
    for dims, mt, sc, k, scaler, dtype, n in specs:
        d = make_detector(dims, mt, sc, k, scaler, seed=n)
        x = raw_rows(rng, n, dims.d_in, dtype)
        ws, wl = oracle(d, x)
        d.threshold = threshold_between(ws, 0.7) if n > 1 else float(ws[0]) * 0.5
        dets.append(d), rows.append(x), want.append((ws, wl))
    got = engine(DIMS[0]).score_rows(dets, rows, want_latents=True)
    for i, (d, g, (ws, wl)) in enumerate(zip(dets, got, want)):
        check(d, g, ws, wl if d.model_type == "hybrid" else None, f"mixed item {i}")
    plain = engine(DIMS[0]).score_rows(dets, rows)
    for g, p in zip(got, plain):
        assert len(p) == 3 and p[2] == g[2]
        same_bits(p[0], g[0], "want_latents changes no score")
        same_bits(p[1], g[1], "want_latents changes no flag")


@pytest.mark.parametrize("model_type,scorer", [("autoencoder", None), ("hybrid", "cen")])
def test_blocks_of_several_passes(model_type, scorer):
    """1,000 rows in workgroup blocks of 192 rows (three passes each, a ragged
    last block of 40), into sentinel-padded outputs: nothing outside is written."""
    from fedmse_decentralized_amd.ops import _hip

    dims = DIMS[0]
    det = make_detector(dims, model_type, scorer, 0, "standard")
    x = raw_rows(np.random.default_rng(9), 1000, dims.d_in)
    ws, wl = oracle(det, x)
    det.threshold = threshold_between(ws, 0.8)
    eng = engine(dims)
    state, _ = eng._score_state(det)
    n, pad = 1000, 7
    scores = torch.full((n + pad,), -7.0, dtype=torch.float64, device=DEV)
    flags = torch.full((n + pad,), 9, dtype=torch.uint8, device=DEV)
    lat = torch.full((n + pad, dims.latent), -7.0, dtype=torch.float32, device=DEV)
    alarms = torch.zeros(3, dtype=torch.int32, device=DEV)
    keep = torch.from_numpy(x).to(DEV)
    desc = _hip.score_desc([state], [keep], [scores[:n]], [flags[:n]], [lat[:n]], alarms[1:2], rows_per_block=192)
    assert len(desc) == 6 and desc["nrows"].tolist() == [192] * 5 + [40]
    rt = _hip.runtime(DEV)
    (dptr,) = rt.desc.put(desc)
    _hip._check(_hip.lib().fedmx_score_rows(dptr, len(desc), rt.stream), "fedmx_score_rows")
    rt.sync()
    s, f, la, al = scores.cpu().numpy(), flags.cpu().numpy(), lat.cpu().numpy(), alarms.cpu().numpy()
    assert np.all(s[n:] == -7.0) and np.all(f[n:] == 9) and np.all(la[n:] == -7.0) and al[0] == 0 and al[2] == 0
    check(det, (s[:n], f[:n], int(al[1]), la[:n]), ws, wl, f"blocks of 192 {model_type}")
    assert 0 < al[1] < n
    with pytest.raises(ValueError):
        _hip.score_desc([state], [keep], [scores[:n]], [flags[:n]], [lat[:n]], alarms, rows_per_block=100)
    with pytest.raises(ValueError):
        _hip.score_desc([state], [keep[:, :50].contiguous()], [scores[:n]], [flags[:n]], [lat[:n]], alarms)


@pytest.mark.parametrize("model_type,scorer,k", KINDS[:3])
def test_non_finite_rows(model_type, scorer, k):
    """A row holding NaN and rows holding +inf / -inf in one raw feature score
    by the cleaning rule and leave the other rows of their 16-row tiles alone."""
    dims = DIMS[0]
    det = make_detector(dims, model_type, scorer, k, "standard")
    x = raw_rows(np.random.default_rng(13), 100, dims.d_in)
    ws, _ = oracle(det, x)
    det.threshold = threshold_between(ws, 0.5)
    eng = engine(dims)
    clean = eng.score_rows([det], [x], want_latents=True)[0]
    bad = x.copy()
    bad[5, 17] = np.nan
    bad[40, 0] = np.inf
    bad[77, 114] = -np.inf
    rows = [5, 40, 77]
    got = eng.score_rows([det], [bad], want_latents=True)[0]
    wb, wl = oracle(det, bad)
    check(det, got, wb, wl if model_type == "hybrid" else None, f"non-finite {model_type}/{scorer}")
    assert np.all(np.isfinite(got[0]))
    dbl_max = np.finfo(np.float64).max
    if model_type == "autoencoder":
        # the row's own error term is non-finite whatever the model makes of it: NaN -> 0, +inf -> DBL_MAX
        assert got[0][5] == 0.0 and all(got[0][r] in (0.0, dbl_max) for r in rows), got[0][rows]
    assert [int(got[1][r]) for r in rows] == [int(got[0][r] > det.threshold) for r in rows]
    others = np.setdiff1d(np.arange(100), rows)
    same_bits(got[0][others], clean[0][others], "rows beside the non-finite ones")
    same_bits(got[1][others], clean[1][others], "flags beside the non-finite ones")
    if model_type == "hybrid":
        same_bits(got[3][others], clean[3][others], "latents beside the non-finite ones")
