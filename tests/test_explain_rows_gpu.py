"""``explain_rows_kernel`` (fedmx_explain.hip) and ``HipEngine.explain_rows``
on the GPU.

a. ``sse`` has the bits ``HipEngine.forward_rows`` (``fwd_rows_kernel``)
   returns on ``Detector.standardise(rows)[which]``; for an autoencoder
   ``_ae_scores(sse)`` has the bits of ``score_rows``' scores at the rows that
   call flagged.
b. The dense residuals lie within a derived bound of a float64 forward over
   the same fp32 parameters and fp32 standardised rows.  With ``u = 2^-24`` and
   ``gamma(n) = n u / (1 - n u)``, a layer of fan-in ``K`` (bias: one more
   term) turns the error bound ``E`` of its input ``a`` into
   ``gamma(K + 1) ((|a| + E) |W|^T + |b|) + E |W|^T`` (any summation order;
   ReLU keeps it), and the subtraction adds ``u (|y| + |x| + E4)``.  The limit
   is twice that: the factor covers the second-order terms dropped.
c. ``idx`` equals the numpy selection rule applied to the kernel's own dense
   output, ``resid`` has the bits of ``resid_full[row, idx]``, unused slots
   hold -1 and 0; one block holds a raw row with a NaN column and one with
   1e300 (NaN first, then the infinite squares, ties by rising feature).
d. CEN ``latent_terms`` have the bits of the numpy terms formed from
   ``forward_rows``' latents and the stored scaler; the root of their sum lies
   within relative 1e-12 of ``score_rows``' score (the device square root's
   tolerance in tests/test_score_rows_gpu.py).
e. ``score_rows`` returns the same bits before and after an ``explain_rows``.

Shapes: 115/27/7 (compact forward order), 120/30/10 (identity), 5/3/2 and
1/1/1; row counts around the 16-row tile and the 64-row pass and 200 rows (four
workgroups, a ragged last one); K in {1, 3, 8, 16}; float64 and float32 input;
both scalers; ``which`` None, a permuted subset with repeats, and empty."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.data.prepare import fitted_scaler_arrays
from fedmse_decentralized_amd.data.scaler import IoTDataProcessor, StandardScaler
from fedmse_decentralized_amd.deploy.detector import Detector, _ae_scores, cen_terms_stored, select_top_k
from fedmse_decentralized_amd.engine.base import pad_features
from fedmse_decentralized_amd.models.layout import ModelDims
from fedmse_decentralized_amd.models.reference import unflatten

DEV = torch.device("cuda", 0)
TOL = 1e-12
DIMS = [ModelDims(115, 27, 7), ModelDims(120, 30, 10), ModelDims(5, 3, 2), ModelDims(1, 1, 1)]
ROW_COUNTS = [1, 15, 16, 17, 63, 64, 65, 200]
TOP_KS = [1, 3, 8, 16]
COMBOS = [("standard", np.float64), ("standard", np.float32), ("minmax", np.float64), ("minmax", np.float32)]
N_TRAIN = 300
U = 2.0 ** -24
_ENGINES, _DETS = {}, {}
ids = dict(ids=lambda d: f"{d.d_in}-{d.hidden}-{d.latent}")


def engine(dims):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    if dims not in _ENGINES:
        _ENGINES[dims] = HipEngine(dims, DEV)
    return _ENGINES[dims]


def raw_rows(rng, n, D, dtype=np.float64):
    """Raw traffic-like rows: columns of very different magnitudes, one constant (when there are several)."""
    mag = 10.0 ** np.linspace(-2, 6, D)
    x = rng.normal(size=(n, D)) * mag + mag
    if D > 2:
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


def detector(dims, model_type="autoencoder", scorer=None, scaler="standard"):
    """Built once per kind and left unchanged."""
    key = (dims, model_type, scorer, scaler)
    if key in _DETS:
        return _DETS[key]
    rng = np.random.default_rng(1000 * dims.d_in + 7)
    proc = IoTDataProcessor(scaler)
    train_raw = raw_rows(rng, N_TRAIN, dims.d_in)
    proc.fit_transform(train_raw)
    sc = fitted_scaler_arrays(proc, scaler)
    sc.pop("kind")
    params = (rng.normal(size=dims.num_params) * 0.4 / np.sqrt(dims.hidden)).astype(np.float32)
    det = Detector(dims=dims, model_type="autoencoder", params=params, scaler_kind=scaler, scaler=sc)
    if model_type == "hybrid":
        _, train_lat = forward_oracle(det, det.standardise(train_raw), False, True)
        zs = StandardScaler().fit(train_lat)
        kw = dict(knn_k=3, train_latents=train_lat) if scorer == "knn" else {}
        det = dataclasses.replace(det, model_type="hybrid", latent_scorer=scorer, latent_mean=zs.mean_,
                                  latent_scale=zs.scale_, **kw)
    _DETS[key] = det
    return det


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


def f64_forward_with_bound(det, x32):
    """(y - x in float64, the limit per element) over the fp32 parameters and fp32 rows."""
    w1, b1, w2, b2, w3, b3, w4, b4 = (t.numpy().astype(np.float64)
                                      for t in unflatten(torch.from_numpy(det.params), det.dims))
    x = x32.astype(np.float64)

    def gamma(n):
        return n * U / (1.0 - n * U)

    a, E = x, np.zeros_like(x)
    for W, b, relu in ((w1, b1, True), (w2, b2, False), (w3, b3, True), (w4, b4, False)):
        aW = np.abs(W).T
        E = gamma(W.shape[1] + 1) * ((np.abs(a) + E) @ aW + np.abs(b)) + E @ aW
        a = a @ W.T + b
        if relu:
            a = np.maximum(a, 0.0)
    limit = 2.0 * (E + U * (np.abs(a) + np.abs(x) + E))
    return a - x, limit


def check_selection(ex, k, D, what):
    """c: idx / resid against the rule on the kernel's own dense output."""
    idx, top = select_top_k(ex.resid_full, k)
    np.testing.assert_array_equal(ex.idx, idx, err_msg=what + " idx")
    same_bits(ex.resid, top, what + " resid")
    kk = min(k, D)
    assert np.all(ex.idx[:, kk:] == -1) and np.all(ex.resid[:, kk:] == 0.0), what
    assert np.all((ex.idx[:, :kk] >= 0) & (ex.idx[:, :kk] < D)), what


@pytest.mark.parametrize("scaler,dtype", COMBOS, ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
@pytest.mark.parametrize("dims", DIMS, **ids)
def test_sse_dense_residuals_and_top_k(dims, scaler, dtype):
    """Every row count as one item of a single launch (the same weights), plus a
    permuted subset with repeats, an empty subset and a block with bad rows;
    one launch per K."""
    D = dims.d_in
    det = detector(dims, "autoencoder", None, scaler)
    rng = np.random.default_rng(77)
    rows = [raw_rows(rng, n, D, dtype) for n in ROW_COUNTS]
    which = [None] * len(rows)
    rows.append(rows[-1]), which.append(rng.permutation(np.r_[np.arange(0, 200, 3), [199, 0, 5, 5, 5]]))   # 72 rows
    rows.append(rows[-2]), which.append(np.zeros(0, np.int64))
    bad = raw_rows(rng, 40, D, dtype)
    bad[5, D // 3] = np.nan
    bad[22, D - 1] = 1e300 if dtype == np.float64 else np.inf
    rows.append(bad), which.append(None)
    picks = [np.arange(x.shape[0]) if w is None else w for x, w in zip(rows, which)]
    std = [det.standardise(x)[p] for x, p in zip(rows, picks)]
    want_sse = [forward_oracle(det, s, True, False)[0] if s.shape[0] else np.zeros(0, np.float32) for s in std]
    eng = engine(dims)
    first, worst = None, 0.0
    for k in TOP_KS:
        got = eng.explain_rows([det] * len(rows), rows, top_k=k, which=which, dense=True)
        for i, (ex, p) in enumerate(zip(got, picks)):
            what = f"{D}/{dims.hidden}/{dims.latent} {scaler} {np.dtype(dtype).name} K={k} item {i} m={p.shape[0]}"
            np.testing.assert_array_equal(ex.rows, p, err_msg=what)
            assert ex.rows.dtype == np.int64 and ex.idx.dtype == np.int32 and ex.idx.shape == (p.shape[0], k), what
            assert ex.resid_full.shape == (p.shape[0], D) and ex.latent_terms is None, what
            same_bits(ex.sse, want_sse[i], what + " sse (a)")
            check_selection(ex, k, D, what)
        if first is None:
            first = got
            for i, ex in enumerate(got[:-1]):   # b: the finite blocks
                if ex.rows.shape[0] == 0:
                    continue
                ref, limit = f64_forward_with_bound(det, std[i])
                err = np.abs(ex.resid_full.astype(np.float64) - ref)
                worst = max(worst, float((err / np.maximum(limit, 1e-300)).max()))
                assert np.all(err <= limit), (i, worst)
        else:
            for a, b in zip(first, got):
                same_bits(b.resid_full, a.resid_full, f"dense residuals do not depend on K ({k})")
    print(f"explain_rows {D}/{dims.hidden}/{dims.latent} {scaler} {np.dtype(dtype).name}: "
          f"worst dense error / limit {worst:.3f}")
    # the bad block: NaN first, the infinite square next, ties by rising feature
    ex = first[-1]
    with np.errstate(all="ignore"):
        for r in (5, 22):
            e = ex.resid_full[r] * ex.resid_full[r]
            assert not np.isfinite(e).all() and ex.idx[r, 0] == int(np.flatnonzero(~np.isfinite(e))[0]), (r, ex.idx[r])
    assert np.isnan(ex.resid_full[5]).any()


@pytest.mark.parametrize("dims", DIMS, **ids)
def test_autoencoder_scores_of_flagged_rows_and_no_side_effect(dims):
    """a (second half) and e: explain the rows a real score_rows call flagged."""
    det = dataclasses.replace(detector(dims, "autoencoder", None, "standard"))
    rows = raw_rows(np.random.default_rng(21), 200, dims.d_in)
    eng = engine(dims)
    s0 = eng.score_rows([det], [rows])[0][0]
    det.threshold = float(np.median(s0))
    before = eng.score_rows([det], [rows], want_latents=True)[0]
    flagged = np.flatnonzero(before[1])
    assert 0 < flagged.size < 200
    ex = eng.explain_rows([det], [rows], top_k=5, which=[flagged])[0]
    same_bits(np.nan_to_num(_ae_scores(ex.sse, dims.d_in)), before[0][flagged], "AE score from sse")
    assert ex.resid_full is None and ex.latent_terms is None
    after = eng.score_rows([det], [rows], want_latents=True)[0]
    same_bits(after[0], before[0], "scores after explain_rows")
    same_bits(after[1], before[1], "flags after explain_rows")
    assert after[2] == before[2]


@pytest.mark.parametrize("scaler,dtype", COMBOS[::3], ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
@pytest.mark.parametrize("dims", DIMS, **ids)
def test_cen_latent_terms(dims, scaler, dtype):
    """d: the exact decomposition of a CEN score, and the feature-space residuals beside it."""
    det = detector(dims, "hybrid", "cen", scaler)
    rng = np.random.default_rng(31)
    rows = raw_rows(rng, 200, dims.d_in, dtype)
    which = rng.permutation(200)[:77]
    eng = engine(dims)
    scores = eng.score_rows([det], [rows])[0][0]
    worst = 0.0
    for w in (None, which):
        p = np.arange(200) if w is None else w
        ex = eng.explain_rows([det], [rows], top_k=3, which=[w], dense=True)[0]
        sse, lat = forward_oracle(det, det.standardise(rows)[p], True, True)
        same_bits(ex.latent_terms, cen_terms_stored(lat, det.latent_mean, det.latent_scale), "latent terms")
        same_bits(ex.sse, sse, "sse of a hybrid detector")
        check_selection(ex, 3, dims.d_in, "hybrid")
        acc = np.zeros(p.shape[0])
        for j in range(dims.latent):
            acc += ex.latent_terms[:, j]
        root = np.nan_to_num(np.sqrt(acc))
        np.testing.assert_allclose(root, scores[p], rtol=TOL, atol=0.0)
        worst = max(worst, float(np.max(np.abs(root - scores[p]) / np.maximum(np.abs(scores[p]), 1e-300))))
    print(f"explain_rows CEN {dims.d_in}/{dims.hidden}/{dims.latent} {scaler}: sqrt(sum terms) vs score {worst:.3e}")


def test_mixed_detectors_in_one_call():
    """Detectors of different dimensions, kinds, scalers, input types, row choices in one launch."""
    rng = np.random.default_rng(5)
    specs = [(DIMS[0], "autoencoder", None, "standard", np.float64, 133, False),
             (DIMS[1], "hybrid", "cen", "minmax", np.float32, 70, True),
             (DIMS[2], "hybrid", "knn", "standard", np.float64, 129, True),
             (DIMS[3], "autoencoder", None, "minmax", np.float32, 17, False),
             (DIMS[0], "hybrid", "cen", "standard", np.float64, 1, False),
             (DIMS[0], "hybrid", "knn", "minmax", np.float32, 64, True)]
    dets, rows, which = [], [], []
    for dims, mt, sc, scaler, dtype, n, sub in specs:
        dets.append(detector(dims, mt, sc, scaler))
        rows.append(raw_rows(rng, n, dims.d_in, dtype))
        which.append(rng.integers(0, n, size=n // 2 + 1) if sub else None)
    got = engine(DIMS[0]).explain_rows(dets, rows, top_k=8, which=which, dense=True)
    for i, (det, x, w, ex) in enumerate(zip(dets, rows, which, got)):
        p = np.arange(x.shape[0]) if w is None else w
        cen = det.latent_scorer == "cen"
        sse, lat = forward_oracle(det, det.standardise(x)[p], True, cen)
        same_bits(ex.sse, sse, f"mixed item {i} sse")
        check_selection(ex, 8, det.dims.d_in, f"mixed item {i}")
        ref, limit = f64_forward_with_bound(det, det.standardise(x)[p])
        assert np.all(np.abs(ex.resid_full.astype(np.float64) - ref) <= limit), i
        if cen:
            same_bits(ex.latent_terms, cen_terms_stored(lat, det.latent_mean, det.latent_scale), f"mixed item {i}")
        else:
            assert ex.latent_terms is None
    alone = engine(DIMS[0]).explain_rows(dets[1:2], rows[1:2], top_k=8, which=which[1:2])[0]
    assert alone.resid_full is None
    same_bits(alone.idx, got[1].idx, "dense changes no index")
    same_bits(alone.resid, got[1].resid, "dense changes no residual")


def test_blocks_of_several_passes_write_nothing_outside():
    """300 chosen rows in workgroup blocks of 128 (two passes each, a ragged
    last block of 44) into sentinel-padded outputs; bad arguments raise."""
    from fedmse_decentralized_amd.ops import _hip

    dims = DIMS[0]
    det = detector(dims, "hybrid", "cen", "standard")
    rng = np.random.default_rng(9)
    x = raw_rows(rng, 500, dims.d_in)
    w = rng.integers(0, 500, size=300)
    eng = engine(dims)
    state, _ = eng._score_state(det)
    m, pad, k = 300, 5, 3
    keep = torch.from_numpy(x).to(DEV)
    wd = torch.from_numpy(w.astype(np.int32)).to(DEV)
    full = {"idx": torch.full((m + pad, k), -9, dtype=torch.int32, device=DEV),
            "resid": torch.full((m + pad, k), -7.0, dtype=torch.float32, device=DEV),
            "sse": torch.full((m + pad,), -7.0, dtype=torch.float32, device=DEV),
            "resid_full": torch.full((m + pad, dims.d_in), -7.0, dtype=torch.float32, device=DEV),
            "latent_terms": torch.full((m + pad, dims.latent), -7.0, dtype=torch.float64, device=DEV)}
    outs = {n: t[:m] for n, t in full.items()}
    desc = _hip.explain_desc([state], [keep], [wd], [outs], k, rows_per_block=128)
    assert len(desc) == 3 and desc["nrows"].tolist() == [128, 128, 44]
    rt = _hip.runtime(DEV)
    (dptr,) = rt.desc.put(desc)
    _hip._check(_hip.lib().fedmx_explain_rows(dptr, len(desc), rt.stream), "fedmx_explain_rows")
    rt.sync()
    host = {n: t.cpu().numpy() for n, t in full.items()}
    assert np.all(host["idx"][m:] == -9) and all(np.all(host[n][m:] == -7.0) for n in host if n != "idx")
    want = eng.explain_rows([det], [x], top_k=k, which=[w], dense=True)[0]
    for n in host:
        same_bits(host[n][:m], getattr(want, n), f"blocks of 128: {n}")
    with pytest.raises(ValueError):
        _hip.explain_desc([state], [keep], [wd], [outs], k, rows_per_block=100)
    with pytest.raises(ValueError):
        _hip.explain_desc([state], [keep], [wd], [outs], 17)
    with pytest.raises(ValueError):
        _hip.explain_desc([state], [keep], [wd.to(torch.int64)], [outs], k)
    for bad in ([500], [-1]):
        with pytest.raises(ValueError):
            _hip.explain_rows([state], [keep], k, which=[np.array(bad)])
        with pytest.raises(ValueError):
            eng.explain_rows([det], [x], top_k=k, which=[bad])
    with pytest.raises(ValueError):
        eng.explain_rows([det], [x], top_k=0)
    with pytest.raises(ValueError):
        eng.explain_rows([det], [x[:, :50]])
