"""``incident_sig_kernel`` + ``incident_sig_fold_kernel`` (fedmx_signature.hip)
and ``HipEngine.incident_signatures`` on the GPU.

Every field of the rule (``rows``, ``err_sum``, ``resid_sum``, ``bad``) must
equal, bit for bit, the oracle ``signature_sums`` applied to the residuals
``HipEngine.explain_rows(dense=True, which=L)`` returns for the same list: a
row's forward does not depend on its tile neighbours, so the kernels' own
residual bits are the yardstick (the stance tests/test_explain_rows_gpu.py takes
for ``idx`` / ``resid``).  The derived fields must equal ``signatures_report``
of those.

Shapes: 115/27/7 (compact forward order), 127/31/15 (identity order), 5/3/2
and 1/1/1; float32 and float64 rows; both scalers; list lengths bracketing the
16-position tile, the 64-position pass and the block (R = 64 and 128), with
incident boundaries inside a tile, at a tile edge and at a block edge, sixteen
one-row incidents in one tile, one incident over four blocks and, at R = 64,
one over ten (the fold kernel's loop is unrolled by four)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.data.prepare import fitted_scaler_arrays
from fedmse_decentralized_amd.data.scaler import IoTDataProcessor
from fedmse_decentralized_amd.deploy.detector import (Detector, Incidents, Signatures, incidents_numpy,
                                                      signature_list, signature_sums, signatures_report)
from fedmse_decentralized_amd.models.layout import ModelDims

DEV = torch.device("cuda", 0)
DIMS = [ModelDims(115, 27, 7), ModelDims(127, 31, 15), ModelDims(5, 3, 2), ModelDims(1, 1, 1)]
FIELDS = ("incidents", "rows", "err_sum", "resid_sum", "bad", "idx", "share", "mean_resid")
_ENGINES = {}


def engine(dims=DIMS[0]):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    if dims not in _ENGINES:
        _ENGINES[dims] = HipEngine(dims, DEV)
    return _ENGINES[dims]


def raw_rows(rng, n, D, dtype=np.float64):
    mag = 10.0 ** np.linspace(-2, 6, D)
    x = rng.normal(size=(n, D)) * mag + mag
    x[:, D // 2] = 3.5
    return x.astype(dtype)


def make_detector(dims, scaler="standard", seed=0):
    rng = np.random.default_rng(1000 * dims.d_in + seed)
    proc = IoTDataProcessor(scaler)
    proc.fit_transform(raw_rows(rng, 120, dims.d_in))
    sc = fitted_scaler_arrays(proc, scaler)
    sc.pop("kind")
    params = (rng.normal(size=dims.num_params) * 0.4 / np.sqrt(dims.hidden)).astype(np.float32)
    return Detector(dims=dims, model_type="autoencoder", params=params, scaler_kind=scaler, scaler=sc,
                    detect_quantile=0.9)


def layout(m, cuts):
    """Flags and incidents whose list has exactly ``m`` positions, a new
    incident starting at every list position in ``cuts`` (those below m):
    inside an incident every third raw row is unflagged, and between two
    incidents lie an unflagged row, a flagged row that belongs to none, and
    another unflagged one."""
    starts = [0] + sorted(c for c in set(cuts) if 0 < c < m)
    sizes = [b - a for a, b in zip(starts, starts[1:] + [m])]
    flags, start, end = [0, 1, 0], [], []
    for c in sizes:
        start.append(len(flags))
        for k in range(c):
            flags.append(1)
            if k % 3 == 1 and k + 1 < c:
                flags.append(0)
        end.append(len(flags) - 1)
        flags += [0, 3, 0]   # (a flag of another value than 1 counts as well, but lies outside)
    flags = np.array(flags, np.uint8)
    start, end = np.array(start, np.int64), np.array(end, np.int64)
    k = len(sizes)
    inc = Incidents(n=int(flags.shape[0]), window=1, min_alarms=1, hold=0, start=start, end=end,
                    alarms=np.array(sizes, np.int64), peak_row=start.copy(), peak_score=np.zeros(k),
                    hot_rows=int(sum(sizes)), count=k, rows_covered=int((end - start + 1).sum()),
                    longest=int((end - start + 1).max()))
    L, seg, rows = signature_list(flags, inc)
    assert L.shape[0] == m and rows.tolist() == sizes
    return flags, inc


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {got} vs {want}"


def check(eng, dets, rows, flags, incs, got, R, top_k, which=None, what=""):
    """The call's results against ``signature_sums`` of the engine's own dense
    residuals of the same lists (one ``explain_rows`` call for all items)."""
    which = which if which is not None else [None] * len(dets)
    lists = [signature_list(f, inc, w) for f, inc, w in zip(flags, incs, which)]
    ex = eng.explain_rows(dets, rows, top_k=1, which=[l[0] for l in lists], dense=True)
    out = []
    for i, (det, (L, seg, cnt), e, g) in enumerate(zip(dets, lists, ex, got)):
        w = np.arange(incs[i].count, dtype=np.int64) if which[i] is None else np.asarray(which[i], np.int64)
        assert isinstance(g, Signatures) and g.block_rows == R, (what, i)
        assert e.resid_full.shape == (L.shape[0], det.dims.d_in)
        want = signatures_report(w, cnt, R, *signature_sums(e.resid_full, seg, w.shape[0], R), top_k)
        for k in FIELDS:
            same_bits(getattr(g, k), getattr(want, k), f"{what} item {i} m={L.shape[0]} {k}")
        out.append((L, seg, e.resid_full))
    return out


def lengths(R):
    return sorted({1, 15, 16, 17, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3})


@pytest.mark.parametrize("scaler", ["standard", "minmax"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d.d_in}-{d.hidden}-{d.latent}")
def test_every_field_matches_the_oracle_on_the_kernels_residuals(dims, dtype, scaler):
    """Every list length as one item of a single call per block size (the same
    weights; different rows and incidents)."""
    det = make_detector(dims, scaler)
    D = dims.d_in
    eng = engine(dims)
    rng = np.random.default_rng(41)
    for R in (64, 128):
        # boundaries inside a tile, at a tile edge, inside the second pass, at the block edge and just behind it
        cuts = (5, 16, 70, R, R + 7)
        items = [(m, cuts) for m in lengths(R)]
        items.append((40, tuple(range(16, 33))))   # sixteen one-row incidents in the second tile
        items.append((3 * R + 10, (R - 3,)))       # the second incident lies in blocks 0, 1, 2 and 3
        if R == 64:
            items.append((9 * R + 10, (R - 3,)))   # ... in blocks 0 to 9: the fold walks past its four-block unroll
        flags, incs, rows = [], [], []
        for m, c in items:
            f, inc = layout(m, c)
            x = raw_rows(rng, inc.n, D, dtype)
            L = signature_list(f, inc)[0]
            if m >= 17:   # NaN, +inf and -inf in listed rows and in one that is not
                x[L[2], 0] = np.nan
                x[L[m - 1], D - 1] = np.inf
                x[L[m // 2], D // 3] = -np.inf
                x[0, 0] = np.nan
            flags.append(f)
            incs.append(inc)
            rows.append(x)
        dets = [det] * len(items)
        got = eng.incident_signatures(dets, rows, flags, incs, top_k=3, block_rows=R)
        what = f"{D}/{dims.hidden}/{dims.latent} {scaler} {np.dtype(dtype).name} R={R}"
        ref = check(eng, dets, rows, flags, incs, got, R, 3, what=what)
        for (m, c), g, inc, (L, seg, resid) in zip(items, got, incs, ref):
            assert int(g.rows.sum()) == m and g.err_sum.shape == (inc.count, D), what
            assert np.all(g.err_sum >= 0.0) and np.isfinite(g.err_sum).all() and np.isfinite(g.resid_sum).all(), what
            if m >= 17:
                assert g.bad[seg[2], 0] >= 1 and g.bad[seg[m - 1], D - 1] >= 1 and g.bad[seg[m // 2], D // 3] >= 1, what
                assert int(g.bad.sum()) == int((~np.isfinite(resid * resid)).sum()), what
            else:
                assert not g.bad.any(), what
            if len(c) == 17:
                assert inc.count == 18 and g.rows[1:17].tolist() == [1] * 16, what
            if m == 3 * R + 10:
                assert g.rows.tolist() == [R - 3, 2 * R + 13], what
            if m == 9 * R + 10:
                assert g.rows.tolist() == [R - 3, 8 * R + 13], what


def test_real_incidents_a_subset_and_two_detectors_in_one_call(monkeypatch):
    """Incidents from ``incidents_numpy`` (hold 0: one-row incidents among
    longer ones), a ``which`` subset, two detectors of different shapes, input
    types and lengths in one call with the default block size; launch counts."""
    from fedmse_decentralized_amd.ops import _hip

    rng = np.random.default_rng(9)
    a, b = make_detector(DIMS[0], "standard", seed=1), make_detector(DIMS[2], "minmax", seed=2)
    fa = (rng.random(700) < 0.55).astype(np.uint8)
    fa[100:132:2], fa[101:132:2] = 1, 0            # sixteen one-row incidents (window 1, hold 0)
    fb = (rng.random(150) < 0.5).astype(np.uint8)
    ia, ib = incidents_numpy(fa, rng.normal(size=700), 1, 1, 0), incidents_numpy(fb, rng.normal(size=150), 3, 2, 1)
    assert ia.count > 40 and ib.count >= 3
    xa, xb = raw_rows(rng, 700, 115, np.float64), raw_rows(rng, 150, 5, np.float32)
    wa = np.flatnonzero(rng.random(ia.count) < 0.7)
    ma, mb = signature_list(fa, ia, wa)[0].shape[0], signature_list(fb, ib)[0].shape[0]
    calls = []
    lib = _hip.lib()
    for name in ("fedmx_incident_signatures", "fedmx_explain_rows", "fedmx_score_rows", "fedmx_incidents",
                 "fedmx_monitor_rows"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: calls.append((_n, a[1])) or _r(*a))
    eng = engine()
    got = eng.incident_signatures([a, b], [xa, torch.from_numpy(xb).to(DEV)], [fa, torch.from_numpy(fb)], [ia, ib],
                                  which=[wa, None])
    R = _hip.score_rows_per_block(ma + mb)
    # one entry: incident_sig_kernel over the blocks, incident_sig_fold_kernel over the incidents
    assert calls == [("fedmx_incident_signatures", -(-ma // R) + -(-mb // R))], calls
    assert got[0].idx.shape == (len(wa), 5) and got[1].idx.shape == (ib.count, 5)
    del calls[:]
    check(eng, [a, b], [xa, xb], [fa, fb], [ia, ib], got, R, 5, which=[wa, None], what="two detectors")
    assert calls == [("fedmx_explain_rows", -(-ma // R) + -(-mb // R))], calls     # explain_rows: its one launch
    del calls[:]
    small = eng.incident_signatures([a, b], [xa, xb], [fa, fb], [ia, ib], top_k=2, which=[wa, None], block_rows=64)
    check(eng, [a, b], [xa, xb], [fa, fb], [ia, ib], small, 64, 2, which=[wa, None], what="two detectors R=64")
    # nothing to do: no launch; an empty item beside a live one gets no workgroup
    del calls[:]
    quiet = incidents_numpy(np.zeros(150, np.uint8), np.zeros(150), 3, 2, 1)
    none = eng.incident_signatures([b, a], [xb, xa], [np.zeros(150, np.uint8), fa], [quiet, ia],
                                   which=[None, np.zeros(0, np.int64)])
    assert calls == [] and none[0].err_sum.shape == (0, 5) and none[1].err_sum.shape == (0, 115)
    assert eng.incident_signatures([], [], [], []) == []
    mixed = eng.incident_signatures([b, b], [xb, xb], [np.zeros(150, np.uint8), fb], [quiet, ib], block_rows=64)
    assert calls == [("fedmx_incident_signatures", -(-mb // 64))] and mixed[0].rows.shape == (0,)
    check(eng, [b], [xb], [fb], [ib], mixed[1:], 64, 5, what="after an empty item")
    # the neighbours launch what they launched before
    del calls[:]
    eng.score_incidents([a], [xa], 8, 3, 2)
    assert [c[0] for c in calls] == ["fedmx_score_rows", "fedmx_incidents"], calls
    del calls[:]
    eng.explain_rows([a], [xa], top_k=3, which=[np.arange(10)])
    assert calls == [("fedmx_explain_rows", 1)], calls
    for bad in (dict(top_k=0), dict(block_rows=96), dict(which=[np.array([2, 1]), None])):
        with pytest.raises(ValueError):
            eng.incident_signatures([a, b], [xa, xb], [fa, fb], [ia, ib], **bad)
    with pytest.raises(ValueError):
        eng.incident_signatures([a, b], [xa[:-1], xb], [fa, fb], [ia, ib])
