"""Incident signatures on the host (README "Incident signatures"): the oracle
``signature_sums`` against a per-row loop written straight from the rule,
``signature_list`` against a row-by-row walk, ``TorchEngine.incident_signatures``
against the oracle, a planted burst on a trained federation's detector, and the
``detect --signatures`` tool."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.deploy.detector import (SIGNATURE_MAX_INCIDENTS, Detector, Incidents, Signatures,
                                                      check_signature_which, explain_rows_numpy,
                                                      incident_signatures_numpy, incidents_numpy, score_rows_numpy,
                                                      signature_list, signature_sums, signatures_report)
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
from fedmse_decentralized_amd.models.layout import ModelDims

DIMS = ModelDims(5, 3, 2)
RULE = ("rows", "err_sum", "resid_sum", "bad")
DERIVED = ("incidents", "idx", "share", "mean_resid")


def make_detector(dims=DIMS, scaler="standard", seed=0, threshold=0.75):
    rng = np.random.default_rng(seed)
    D = dims.d_in
    if scaler == "standard":
        sc = {"mean_": rng.normal(size=D), "scale_": rng.uniform(0.5, 2.0, size=D)}
    else:
        sc = {"scale_": rng.uniform(0.5, 2.0, size=D), "min_": rng.normal(size=D)}
    return Detector(dims=dims, model_type="autoencoder", params=(0.3 * rng.normal(size=dims.num_params)).astype(np.float32),
                    scaler_kind=scaler, scaler=sc, threshold=threshold, detect_quantile=0.9)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_signatures(got, want):
    assert isinstance(got, Signatures) and got.block_rows == want.block_rows
    for k in RULE + DERIVED:
        assert same_bits(getattr(got, k), getattr(want, k)), (k, getattr(got, k), getattr(want, k))


# ---------------------------------------------------------------------------
# steps 3 and 4
# ---------------------------------------------------------------------------
def loop_sums(resid, seg, s, R):
    """Steps 3 and 4 of the rule, one list position at a time."""
    m, D = resid.shape
    nb = -(-m // R)
    part = {}   # (block, incident, wave) -> [se, sr, bad] per feature
    for b in range(nb):
        hi = min(m, (b + 1) * R)
        ntiles = -(-(hi - b * R) // 16)
        for w in range(4):
            for t in range(w, ntiles, 4):
                for p in range(b * R + 16 * t, min(hi, b * R + 16 * t + 16)):
                    acc = part.setdefault((b, int(seg[p]), w), [[0.0] * D, [0.0] * D, [0] * D])
                    for d in range(D):
                        r = resid[p, d]
                        with np.errstate(all="ignore"):
                            e = np.float32(r * r)
                        if not np.isfinite(e):
                            acc[2][d] += 1
                        else:
                            acc[0][d] = acc[0][d] + float(e)
                            acc[1][d] = acc[1][d] + float(r)
    err, res, bad = np.zeros((s, D)), np.zeros((s, D)), np.zeros((s, D), np.int64)
    zero = [[0.0] * D, [0.0] * D, [0] * D]
    for j in range(s):
        pos = np.flatnonzero(seg == j)
        if not pos.size:
            continue
        for b in range(int(pos[0]) // R, int(pos[-1]) // R + 1):
            p = [part.get((b, j, w), zero) for w in range(4)]
            for d in range(D):
                for k, out in ((0, err), (1, res)):
                    out[j, d] = out[j, d] + (((p[0][k][d] + p[1][k][d]) + p[2][k][d]) + p[3][k][d])
                bad[j, d] += p[0][2][d] + p[1][2][d] + p[2][2][d] + p[3][2][d]
    return err, res, bad


def random_case(rng, m_max=300):
    R = int(rng.choice([64, 128]))
    m = int(rng.integers(0, m_max + 1))
    s = int(rng.integers(1, 21))
    D = int(rng.integers(1, 4))
    # rising incident positions; some incidents may get no position at all
    seg = np.sort(rng.integers(0, s, size=m)).astype(np.int32)
    mag = 10.0 ** rng.integers(-3, 8, size=(m, D))
    resid = (rng.normal(size=(m, D)) * mag).astype(np.float32)
    if m:
        k = max(1, m // 20)
        resid[rng.integers(0, m, size=k), rng.integers(0, D, size=k)] = \
            rng.choice(np.array([np.nan, np.inf, -np.inf, 3e30, -0.0], np.float32), size=k)   # (3e30^2: +inf in fp32)
    return resid, seg, s, R


def test_signature_sums_equals_the_per_row_loop():
    rng = np.random.default_rng(11)
    seen_bad = seen_multi_block = 0
    for case in range(320):
        resid, seg, s, R = random_case(rng)
        got = signature_sums(resid, seg, s, R)
        want = loop_sums(resid, seg, s, R)
        for g, w, k in zip(got, want, ("err_sum", "resid_sum", "bad")):
            assert same_bits(g, w), (case, k, R, resid.shape, g, w)
        seen_bad += int(got[2].any())
        seen_multi_block += int(resid.shape[0] > 2 * R)
    assert seen_bad > 100 and seen_multi_block > 20


def test_signature_sums_order_is_the_rule():
    """Values whose float64 sum depends on the order: 2^60 +- small ones."""
    R, m = 64, 150
    resid = np.ones((m, 1), np.float32)
    resid[[0, 17, 70, 149], 0] = np.float32(2.0 ** 30)    # e = 2^60: later ones vanish beside it, earlier ones count
    seg = np.r_[np.zeros(20, np.int32), np.ones(110, np.int32), np.full(20, 2, np.int32)]
    got = signature_sums(resid, seg, 3, R)
    want = loop_sums(resid, seg, 3, R)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    # two streams by hand: stream 0 (tile 0) starts with e = 2^60 and absorbs its fifteen 64s (ulp 256); stream 1
    # (tile 1) sums sixteen 64s to 1024, which the fold then adds exactly.  One left-to-right sum would give 2^60.
    two = np.full((32, 1), 8.0, np.float32)
    two[0, 0] = np.float32(2.0 ** 30)
    e, r, b = signature_sums(two, np.zeros(32, np.int32), 1, R)
    assert e[0, 0] == 2.0 ** 60 + 1024.0 and r[0, 0] == 2.0 ** 30 + 248.0 and b[0, 0] == 0
    with pytest.raises(ValueError):
        signature_sums(resid, seg[::-1].copy(), 3, R)
    with pytest.raises(ValueError):
        signature_sums(resid, seg, 2, R)
    with pytest.raises(ValueError):
        signature_sums(resid, seg, 3, 100)
    z = signature_sums(resid[:0], seg[:0], 3, R)
    assert z[0].shape == (3, 1) and not z[0].any() and not z[1].any() and not z[2].any()


# ---------------------------------------------------------------------------
# step 1
# ---------------------------------------------------------------------------
def walk_list(flags, inc, which):
    L, seg = [], []
    for i in range(len(flags)):
        for j, k in enumerate(which):
            if flags[i] != 0 and inc.start[k] <= i <= inc.end[k]:
                L.append(i)
                seg.append(j)
    return np.array(L, np.int64), np.array(seg, np.int32)


def random_incidents(rng):
    n = int(rng.integers(1, 200))
    flags = (rng.random(n) < rng.choice([0.1, 0.3, 0.6, 0.9])).astype(np.uint8) * int(rng.integers(1, 4))
    w = int(rng.integers(1, 12))
    return flags, incidents_numpy(flags, rng.normal(size=n), w, int(rng.integers(1, w + 1)), int(rng.integers(0, 6)))


def test_signature_list_equals_a_walk_and_every_incident_has_a_row():
    rng = np.random.default_rng(4)
    walked = 0
    for case in range(1000):
        flags, inc = random_incidents(rng)
        L, seg, rows = signature_list(flags, inc)
        assert L.dtype == np.int64 and seg.dtype == np.int32 and rows.dtype == np.int64
        assert rows.shape == (inc.count,) and np.all(rows >= 1), (case, rows)
        assert int(rows.sum()) == L.shape[0] and np.all(rows <= inc.alarms)
        if case % 5 == 0:
            which = np.flatnonzero(rng.random(inc.count) < 0.6)
            for w in (None, which):
                L, seg, rows = signature_list(flags, inc, w)
                wl, ws = walk_list(flags, inc, np.arange(inc.count) if w is None else w)
                assert same_bits(L, wl) and same_bits(seg, ws), case
                assert same_bits(rows, np.bincount(ws, minlength=len(rows)).astype(np.int64))
            walked += inc.count
    assert walked > 100


def test_signature_list_refuses_a_bad_which():
    rng = np.random.default_rng(8)
    flags = (rng.random(300) < 0.5).astype(np.uint8)
    inc = incidents_numpy(flags, rng.normal(size=300), 2, 1, 0)
    assert inc.count >= 10
    for bad in ([1, 1], [2, 1], [0, inc.count], [-1, 0], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            signature_list(flags, inc, np.array(bad))
    with pytest.raises(ValueError):
        signature_list(flags[:-1], inc)
    assert same_bits(check_signature_which(None, 3), np.arange(3, dtype=np.int64))
    assert check_signature_which(np.arange(SIGNATURE_MAX_INCIDENTS), 5000).shape == (SIGNATURE_MAX_INCIDENTS,)
    with pytest.raises(ValueError):
        check_signature_which(np.arange(SIGNATURE_MAX_INCIDENTS + 1), 5000)
    with pytest.raises(ValueError):
        check_signature_which(None, SIGNATURE_MAX_INCIDENTS + 1)
    # more than 4096 incidents in the flags themselves: all of them is too many, a subset is fine
    n = 2 * (SIGNATURE_MAX_INCIDENTS + 4)
    many = np.zeros(n, np.uint8)
    many[::2] = 1
    inc = incidents_numpy(many, np.zeros(n), 1, 1, 0)
    assert inc.count == SIGNATURE_MAX_INCIDENTS + 4
    with pytest.raises(ValueError):
        signature_list(many, inc)
    L, seg, rows = signature_list(many, inc, np.arange(4, inc.count))
    assert L.tolist() == list(range(8, n, 2)) and rows.tolist() == [1] * SIGNATURE_MAX_INCIDENTS


# ---------------------------------------------------------------------------
# step 5 and the engines
# ---------------------------------------------------------------------------
def test_report_ranks_shares_and_similarity():
    err = np.array([[1.0, 4.0, 4.0, 0.0], [0.0, 0.0, 0.0, 0.0], [2.0, 8.0, 8.0, 0.0]])
    res = np.array([[-1.0, 6.0, -6.0, 0.0], [0.0] * 4, [1.0] * 4])
    bad = np.array([[0, 1, 3, 0], [0] * 4, [0] * 4], np.int64)
    sig = signatures_report(np.array([2, 5, 6]), np.array([3, 1, 2]), 64, err, res, bad, 6)
    # equal sums: the lower feature first
    assert sig.idx.dtype == np.int32 and sig.idx.tolist() == [[1, 2, 0, 3, -1, -1], [0, 1, 2, 3, -1, -1],
                                                              [1, 2, 0, 3, -1, -1]]
    assert sig.share[0].tolist() == [4 / 9, 4 / 9, 1 / 9, 0.0, 0.0, 0.0] and np.isnan(sig.share[1, :4]).all()
    assert sig.share[1, 4:].tolist() == [0.0, 0.0]
    assert sig.mean_resid[0].tolist() == [3.0, -6.0, -1 / 3, 0.0, 0.0, 0.0]     # 6 / (3 - 1), -6 / max(3 - 3, 1)
    sim = sig.similarity()
    assert sim.shape == (3, 3) and sim[0, 2] == pytest.approx(1.0) and np.isnan(sim[1]).all() and np.isnan(sim[:, 1]).all()
    assert signatures_report(np.array([0]), np.array([1]), 64, err[:1], res[:1], bad[:1], 2).idx.tolist() == [[1, 2]]
    with pytest.raises(ValueError):
        signatures_report(np.array([0]), np.array([1]), 64, err[:1], res[:1], bad[:1], 17)


def flagged_case(det, rng, n, rate=0.5, params=(4, 2, 1)):
    rows = rng.normal(size=(n, det.dims.d_in)) * 2.0
    scores = score_rows_numpy(det, rows)[0]
    det = dataclasses.replace(det, threshold=float(np.quantile(scores, 1.0 - rate)))
    scores, flags, _ = score_rows_numpy(det, rows)
    return det, rows, flags, incidents_numpy(flags, scores, *params)


def test_torch_engine_returns_the_oracles_bits():
    rng = np.random.default_rng(17)
    big = ModelDims(9, 4, 3)
    a = flagged_case(make_detector(), rng, 400)
    b = flagged_case(make_detector(big, "minmax", seed=3), rng, 90)
    a[1][5, 0] = np.nan   # (flags and incidents stay as they were: the row now counts as bad where it is listed)
    eng = TorchEngine(DIMS, torch.device("cpu"))
    assert a[3].count >= 3 and b[3].count >= 2
    wb = np.array([0, b[3].count - 1])
    got = eng.incident_signatures([a[0], b[0]], [a[1], torch.from_numpy(b[1])], [a[2], torch.from_numpy(b[2])],
                                  [a[3], b[3]], top_k=3, which=[None, wb], block_rows=64)
    same_signatures(got[0], incident_signatures_numpy(a[0], a[1], a[2], a[3], 3, block_rows=64))
    same_signatures(got[1], incident_signatures_numpy(b[0], b[1], b[2], b[3], 3, which=wb, block_rows=64))
    assert got[1].incidents.tolist() == wb.tolist() and got[0].idx.shape == (a[3].count, 3)
    # the default block size: that of all list positions of the call
    from fedmse_decentralized_amd.ops._hip import score_rows_per_block

    m = signature_list(a[2], a[3])[0].shape[0] + signature_list(b[2], b[3])[0].shape[0]
    dflt = eng.incident_signatures([a[0], b[0]], [a[1], b[1]], [a[2], b[2]], [a[3], b[3]])
    assert dflt[0].block_rows == dflt[1].block_rows == score_rows_per_block(m) and dflt[0].idx.shape[1] == 5
    # an item without an incident
    none = eng.incident_signatures([a[0]], [a[1]], [np.zeros_like(a[2])],
                                   [incidents_numpy(np.zeros_like(a[2]), np.zeros(400), 4, 2, 1)])[0]
    assert none.rows.shape == (0,) and none.err_sum.shape == (0, 5) and none.similarity().shape == (0, 0)
    for bad in (dict(top_k=0), dict(top_k=17), dict(block_rows=100), dict(which=[np.array([1, 0])])):
        with pytest.raises(ValueError):
            eng.incident_signatures([a[0]], [a[1]], [a[2]], [a[3]], **bad)
    with pytest.raises(ValueError):
        eng.incident_signatures([a[0]], [a[1][:-1]], [a[2]], [a[3]])
    with pytest.raises(ValueError):
        eng.incident_signatures([a[0], b[0]], [a[1]], [a[2]], [a[3]])


def test_a_single_stream_sums_left_to_right():
    rng = np.random.default_rng(23)
    det, rows, flags, inc = flagged_case(make_detector(seed=5), rng, 40, rate=0.3, params=(6, 2, 3))
    L, seg, cnt = signature_list(flags, inc)
    assert 1 <= L.shape[0] <= 16 and inc.count >= 1, (L.shape, inc.count)
    sig = incident_signatures_numpy(det, rows, flags, inc, 2, block_rows=64)
    r = explain_rows_numpy(det, rows, 2, which=L, dense=True).resid_full
    e = (r * r).astype(np.float64)
    for j in range(inc.count):
        acc, accr = np.zeros(5), np.zeros(5)
        for p in np.flatnonzero(seg == j):
            acc, accr = acc + e[p], accr + r[p].astype(np.float64)
        assert same_bits(sig.err_sum[j], acc) and same_bits(sig.resid_sum[j], accr)
    assert same_bits(sig.rows, cnt) and not sig.bad.any()


# ---------------------------------------------------------------------------
# a planted burst on a trained detector
# ---------------------------------------------------------------------------
BURST_SHIFT = 16.0         # train standard deviations added to the burst's feature (chosen on the oracle, see the test)
BURST_F, BURST_G = 7, 60
BURSTS = ((30, 60, BURST_F), (90, 120, BURST_G), (150, 180, BURST_F), (200, 230, BURST_G))


@pytest.fixture(scope="module")
def trained():
    """A small synthetic federation run to its end, as tests/test_monitor_rows.py
    builds one: (engine, client 0's detector, its benign raw test rows)."""
    import test_monitor_rows as tm
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    import tempfile

    mp = pytest.MonkeyPatch()
    mp.setattr(synthetic.SyntheticSpec, "resolved", tm._small(synthetic.SyntheticSpec.resolved))
    federation._PREP_CACHE.clear()
    try:
        with tempfile.TemporaryDirectory() as out:
            cfg = tm._cfg(out, export_baseline=False)
            fed = federation.Federation(cfg, "autoencoder", "avg", 0).setup()
            fed.run_all()
            _, _, _, test_raw, labels = tm.raw_splits(cfg)[0]
            det = Detector.load(os.path.join(fed.save_dirs[0], "detector.npz"))
            yield fed.engine, det, test_raw[labels == 0]
    finally:
        mp.undo()
        federation._PREP_CACHE.clear()


def test_a_planted_burst_names_its_feature(trained):
    """A condition on the rule (the oracle alone).  240 rows drawn with
    repeats from the benign test rows the detector does not flag; four runs of
    30 rows get BURST_SHIFT train standard deviations added to one feature: f,
    g, f again, g again.  Each run must come out as one incident that ranks its
    feature first with a negative mean residual (the model reconstructs the
    value it knows, below the shifted one), and an f-incident must resemble
    the other f-incident more than a g-incident.  The shift was chosen on this
    oracle among 4, 8, 16 and 32: at 4 and 8 too few burst rows pass the
    threshold for an incident (6 of 8 rows); at 16 every burst row is flagged,
    the four incidents hold 25 flagged rows each, the burst's feature carries
    0.76 to 0.81 of the summed squared residual (the next feature 0.005) and
    the similarities are 0.9999 within a feature and 0.006 across."""
    eng, det, benign = trained
    assert det.scaler_kind == "standard"
    quiet = benign[score_rows_numpy(det, benign, engine=eng)[1] == 0]
    assert quiet.shape[0] >= 5
    rng = np.random.default_rng(3)
    rows = quiet[rng.integers(0, quiet.shape[0], size=240)].copy()
    for a, b, d in BURSTS:
        rows[a:b, d] += BURST_SHIFT * det.scaler["scale_"][d]
    scores, flags, _ = score_rows_numpy(det, rows, engine=eng)
    inc = incidents_numpy(flags, scores, 8, 6, 4)
    own = [int(np.flatnonzero((inc.start <= a + 8) & (inc.end >= b - 1))[0]) for a, b, _ in BURSTS]
    assert len(set(own)) == 4, (inc.start, inc.end)
    sig = incident_signatures_numpy(det, rows, flags, inc, 5, which=np.array(own), block_rows=64, engine=eng)
    print("shares", sig.share[:, :2], "mean_resid", sig.mean_resid[:, 0], "similarity", sig.similarity())
    for j, (a, b, d) in enumerate(BURSTS):
        assert sig.rows[j] >= 25 and sig.idx[j, 0] == d, (j, sig.idx[j], sig.share[j])
        assert sig.share[j, 0] > 0.5 and sig.share[j, 0] > 10.0 * sig.share[j, 1], (j, sig.share[j])
        assert sig.mean_resid[j, 0] < 0.0, (j, sig.mean_resid[j])
    sim = sig.similarity()
    cross = max(sim[0, 1], sim[0, 3], sim[2, 1], sim[2, 3])
    assert cross < sim[0, 2] and cross < sim[1, 3], sim


# ---------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------
INCIDENT_KEYS = ["incident_" + k for k in ("start", "end", "alarms", "peak_row", "peak_score", "params")]
SIGNATURE_KEYS = ["signature_" + k for k in ("incident", "rows", "idx", "share", "mean_resid", "err_sum", "resid_sum",
                                             "bad", "similarity")]


def test_detect_signatures(tmp_path, capsys):
    from fedmse_decentralized_amd import detect

    rng = np.random.default_rng(2)
    det, rows, flags, inc = flagged_case(make_detector(), rng, 300)
    assert inc.count >= 4
    bundle = det.save(str(tmp_path / "detector.npz"))
    csv = str(tmp_path / "traffic.csv")
    np.savetxt(csv, rows, delimiter=",", fmt="%.17g")
    base = ["--detector", bundle, "--input", csv, "--backend", "torch", "--incidents", "--incident-window", "4",
            "--incident-min", "2", "--incident-hold", "1"]
    plain, out = str(tmp_path / "plain.npz"), str(tmp_path / "sig.npz")
    # without the flag: the keys and arrays of before it existed
    assert detect.main(base + ["--output", plain]) == 0
    plain_lines = capsys.readouterr().out.strip().splitlines()
    assert len(plain_lines) == 2 and plain_lines[1].startswith("incidents: ")
    eng = TorchEngine(DIMS, torch.device("cpu"))
    s, f, a, want_inc = eng.score_incidents([det], [rows], 4, 2, 1)[0]
    with np.load(plain, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["scores", "flags", "alarms", "threshold"] + INCIDENT_KEYS)
        before = {k: z[k] for k in z.files}
    assert same_bits(before["scores"], s) and same_bits(before["flags"], f) and int(before["alarms"]) == a
    for k in ("start", "end", "alarms", "peak_row", "peak_score"):
        assert same_bits(before["incident_" + k], getattr(want_inc, k)), k
    assert before["incident_params"].tolist() == [4, 2, 1] and float(before["threshold"]) == det.threshold
    # with it
    assert detect.main(base + ["--output", out, "--signatures", "3", "--signature-top", "2"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3 and lines[1] == plain_lines[1] and lines[2].startswith("# signatures: incidents 3 top_k 2 ")
    order = sorted(range(inc.count), key=lambda k: (-int(inc.alarms[k]), k))[:3]
    which = np.array(sorted(order), np.int64)
    want = eng.incident_signatures([det], [rows], [f], [want_inc], top_k=2, which=[which])[0]
    assert lines[2].split().count("incident") == 3 and f"incident {int(which[0])} rows {int(want.rows[0])} " in lines[2]
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(list(before) + SIGNATURE_KEYS)
        for k, v in before.items():
            assert same_bits(z[k], v), k
        assert same_bits(z["signature_incident"], which)
        for k in ("rows", "idx", "share", "mean_resid", "err_sum", "resid_sum", "bad"):
            assert same_bits(z["signature_" + k], getattr(want, k)), k
        assert same_bits(z["signature_similarity"], want.similarity()) and z["signature_similarity"].shape == (3, 3)
    # more incidents asked for than there are: all of them
    assert detect.main(base + ["--output", out, "--signatures", "4096"]) == 0
    capsys.readouterr()
    with np.load(out, allow_pickle=False) as z:
        assert z["signature_incident"].tolist() == list(range(inc.count)) and z["signature_idx"].shape == (inc.count, 5)
    for bad in (["--signatures", "0"], ["--signatures", "4097"], ["--signatures", "2", "--signature-top", "0"],
                ["--signatures", "2", "--signature-top", "17"]):
        with pytest.raises(SystemExit):
            detect.main(base + bad)
        capsys.readouterr()
    with pytest.raises(SystemExit):   # --signatures without --incidents
        detect.main(["--detector", bundle, "--input", csv, "--backend", "torch", "--signatures", "2"])
    capsys.readouterr()
