"""Calibrated detection thresholds and operating-point metrics (README
"Detection thresholds"): the rank rule, ``TorchEngine.detect_metrics`` against
a literal numpy oracle (clean, ``np.sort(c)[j]``, compare, count) bit for
bit, the evaluator's two metrics, config ranges, the report line and a 2-rank
gloo federation.  The oracle and the case list are shared with the GPU tests
(tests/test_detection_metrics_gpu.py)."""
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmse_decentralized_amd.config import ExperimentConfig
from fedmse_decentralized_amd.eval.metrics import DETECT_FIELDS, calibration_rank, detection_fields

DBL_MAX = np.finfo(np.float64).max
SCALE = 1.0 / 115   # the AE's score_scale (fp32 SSE -> per-row MSE)


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def clean(v, scale):
    v = np.asarray(v)
    if v.dtype == np.float32:
        v = (v * np.float32(scale)).astype(np.float64)   # fp32 product, then widened
    v = v.astype(np.float64).copy()
    v[np.isnan(v)] = 0.0
    v[v == np.inf] = DBL_MAX
    v[v == -np.inf] = -DBL_MAX
    return v


def oracle(calib, scores, labels, j, calib_labels=None, scale=1.0, value="f1"):
    """[8] float64: value, tau, tp, fp, fn, tn, precision, recall."""
    c = clean(calib, scale)
    if calib_labels is not None:
        c = c[np.asarray(calib_labels) == 0]
    tau = float("nan")
    if j >= 0:
        tau = float(np.sort(c)[j])
        if tau == 0.0:
            tau = 0.0
    s = clean(scores, scale)
    y = np.asarray(labels) != 0
    pred = s > tau
    tp, fp = int(np.sum(pred & y)), int(np.sum(pred & ~y))
    fn, tn = int(np.sum(~pred & y)), int(np.sum(~pred & ~y))
    if math.isnan(tau) or not y.any() or y.all():
        precision = recall = f1 = float("nan")
    else:
        precision = tp / (tp + fp) if tp + fp else 0.0
        recall = tp / (tp + fn) if tp + fn else 0.0
        f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return np.array([recall if value == "recall" else f1, tau, tp, fp, fn, tn, precision, recall], dtype=np.float64)


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).reshape(-1)
                         & ~(np.isnan(got) & np.isnan(want)).reshape(-1))
    assert bad.size == 0, f"{what}: entries {bad[:8].tolist()} differ: {got.reshape(-1)[bad[:8]]} vs " \
                          f"{want.reshape(-1)[bad[:8]]}"


# ---------------------------------------------------------------------------
# the case list: dicts(calib, scores, labels, j, calib_labels | None, scale, value)
# ---------------------------------------------------------------------------
SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 8193, 20000]


def _from_key(k):
    """The double whose sortable key (sign set -> ~bits, else bits | 1 << 63) is k."""
    k = np.asarray(k, dtype=np.uint64)
    top = np.uint64(1) << np.uint64(63)
    bits = np.where((k & top) != 0, k ^ top, ~k)
    return bits.view(np.float64)


def _test_set(rng, calib, n, dtype):
    """Test scores around the calibration values (some exactly equal to them), mixed labels."""
    c = np.asarray(calib, dtype=np.float64)
    c = np.nan_to_num(c)
    s = rng.choice(c, size=n) if c.size else rng.normal(size=n)
    s = s + rng.choice([0.0, 0.0, 0.5, -0.5], size=n) * (np.abs(s) + 1.0)
    return s.astype(dtype), (rng.random(n) < 0.6).astype(np.int32)


def case(calib, scores, labels, j, calib_labels=None, scale=1.0, value="f1", name=""):
    return dict(calib=calib, scores=scores, labels=np.asarray(labels, dtype=np.int32), j=int(j),
                calib_labels=None if calib_labels is None else np.asarray(calib_labels, dtype=np.int32),
                scale=scale, value=value, name=name)


def make_cases():
    rng = np.random.default_rng(20250)
    out = []
    for n_c in SIZES:
        for dtype in (np.float64, np.float32):
            scale = 1.0 if dtype == np.float64 else SCALE
            c = (rng.gamma(2.0, 3.0, size=n_c) * (1.0 if dtype == np.float64 else 115.0)).astype(dtype)
            s, y = _test_set(rng, c if dtype == np.float64 else c.astype(np.float64), min(2 * n_c + 3, 3000), dtype)
            for j in sorted({0, n_c - 1, calibration_rank(n_c, 0.95)}):
                out.append(case(c, s, y, j, scale=scale, name=f"n_c={n_c} {np.dtype(dtype).name} j={j}"))
    n_c = 1025
    mid = calibration_rank(n_c, 0.95)
    y0 = (rng.random(700) < 0.5).astype(np.int32)
    # all equal
    c = np.full(n_c, 3.25)
    out.append(case(c, np.r_[c[:350], c[:350] + 1e-9], y0, mid, name="all equal"))
    # keys that differ only in the lowest / the highest byte
    base = np.float64(1.5).view(np.uint64) | (np.uint64(1) << np.uint64(63))
    low = _from_key(base + rng.integers(0, 256, size=n_c).astype(np.uint64))
    out.append(case(low, rng.choice(low, size=700), y0, mid, name="lowest key byte"))
    out.append(case(low, rng.choice(low, size=700), y0, 0, name="lowest key byte j=0"))
    high = _from_key((rng.integers(0, 256, size=n_c).astype(np.uint64) << np.uint64(56))
                     | np.uint64(0x000F_0000_0000_0000))
    high = high[np.isfinite(high)]
    out.append(case(high, rng.choice(high, size=700), y0, calibration_rank(high.size, 0.95), name="highest key byte"))
    out.append(case(high, rng.choice(high, size=700), y0, high.size // 2, name="highest key byte mid"))
    # mixed signs, +-0
    mixed = rng.normal(size=n_c)
    out.append(case(mixed, rng.choice(mixed, size=700), y0, n_c // 2, name="mixed signs"))
    out.append(case(mixed.astype(np.float32), rng.choice(mixed, size=700).astype(np.float32), y0, n_c // 3,
                    scale=SCALE, name="mixed signs f32"))
    zeros = np.r_[np.full(300, -0.0), np.full(300, 0.0), -np.abs(rng.normal(size=200)), np.abs(rng.normal(size=225))]
    rng.shuffle(zeros)
    sz = np.r_[np.full(200, -0.0), np.full(200, 0.0), rng.normal(size=300) * 1e-3]
    for j in (199, 200, 499, 500, 799, 800):   # below, the -0 / +0 run and its two ends, above
        out.append(case(zeros, sz, y0, j, name=f"+-0 j={j}"))
    # NaN and +-inf among the inputs
    bad = rng.normal(size=n_c)
    bad[rng.choice(n_c, 60, replace=False)] = np.nan
    bad[rng.choice(n_c, 20, replace=False)] = np.inf
    bad[rng.choice(n_c, 20, replace=False)] = -np.inf
    sb = rng.normal(size=700)
    sb[::7], sb[3::11], sb[5::13] = np.nan, np.inf, -np.inf
    for j in (0, 10, n_c // 2, n_c - 5, n_c - 1):
        out.append(case(bad, sb, y0, j, name=f"nan/inf j={j}"))
    out.append(case(bad.astype(np.float32), sb.astype(np.float32), y0, n_c - 1, scale=SCALE, name="nan/inf f32"))
    # duplicates straddling rank j; test scores equal to tau
    dup = np.r_[np.arange(400, dtype=np.float64), np.full(300, 400.0), 401.0 + np.arange(325)]
    rng.shuffle(dup)
    sd = np.r_[np.full(300, 400.0), np.full(200, 399.0), np.full(200, 401.0)]
    for j in (399, 400, 550, 699, 700):
        out.append(case(dup, sd, y0, j, name=f"duplicates j={j}"))
    # interleaved label filter (tpr_at_fpr: calibration = the test scores with label 0)
    for n in (1, 2, 257, 1025, 8193):
        for dtype in (np.float64, np.float32):
            s = (rng.gamma(2.0, 3.0, size=n) + 4.0 * (np.arange(n) % 3 == 1)).astype(dtype)
            y = (np.arange(n) % 3 == 1).astype(np.int32)
            n0 = int(np.sum(y == 0))
            for q in (0.99, 0.9):
                out.append(case(s, s, y, calibration_rank(n0, q), calib_labels=y,
                                scale=1.0 if dtype == np.float64 else SCALE, value="recall",
                                name=f"filter n={n} {np.dtype(dtype).name} q={q}"))
    s = rng.normal(size=300)
    out.append(case(s, s, np.ones(300), calibration_rank(0, 0.99), calib_labels=np.ones(300), value="recall",
                    name="filter, no label-0 row"))
    # n = 0, single-class test sets, j = -1
    c = rng.normal(size=257)
    out.append(case(c, np.zeros(0), np.zeros(0), 200, name="n = 0"))
    out.append(case(c, rng.normal(size=300), np.zeros(300), 200, name="normal rows only"))
    out.append(case(c, rng.normal(size=300), np.ones(300), 200, name="abnormal rows only"))
    out.append(case(c, rng.normal(size=300), y0[:300], -1, name="j = -1"))
    out.append(case(np.zeros(0), rng.normal(size=300), y0[:300], calibration_rank(0, 0.95), name="n_c = 0"))
    return out


CASES = make_cases()


def run_engine(engine, cases, device="cpu"):
    """One detect_metrics call per (dtype, filter, scale, value) group; [8, len(cases)]."""
    out = np.full((8, len(cases)), np.nan)
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c["calib"].dtype.str, c["calib_labels"] is not None, c["scale"], c["value"]), []).append(i)
    for (_, filt, scale, value), idx in groups.items():
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
        sel = [cases[i] for i in idx]
        res = engine.detect_metrics([t(c["calib"]) for c in sel], [t(c["scores"]) for c in sel],
                                    [t(c["labels"]) for c in sel], [c["j"] for c in sel],
                                    calib_labels=[t(c["calib_labels"]) for c in sel] if filt else None,
                                    score_scale=scale, value=value)
        out[:, idx] = res
    return out


def oracle_all(cases):
    return np.stack([oracle(c["calib"], c["scores"], c["labels"], c["j"], c["calib_labels"], c["scale"], c["value"])
                     for c in cases], axis=1)


@pytest.fixture(scope="module")
def expected():
    want = oracle_all(CASES)
    want.setflags(write=False)
    return want


# ---------------------------------------------------------------------------
def test_calibration_rank():
    assert calibration_rank(0, 0.95) == -1
    assert calibration_rank(170, 0.95) == 161
    for n in (1, 2, 17, 170, 1000):
        assert calibration_rank(n, 1.0) == n - 1
        assert calibration_rank(n, 1e-12) == 0
        for q in (0.5, 0.9, 0.95, 0.99):
            j = calibration_rank(n, q)
            assert j == min(n - 1, max(0, math.ceil(q * n) - 1)) and 0 <= j < n


def test_torch_engine_matches_oracle(expected):
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine

    got = run_engine(TorchEngine(), CASES)
    for i, c in enumerate(CASES):
        assert_same_bits(got[:, i], expected[:, i], c["name"])


def test_case_list_covers_what_it_claims(expected):
    """The list holds thresholds of both signs and a zero reported as +0.0,
    undefined and defined cases, and test scores equal to the threshold."""
    tau = expected[1]
    assert (tau < 0).any() and (tau > 0).any() and np.isnan(tau).any()
    zero = tau == 0.0
    assert zero.any() and not np.signbit(tau[zero]).any()
    assert np.isnan(expected[0]).any() and (expected[0] > 0).any()
    assert any(np.any(clean(c["scores"], c["scale"]) == expected[1, i]) for i, c in enumerate(CASES))


def test_flags_at_most_the_calibration_tail():
    """scores = calib, all labels 0: at most n_c - 1 - j rows lie strictly above the j-th smallest."""
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine

    rng = np.random.default_rng(3)
    cases = []
    for n_c in (1, 2, 170, 1025):
        for c in (rng.normal(size=n_c), np.round(rng.normal(size=n_c), 1), np.full(n_c, 2.0)):
            for j in sorted({0, n_c - 1, calibration_rank(n_c, 0.95), n_c // 2}):
                cases.append(case(c, c, np.zeros(n_c), j))
    got = run_engine(TorchEngine(), cases)
    for i, c in enumerate(cases):
        assert got[3, i] <= c["calib"].size - 1 - c["j"], (c["calib"].size, c["j"], got[:, i])
        assert got[2, i] == 0 and got[3, i] + got[5, i] == c["calib"].size


def _small(orig):
    def resolved(self):
        s = orig(self)
        s.normal_rows, s.abnormal_rows, s.test_normal_rows = (60, 70), (80, 90), 15
        return s
    return resolved


def _shrink_worker():
    """Small clients, in a spawned worker process (nothing to restore there)."""
    from fedmse_decentralized_amd.data import synthetic

    synthetic.SyntheticSpec.resolved = _small(synthetic.SyntheticSpec.resolved)


@pytest.fixture
def shrunk(monkeypatch):
    """Small clients for this test only: the class is restored afterwards, and
    so is the prepared-data cache, which holds data of the patched sizes."""
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    monkeypatch.setattr(synthetic.SyntheticSpec, "resolved", _small(synthetic.SyntheticSpec.resolved))
    federation._PREP_CACHE.clear()
    yield
    federation._PREP_CACHE.clear()


def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=4, num_rounds=2, epoch=1, batch_size=12, output_root=out,
                backend="torch", device="cpu", log_level="WARNING", global_early_stop=False, save_checkpoints=False,
                compat="fixed", metric="detection")
    base.update(kw)
    return ExperimentConfig(**base)


def _detection_json(rs):
    return [{k: [None if v != v else v for v in r.detection[k].tolist()] for k in DETECT_FIELDS} for r in rs]


@pytest.mark.parametrize("model_type", ["hybrid", "autoencoder"])
@pytest.mark.parametrize("metric", ["detection", "tpr_at_fpr"])
def test_evaluate_clients_both_metrics(tmp_path, shrunk, metric, model_type):
    """A small synthetic federation: the metric is F1 / recall at a threshold
    that is one of the calibration scores, the counts add up to the test set,
    and the federation's round reports the same values."""
    from fedmse_decentralized_amd.eval.evaluator import evaluate_clients
    from fedmse_decentralized_amd.federation import Federation

    fed = Federation(_cfg(str(tmp_path), metric=metric, detect_quantile=0.9, target_fpr=0.1), model_type, "avg",
                     0).setup()
    r = fed.run_round()
    fed.finish()
    fed.writer.flush()
    eng, st = fed.engine, fed.engine.store
    er = evaluate_clients(eng, list(range(fed.N)), model_type, metric)
    assert set(DETECT_FIELDS) <= set(er.extra) and r.detection is not None
    for k in DETECT_FIELDS:
        assert_same_bits(r.detection[k], er.extra[k], k)
    assert_same_bits(r.metrics, er.metrics, "metric")
    assert_same_bits(er.metrics, er.extra["f1" if metric == "detection" else "recall"], "value")
    for c in range(fed.N):
        y = st.labels(c)
        assert er.extra["tp"][c] + er.extra["fn"][c] == np.sum(y != 0)
        assert er.extra["fp"][c] + er.extra["tn"][c] == np.sum(y == 0)
        n0 = int(np.sum(y == 0))
        if metric == "tpr_at_fpr":   # at most the target share of the normal rows is flagged
            assert er.extra["fp"][c] <= n0 - 1 - calibration_rank(n0, 0.9)
        assert er.extra["fpr"][c] == er.extra["fp"][c] / n0
        assert np.isfinite(er.extra["threshold"][c]) and 0.0 <= er.metrics[c] <= 1.0
    # the results file carries the value, the detection file everything
    import glob

    (res,) = glob.glob(os.path.join(str(tmp_path), "**", f"*_{model_type}_avg_results.json"), recursive=True)
    assert os.path.basename(os.path.dirname(res)) == metric
    line = json.loads(open(res).read().splitlines()[0])
    assert line["client_metrics"] == r.metrics.tolist()
    (det,) = glob.glob(os.path.join(os.path.dirname(res), "*_detection.jsonl"))
    d = json.loads(open(det).read().splitlines()[0])
    assert d["round"] == 1 and d["threshold"] == r.detection["threshold"].tolist()
    assert d["tp"] == [int(v) for v in r.detection["tp"]]


def test_other_metrics_report_no_detection(tmp_path, shrunk):
    from fedmse_decentralized_amd.federation import Federation

    fed = Federation(_cfg(str(tmp_path), metric="AUC"), "hybrid", "avg", 0, write_reports=False).setup()
    assert fed.run_round().detection is None


def test_config_ranges():
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ExperimentConfig(detect_quantile=bad)
    for bad in (1.0, -0.01, 2.0):
        with pytest.raises(ValueError):
            ExperimentConfig(target_fpr=bad)
    ExperimentConfig(detect_quantile=1.0, target_fpr=0.0)
    import argparse

    from fedmse_decentralized_amd.config import add_arguments, from_args

    ns = add_arguments(argparse.ArgumentParser()).parse_args(["--metric", "tpr_at_fpr", "--target-fpr", "0.05",
                                                              "--detect-quantile", "0.99"])
    cfg = from_args(ns)
    assert (cfg.metric, cfg.target_fpr, cfg.detect_quantile) == ("tpr_at_fpr", 0.05, 0.99)
    with pytest.raises(ValueError):
        from_args(add_arguments(argparse.ArgumentParser()).parse_args(["--target-fpr", "1"]))


def test_detection_line_round_trips(tmp_path):
    from fedmse_decentralized_amd.io import reports

    rows = np.array([[0.8, np.nan, np.nan], [1.25, 0.0, np.nan], [4, 0, 0], [1, 0, 0], [1, 3, 0], [9, 0, 5],
                     [0.8, np.nan, np.nan], [0.8, np.nan, np.nan]], dtype=np.float64)
    det = detection_fields(rows)
    assert det["f1"][0] == 2 * 4 / (2 * 4 + 1 + 1) and det["fpr"][0] == 1 / 10
    assert np.isnan(det["f1"][1:]).all() and np.isnan(det["fpr"][1:]).all()
    cfg = _cfg(str(tmp_path))
    path = reports.append_detection_result(cfg, 0, 4, det, "hybrid", "mse_avg")
    assert path.endswith("_hybrid_mse_avg_detection.jsonl")
    assert os.path.dirname(path) == os.path.dirname(reports.results_path(cfg, 0, "hybrid", "mse_avg"))
    reports.append_detection_result(cfg, 0, 5, det, "hybrid", "mse_avg")
    lines = [json.loads(ln) for ln in open(path).read().splitlines()]
    assert [ln["round"] for ln in lines] == [5, 6] and lines[0]["metric"] == "detection"
    d = lines[0]
    assert d["threshold"] == [1.25, 0.0, None] and d["tp"] == [4, 0, 0] and d["tn"] == [9, 0, 5]
    assert d["precision"] == [0.8, None, None] and d["f1"] == [det["f1"][0], None, None]
    for k in DETECT_FIELDS:
        back = np.array([np.nan if v is None else v for v in d[k]], dtype=np.float64)
        assert_same_bits(back, det[k], k)


# ---------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out, metric):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    _shrink_worker()
    from fedmse_decentralized_amd.federation import Federation
    from fedmse_decentralized_amd.parallel.launch import init_comm, shutdown

    comm = init_comm(backend="gloo", device="cpu")
    fed = Federation(_cfg(out, metric=metric), "hybrid", "mse_avg", 0, comm=comm).setup()
    rs = [fed.run_round() for _ in range(2)]
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"metrics": [r.metrics.tolist() for r in rs], "detection": _detection_json(rs)}, f)
    shutdown(comm)


@pytest.mark.timeout(300)
def test_gloo_two_ranks_report_the_same_detection(tmp_path):
    """The single-process run is a worker too (a group of one rank takes the
    loopback path): a threshold is a score's own bits, so both runs must
    compute under the same conditions -- a fresh process with one torch
    thread -- where the rank-based AUC would forgive a last-bit difference."""
    out, single = str(tmp_path), str(tmp_path / "single")
    os.makedirs(single)
    mp.start_processes(_worker, args=(2, _free_port(), out, "detection"), nprocs=2, join=True, start_method="spawn")
    mp.start_processes(_worker, args=(1, _free_port(), single, "detection"), nprocs=1, join=True,
                       start_method="spawn")
    want = json.load(open(os.path.join(single, "rank0.json")))
    assert len(want["detection"]) == 2 and set(want["detection"][-1]) == set(DETECT_FIELDS)
    assert all(v is not None for v in want["detection"][-1]["threshold"])
    for r in range(2):
        d = json.load(open(os.path.join(out, f"rank{r}.json")))
        assert d["detection"] == want["detection"]
        assert d["metrics"] == want["metrics"]
