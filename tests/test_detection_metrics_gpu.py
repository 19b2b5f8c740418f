"""``detect_kernel`` (fedmx_detect.hip) on the GPU against the numpy oracle of
tests/test_detection_metrics.py, bit for bit on all 8 output rows, and the
two calibrated-threshold metrics through the engines, the device-resident
round, the host-decision round and two gloo ranks sharing the GPU."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.config import ExperimentConfig
from fedmse_decentralized_amd.eval.metrics import DETECT_FIELDS
from test_detection_metrics import CASES, assert_same_bits, case, oracle_all, run_engine
from test_device_protocol_gpu import _shrink

SENTINEL = -7.0


@pytest.fixture(scope="module")
def expected():
    want = oracle_all(CASES)
    want.setflags(write=False)
    return want


def run_kernel(cases, extra_columns=0):
    """Every group of cases that shares (dtype, filter, scale, value) in one
    launch (clients of unequal sizes side by side), into a sentinel-filled
    [8, k + extra_columns] device tensor.  Returns ([8, len(cases)], launches)."""
    from fedmse_decentralized_amd.ops import _hip

    dev = torch.device("cuda", 0)
    rt = _hip.runtime(dev)
    out = np.full((8, len(cases)), np.nan)
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c["calib"].dtype.str, c["calib_labels"] is not None, c["scale"], c["value"]), []).append(i)
    for (_, filt, scale, value), idx in groups.items():
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        sel = [cases[i] for i in idx]
        k = len(sel)
        res = torch.full((8, k + extra_columns), SENTINEL, dtype=torch.float64, device=dev)
        keep = [[t(c["calib"]) for c in sel], [t(c["scores"]) for c in sel], [t(c["labels"]) for c in sel],
                [t(c["calib_labels"]) for c in sel] if filt else None]
        desc = _hip.detect_desc(keep[0], keep[1], keep[2], [c["j"] for c in sel], res.data_ptr(), k + extra_columns,
                                calib_labels=keep[3], f32_scale=scale, value_is_recall=value == "recall")
        (dptr,) = rt.desc.put(desc)
        _hip._check(_hip.lib().fedmx_detect(dptr, k, rt.stream), "fedmx_detect")
        rt.sync()
        host = res.cpu().numpy()
        assert np.all(host[:, k:] == SENTINEL), "columns beyond the launch's clients were written"
        assert not np.any(host[:, :k] == SENTINEL), "an output was left unwritten"
        out[:, idx] = host[:, :k]
    return out, len(groups)


def test_kernel_matches_oracle(expected):
    got, launches = run_kernel(CASES, extra_columns=3)
    assert launches <= 6   # the whole list in a handful of launches of many unequal clients
    for i, c in enumerate(CASES):
        assert_same_bits(got[:, i], expected[:, i], c["name"])


def test_kernel_single_client_launches(expected):
    """One client per launch (grid of 1) for a few cases of each kind."""
    pick = list(range(0, len(CASES), 9))
    for i in pick:
        got, _ = run_kernel([CASES[i]])
        assert_same_bits(got[:, 0], expected[:, i], CASES[i]["name"])


def test_descriptor_checks():
    from fedmse_decentralized_amd.ops import _hip

    dev = torch.device("cuda", 0)
    c = torch.zeros(5, dtype=torch.float64, device=dev)
    y = torch.zeros(5, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        _hip.detect_desc([c], [c], [y], [5], 0, 1)            # rank beyond the calibration values
    with pytest.raises(ValueError):
        _hip.detect_desc([c.float()], [c], [y], [0], 0, 1)    # mixed dtypes
    with pytest.raises(ValueError):
        _hip.detect_desc([c], [c], [y.long()], [0], 0, 1)     # labels must be int32
    with pytest.raises(ValueError):
        _hip.detect_desc([c, c], [c, c], [y, y], [0, 0], 0, 1)   # stride below the item count


def test_hip_engine_matches_torch_engine(expected):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
    from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS

    hip = run_engine(HipEngine(DEFAULT_DIMS, torch.device("cuda", 0)), CASES, device="cuda:0")
    ref = run_engine(TorchEngine(), CASES)
    assert_same_bits(hip, ref, "HipEngine vs TorchEngine")
    assert_same_bits(hip, expected, "HipEngine vs oracle")


def test_large_calibration_set_needs_no_host_path():
    """n_c = 10,000 calibration values and 100,000 test rows in one client:
    beyond any LDS-resident sort, still exact."""
    rng = np.random.default_rng(77)
    c = rng.gamma(2.0, 2.0, size=10_000)
    s = np.r_[rng.gamma(2.0, 2.0, size=40_000), rng.gamma(4.0, 3.0, size=60_000)]
    y = np.r_[np.zeros(40_000), np.ones(60_000)]
    cases = [case(c, s, y, 9499), case(s, s, y, 39_599, calib_labels=y, value="recall")]
    got, _ = run_kernel(cases)
    assert_same_bits(got, oracle_all(cases), "large")


# ---------------------------------------------------------------------------
def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=6, num_rounds=3, epoch=2, batch_size=12, output_root=out,
                backend="hip", device="cuda", log_level="WARNING", compat="fixed", global_early_stop=False,
                save_checkpoints=False, metric="detection")
    base.update(kw)
    return ExperimentConfig(**base)


def _run(cfg, model_type, update_type, rounds, comm=None):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.federation import Federation

    federation._PREP_CACHE.clear()
    fed = Federation(cfg, model_type, update_type, 0, comm=comm).setup()
    rs = [fed.run_round() for _ in range(rounds)]
    fed.finish()
    fed.writer.flush()
    out = dict(agg=[r.aggregator for r in rs], metrics=[r.metrics for r in rs], det=[r.detection for r in rs])
    torch.cuda.synchronize()
    return fed, out


def _same_detection(a, b, what):
    assert len(a) == len(b)
    for rnd, (x, y) in enumerate(zip(a, b)):
        assert x is not None and y is not None and set(x) == set(DETECT_FIELDS) == set(y)
        for k in DETECT_FIELDS:
            assert_same_bits(x[k], y[k], f"{what} round {rnd + 1} {k}")


@pytest.mark.parametrize("model_type", ["hybrid", "autoencoder"])
@pytest.mark.parametrize("metric", ["detection", "tpr_at_fpr"])
def test_device_round_matches_host_round_and_evaluate(tmp_path, metric, model_type):
    _shrink()
    fa, a = _run(_cfg(str(tmp_path / "dev"), metric=metric, device_protocol=True), model_type, "mse_avg", 3)
    fb, b = _run(_cfg(str(tmp_path / "host"), metric=metric, device_protocol=False), model_type, "mse_avg", 3)
    assert fa._fast is not None and fb._fast is None
    assert a["agg"] == b["agg"]
    _same_detection(a["det"], b["det"], "device vs host")
    value = "f1" if metric == "detection" else "recall"
    for x, y, d in zip(a["metrics"], b["metrics"], a["det"]):
        assert_same_bits(x, y, "metric")
        assert_same_bits(x, d[value], "metric is the detection's value")
    assert torch.equal(fa.engine.store.params, fb.engine.store.params)
    # thresholds are real scores, the counts cover each client's test set
    st = fa.engine.store
    last = a["det"][-1]
    for c in range(fa.N):
        y = st.labels(c)
        assert last["tp"][c] + last["fn"][c] == np.sum(y != 0) and last["fp"][c] + last["tn"][c] == np.sum(y == 0)
    assert np.isfinite(last["threshold"]).all() and np.isfinite(a["metrics"][-1]).all()
    # the final round's evaluation, run again through HipEngine.evaluate on the live parameters
    er = fa.engine.evaluate(model_type, metric)
    assert_same_bits(er.metrics, a["metrics"][-1], "evaluate() metric")
    for k in DETECT_FIELDS:
        assert_same_bits(er.extra[k], last[k], f"evaluate() extra {k}")
    # identical detection report lines
    import glob

    (pa,) = glob.glob(os.path.join(str(tmp_path / "dev"), "**", "*_detection.jsonl"), recursive=True)
    pb = pa.replace(str(tmp_path / "dev"), str(tmp_path / "host"))
    assert open(pa).read() == open(pb).read() and len(open(pa).read().splitlines()) == 3


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _json(det):
    return [{k: [None if v != v else v for v in d[k].tolist()] for k in DETECT_FIELDS} for d in det]


def _worker(rank, world, port, out, metric, model_type):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), FEDMX_DEVICE_INDEX="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    _shrink()
    from fedmse_decentralized_amd.parallel.launch import init_comm, shutdown

    comm = init_comm(backend="gloo", device="cuda")
    fed, res = _run(_cfg(os.path.join(out, f"r{rank}"), metric=metric, debug_replica_check=True), model_type,
                    "mse_avg", 3, comm=comm)
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"fast": fed._fast is not None, "agg": res["agg"], "metrics": [m.tolist() for m in res["metrics"]],
                   "det": _json(res["det"])}, f)
    shutdown(comm)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("metric,model_type", [("detection", "hybrid"), ("tpr_at_fpr", "autoencoder")])
def test_two_ranks_one_gpu_report_the_same_detection(tmp_path, metric, model_type):
    out = str(tmp_path)
    mp.start_processes(_worker, args=(2, _port(), out, metric, model_type), nprocs=2, join=True,
                       start_method="spawn")
    _shrink()
    fed, ref = _run(_cfg(os.path.join(out, "single"), metric=metric), model_type, "mse_avg", 3)
    assert fed._fast is not None
    want = _json(ref["det"])
    for r in range(2):
        d = json.load(open(os.path.join(out, f"rank{r}.json")))
        assert d["fast"] and d["agg"] == ref["agg"]
        assert d["det"] == want
        assert d["metrics"] == [m.tolist() for m in ref["metrics"]]


def test_poisoned_run_reports_detection(tmp_path):
    """Client 2 poisons its update (x 25) under trimmed_mean: every round's
    detection is populated, and finite for the clients whose test set holds
    both classes.  No quality bar."""
    _shrink()
    fed, a = _run(_cfg(str(tmp_path), malicious_clients=[2], malicious_scale=25.0, num_participants=1.0),
                  "hybrid", "trimmed_mean", 3)
    assert fed._fast is not None
    st = fed.engine.store
    both = [c for c in range(fed.N) if 0 < np.sum(st.labels(c) != 0) < st.labels(c).size]
    assert both
    for d in a["det"]:
        assert d is not None and set(d) == set(DETECT_FIELDS)
        for k in DETECT_FIELDS:
            assert d[k].shape == (fed.N,) and np.isfinite(d[k][both]).all(), k
