"""The multi-workgroup AUC path (fedmx_auc_large.hip) on the GPU: equal to the
host library's AUC of the read scores to the bit, from the raw binding up to
the engine's plan and the device-resident round, with the host AUC made to
raise wherever the device has to answer alone."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.config import ExperimentConfig
from fedmse_decentralized_amd.eval.metrics import read_scores
from fedmse_decentralized_amd.models.layout import ModelDims
from fedmse_decentralized_amd.ops import _hip, _host

from test_auc_large import CASES, WANT

DEV = torch.device("cuda")


def _dev(s, y):
    return torch.from_numpy(np.ascontiguousarray(s)).to(DEV), torch.from_numpy(np.asarray(y).astype(np.int32)).to(DEV)


def _same(got, want):
    return (np.isnan(got) and np.isnan(want)) or got == want


def _tied(small, small_is_positive, extra=9):
    """test_auc_at_the_lds_sort_limit's construction."""
    rng = np.random.default_rng(small)
    y = np.r_[np.full(small, int(small_is_positive)), np.full(small + extra, int(not small_is_positive))]
    rng.shuffle(y)
    return np.round(rng.normal(size=len(y)) + 0.3 * y, 2), y


def _engine():
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    return HipEngine(ModelDims(115, 27, 7), DEV)


def _raise(*a, **k):
    raise AssertionError("the host AUC must not be called")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_raw_path_many_chunks(dtype):
    """The CPU grid at 64 keys a chunk, all pairs in one launch; float32 scores
    are the grid's rounded to float32 (read with the case's scale)."""
    cases = [(name, s.astype(dtype) if s.dtype == np.float64 else s, y, scale) for name, s, y, scale in CASES]
    cases += [("single-class", np.arange(9, dtype=dtype), np.ones(9, np.int64), 1.0),
              ("no-rows", np.zeros(0, dtype=dtype), np.zeros(0, np.int64), 1.0)]
    for scale in sorted({c[3] for c in cases}):
        sub = [c for c in cases if c[3] == scale]
        pairs = [_dev(s, y) for _, s, y, _ in sub]
        view = _hip.auc_large([p[0] for p in pairs], [p[1] for p in pairs], scale, chunk_keys=64)
        _hip.runtime(DEV).sync()
        for (name, s, y, _), got in zip(sub, np.array(view)):
            want = WANT[name] if (name in WANT and s.dtype == np.float64) else _host.roc_auc(read_scores(s, scale), y)
            assert _same(got, want), (name, got, want)
            if name in ("single-class", "no-rows"):
                assert np.isnan(got)


@pytest.mark.parametrize("small", [8193, 16384, 16385])
def test_raw_path_beyond_the_lds_sort(small):
    pairs, want = [], []
    for small_is_positive in (True, False):
        s, y = _tied(small, small_is_positive)
        for dtype in (np.float64, np.float32):
            pairs.append(_dev(s.astype(dtype), y))
            want.append(_host.roc_auc(read_scores(s.astype(dtype)), y))
    view = _hip.auc_large([p[0] for p in pairs], [p[1] for p in pairs])
    _hip.runtime(DEV).sync()
    assert list(np.array(view)) == want


def test_mixed_descriptors_and_counter_reset():
    """Five pairs of mixed sizes in one call, each right on its own; the same
    descriptors and workspace launched again give the same bits (finalize
    re-zeroes the counters)."""
    rng = np.random.default_rng(5)
    y4 = np.r_[np.ones(20000, np.int64), np.zeros(300, np.int64)]
    rng.shuffle(y4)
    data = [_tied(5, True), _tied(8193, False), (rng.normal(size=40), np.zeros(40, np.int64)),
            (np.zeros(0), np.zeros(0, np.int64)), (np.round(rng.normal(size=20300) + 0.2 * y4, 1), y4)]
    pairs = [_dev(s, y) for s, y in data]
    want = [_host.roc_auc(read_scores(s), y) for s, y in data]
    assert np.isnan(want[2]) and np.isnan(want[3])
    rows = [len(y) for _, y in data]
    ws = torch.empty(sum(rows), dtype=torch.float64, device=DEV)
    ctr = torch.zeros(_hip.AUC_LARGE_CTR_WORDS * len(pairs), dtype=torch.int64, device=DEV)
    out = torch.full((len(pairs),), -7.0, dtype=torch.float64, device=DEV)
    desc = _hip.auc_large_desc([p[0] for p in pairs], [p[1] for p in pairs], out.data_ptr(), ws.data_ptr(),
                               ctr.data_ptr())
    blob = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    chunks, slices = _hip.auc_large_grid([min(int(y.sum()), int((y == 0).sum())) for _, y in data],
                                         [max(int(y.sum()), int((y == 0).sum())) for _, y in data])
    assert chunks == 2
    runs = []
    for _ in range(2):
        out.fill_(-7.0)
        _hip.launch_auc_large(blob, len(pairs), max(rows), chunks, slices, DEV)
        _hip.runtime(DEV).sync()
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
        assert int(ctr.abs().sum()) == 0
    for got, w in zip(runs[0], want):
        assert _same(got, w), (runs[0], want)
    assert runs[0].tobytes() == runs[1].tobytes()


def test_engine_auc_recomputes_on_the_device(monkeypatch):
    eng = _engine()
    s, y = _tied(8193, True)
    want = _host.roc_auc(s, y)
    st, yt = _dev(s, y)
    raw = _hip.auc([st], [yt])
    _hip.runtime(DEV).sync()
    assert float(raw[0]) == -1.0   # auc_kernel still gives up here
    monkeypatch.setattr(_host, "roc_auc", _raise)
    assert float(eng.auc([st], [yt])[0]) == want


def test_auc_large_refuses_more_than_2_pow_26_rows():
    n = (1 << 26) + 1
    s = torch.zeros(n, dtype=torch.float32, device=DEV)
    y = torch.zeros(n, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        _hip.auc_large([s], [y])


# ---------------------------------------------------------------------------
SMALL = dict(normal_rows=(150, 170), abnormal_rows=(200, 220), test_normal_rows=30)
LARGE = dict(normal_rows=(150, 170), abnormal_rows=(8400, 8420), test_normal_rows=8300)
BIG_CLIENT = 1


class _sizes:
    """Client BIG_CLIENT (when ``big``) with both test classes beyond 8,192
    rows, every other client shrunk as in tests/test_device_protocol_gpu.py."""

    def __init__(self, big=True):
        self.big = big

    def __enter__(self):
        from fedmse_decentralized_amd import federation
        from fedmse_decentralized_amd.data import synthetic

        self.fed, self.cls = federation, synthetic.SyntheticSpec
        self.saved_gen, self.saved_resolved = federation.generate_client, self.cls.resolved
        # (another test module may have shrunk every spec: explicit sizes need the original)
        self.cls.resolved = getattr(self.cls, "_fedmx_orig_resolved", self.saved_resolved)
        orig = self.saved_gen

        def gen(spec, client):
            return orig(dataclasses.replace(spec, **(LARGE if (self.big and client == BIG_CLIENT) else SMALL)), client)
        federation.generate_client = gen
        federation._PREP_CACHE.clear()
        return self

    def __exit__(self, *exc):
        self.fed.generate_client = self.saved_gen
        self.cls.resolved = self.saved_resolved
        self.fed._PREP_CACHE.clear()
        return False


def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=3, num_rounds=2, epoch=2, batch_size=12, output_root=out,
                backend="hip", device="cuda", log_level="WARNING", compat="fixed", global_early_stop=False,
                save_checkpoints=False, model_types=["hybrid"], update_types=["mse_avg"])
    base.update(kw)
    return ExperimentConfig(**base)


def _federation(cfg):
    from fedmse_decentralized_amd import federation

    federation._PREP_CACHE.clear()
    return federation.Federation(cfg, "hybrid", "mse_avg", 0).setup()


def test_plan_holds_the_large_clients_and_evaluates_without_the_host(tmp_path, monkeypatch):
    with _sizes(big=False):
        fed = _federation(_cfg(str(tmp_path / "small")))
        for model_type in ("hybrid", "autoencoder"):
            assert fed.engine._plan(model_type)["auc_large"] is None   # nothing added when no client is large
        fed.finish()
    with _sizes():
        fed = _federation(_cfg(str(tmp_path / "big")))
        eng, st = fed.engine, fed.engine.store
        big = [c for c in range(3) if min(int(st.labels(c).sum()), int((st.labels(c) == 0).sum())) > 8192]
        assert len(big) == 1
        for model_type in ("hybrid", "autoencoder"):
            p = eng._plan(model_type)
            assert p["auc_large"]["clients"] == big
            scale = p["auc_scale"]
            # the host value first: the scores this very evaluation leaves on the device
            eng.evaluate_launch(model_type)
            eng._rt.sync()
            scores = [s.detach().clone() for s in p["scores"]]
            want = [_host.roc_auc(read_scores(s.cpu().numpy(), scale), st.labels(c)) for c, s in enumerate(scores)]
            small = _hip.auc(scores, p["labels"], scale)
            _hip.runtime(DEV).sync()
            small = np.array(small)
            assert [c for c in range(3) if small[c] == -1.0] == big
            with monkeypatch.context() as mp:
                mp.setattr(_host, "roc_auc", _raise)
                got = eng.evaluate(model_type).metrics
            for c in range(3):
                assert got[c] == (want[c] if c in big else small[c]), (model_type, c, got, want, small)
                assert abs(got[c] - want[c]) < 1e-12
        fed.finish()


def test_device_round_reports_the_large_client_without_the_host(tmp_path, monkeypatch):
    def run(out, device_protocol):
        fed = _federation(_cfg(out, network_size=4, device_protocol=device_protocol))
        rs = [fed.run_round() for _ in range(2)]
        fed.finish()
        fed.writer.flush()
        torch.cuda.synchronize()
        return fed, [r.metrics.tolist() for r in rs]

    with _sizes():
        with monkeypatch.context() as mp:
            mp.setattr(_host, "roc_auc", _raise)
            fa, a = run(str(tmp_path / "dev"), True)
        fb, b = run(str(tmp_path / "host"), False)
    assert fa._fast is not None and fb._fast is None
    labs = [fa.engine.store.labels(c) for c in range(4)]
    assert sum(min(int(l.sum()), int((l == 0).sum())) > 8192 for l in labs) == 1
    assert a == b
    assert all(0.5 < m <= 1.0 for ms in a for m in ms)
