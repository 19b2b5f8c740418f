"""``knn_score_kernel`` (fedmx_knn.hip) on the GPU against ``knn_score_numpy``
on the inputs of tests/test_knn_scorer.py (whose sensitivity test shows they
sit on no rounding boundary), and ``latent_scorer="knn"`` through the engines,
the cached evaluation plans, the device-resident round and the host round."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.config import ExperimentConfig
from fedmse_decentralized_amd.engine.torch_engine import knn_score_numpy
from test_detection_metrics import assert_same_bits
from test_device_protocol_gpu import _shrink
from test_knn_scorer import GPU_TOL, gpu_cases, latents, mixed_launch

DEV = torch.device("cuda", 0)
SENTINEL = -7.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strided(a):
    """[n, Z] view with row stride 16 over a [n, 16] buffer whose other columns hold NaN."""
    buf = torch.full((a.shape[0], 16), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = _t(a)
    return buf[:, :a.shape[1]]


def run_launch(pairs, latent, k, strided=False, launch_k=None):
    """One launch over (train, query) pairs into a sentinel-padded output."""
    from fedmse_decentralized_amd.ops import _hip

    rt = _hip.runtime(DEV)
    wrap = _strided if strided else _t
    tr = [wrap(a) for a, _ in pairs]
    qu = [wrap(b) for _, b in pairs]
    total = sum(int(q.shape[0]) for q in qu)
    out = torch.full((total + 5,), SENTINEL, dtype=torch.float64, device=DEV)
    desc, views = _hip.knn_desc(tr, qu, out, latent, k)
    (dptr,) = rt.desc.put(desc)
    _hip._check(_hip.lib().fedmx_knn_score(dptr, len(desc), k if launch_k is None else launch_k,
                                           _hip.knn_grid_y(qu), rt.stream), "fedmx_knn_score")
    rt.sync()
    host = out.cpu().numpy()
    assert np.all(host[total:] == SENTINEL), "slots beyond the launch's query rows were written"
    assert not np.any(host[:total] == SENTINEL), "a score was left unwritten"
    return [v.cpu().numpy() for v in views]


@pytest.fixture(scope="module")
def T():
    from fedmse_decentralized_amd.ops import _hip

    return _hip.knn_tile_rows()


@pytest.fixture(scope="module")
def cases(T):
    out = []
    for name, tr, qu, k in gpu_cases(T):
        want = knn_score_numpy(tr, qu, k)
        want.setflags(write=False)
        out.append((name, tr, qu, k, want))
    return out


@pytest.mark.parametrize("i", range(10))
def test_kernel_matches_oracle(cases, i):
    name, tr, qu, k, want = cases[i]
    (got,) = run_launch([(tr, qu)], tr.shape[1], k)
    err = np.max(np.abs(got - want) / (1.0 + np.abs(want)))
    print(f"{name}: max |got - want| / (1 + |want|) = {err:.3e}")
    np.testing.assert_allclose(got, want, rtol=GPU_TOL, atol=GPU_TOL, err_msg=name)


@pytest.mark.parametrize("strided", [False, True])
def test_mixed_descriptors_in_one_launch(T, strided):
    pairs = mixed_launch(T)
    got = run_launch(pairs, 7, 5, strided=strided)
    for i, ((tr, qu), g) in enumerate(zip(pairs, got)):
        np.testing.assert_allclose(g, knn_score_numpy(tr, qu, 5), rtol=GPU_TOL, atol=GPU_TOL, err_msg=f"item {i}")
    # a launch whose list capacity is above the descriptors' k scores them at their own k
    wide = run_launch(pairs, 7, 5, strided=strided, launch_k=16)
    for g, w in zip(got, wide):
        assert_same_bits(w, g, "launch capacity 16, k = 5")


def test_duplicates_and_exact_hits():
    rng = np.random.default_rng(7300)
    base = latents(rng, 30, 7)
    train = np.repeat(base, 20, axis=0)[rng.permutation(600)]
    query = np.concatenate([base[:10], latents(rng, 200, 7, 1.5)])
    (got,) = run_launch([(train, query)], 7, 16)
    # the 16 nearest of a train row's copy are among its 20 copies
    assert np.all(got[:10] == 0.0)
    np.testing.assert_allclose(got, knn_score_numpy(train, query, 16), rtol=GPU_TOL, atol=GPU_TOL)
    (hit,) = run_launch([(train, query)], 7, 1)
    assert np.all(hit[:10] == 0.0) and np.all(hit[10:] > 0.0)
    np.testing.assert_allclose(hit, knn_score_numpy(train, query, 1), rtol=GPU_TOL, atol=GPU_TOL)


def test_non_finite_queries_score_inf():
    rng = np.random.default_rng(7400)
    train, query = latents(rng, 500, 7), latents(rng, 300, 7, 1.5)
    clean = run_launch([(train, query), (train[:50], query[:40])], 7, 5)
    bad = query.copy()
    bad[3, 2] = np.nan
    bad[77, 0] = np.inf
    bad[299, 6] = -np.inf
    got = run_launch([(train, bad), (train[:50], query[:40])], 7, 5)
    rows = [3, 77, 299]
    assert np.all(got[0][rows] == np.inf)
    keep = np.setdiff1d(np.arange(300), rows)
    assert_same_bits(got[0][keep], clean[0][keep], "rows beside the non-finite ones")
    assert_same_bits(got[1], clean[1], "the launch's other descriptor")
    np.testing.assert_array_equal(got[0][rows], knn_score_numpy(train, bad, 5)[rows])


def test_binding_checks():
    from fedmse_decentralized_amd.ops import _hip

    x = torch.zeros(4, 7, dtype=torch.float32, device=DEV)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        _hip.knn_desc([x[:0]], [x], out, 7, 5)          # no train rows
    for k in (0, 17):
        with pytest.raises(ValueError):
            _hip.knn_desc([x], [x], out, 7, k)
    with pytest.raises(ValueError):
        _hip.knn_desc([x.double()], [x], out, 7, 5)
    with pytest.raises(ValueError):
        _hip.knn_desc([x], [x], out[:3], 7, 5)          # more query rows than output slots
    assert _hip.lib().fedmx_knn_desc_size() == _hip.KNN_DTYPE.itemsize
    assert _hip.lib().fedmx_knn_max_k() == _hip.KNN_MAX_K == 16


def test_hip_engine_matches_torch_engine(cases):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
    from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS

    hip, ref = HipEngine(DEFAULT_DIMS, DEV), TorchEngine()
    sel = [c for c in cases if c[1].shape[1] == DEFAULT_DIMS.latent and c[3] == 16]
    assert len(sel) >= 2
    got = hip.knn_scores([_t(c[1]) for c in sel], [_t(c[2]) for c in sel], 16)
    want = ref.knn_scores([torch.from_numpy(c[1]) for c in sel], [torch.from_numpy(c[2]) for c in sel], 16)
    hip.synchronize()
    for g, w, c in zip(got, want, sel):
        np.testing.assert_allclose(g.cpu().numpy(), w.numpy(), rtol=GPU_TOL, atol=GPU_TOL, err_msg=c[0])
        np.testing.assert_array_equal(w.numpy(), c[4])


# ---------------------------------------------------------------------------
def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=6, num_rounds=3, epoch=2, batch_size=12, output_root=out,
                backend="hip", device="cuda", log_level="WARNING", compat="fixed", global_early_stop=False,
                save_checkpoints=False)
    base.update(kw)
    return ExperimentConfig(**base)


def _run(cfg, rounds=3):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.federation import Federation

    federation._PREP_CACHE.clear()
    fed = Federation(cfg, "hybrid", "mse_avg", 0).setup()
    rs = [fed.run_round() for _ in range(rounds)]
    fed.finish()
    fed.writer.flush()
    out = dict(agg=[r.aggregator for r in rs], metrics=[r.metrics for r in rs], det=[r.detection for r in rs])
    torch.cuda.synchronize()
    return fed, out


def _same(a, b, what):
    assert a["agg"] == b["agg"], what
    for rnd, (x, y) in enumerate(zip(a["metrics"], b["metrics"])):
        assert_same_bits(x, y, f"{what} round {rnd + 1} metric")
    for rnd, (x, y) in enumerate(zip(a["det"], b["det"])):
        assert (x is None) == (y is None)
        if x is not None:
            assert set(x) == set(y)
            for k in x:
                assert_same_bits(x[k], y[k], f"{what} round {rnd + 1} {k}")


@pytest.mark.parametrize("metric", ["AUC", "detection"])
def test_device_round_matches_host_round_and_evaluate(tmp_path, metric):
    _shrink()
    kw = dict(metric=metric, latent_scorer="knn", knn_k=5)
    fa, a = _run(_cfg(str(tmp_path / "dev"), device_protocol=True, **kw))
    fb, b = _run(_cfg(str(tmp_path / "host"), device_protocol=False, **kw))
    assert fa._fast is not None and fb._fast is None
    _same(a, b, "device vs host")
    assert torch.equal(fa.engine.store.params, fb.engine.store.params)
    assert np.isfinite(a["metrics"][-1]).all()
    # the final round's evaluation, run again through HipEngine.evaluate on the live parameters
    er = fa.engine.evaluate("hybrid", metric)
    assert_same_bits(er.metrics, a["metrics"][-1], "evaluate() metric")
    if metric == "detection":
        for k, v in a["det"][-1].items():
            assert_same_bits(er.extra[k], v, f"evaluate() extra {k}")
    # the scores behind it are the kNN oracle's on the device's own latents
    eng, st = fa.engine, fa.engine.store
    p = eng._plan("hybrid", metric=metric)
    lat = p["fwd"].lat_views()
    m = 3 if metric == "detection" else 2
    for c in range(fa.N):
        want = knn_score_numpy(lat[m * c].cpu().numpy(), lat[m * c + 1].cpu().numpy(), 5)
        np.testing.assert_allclose(p["scores"][c].cpu().numpy(), want, rtol=GPU_TOL, atol=GPU_TOL)
    # and the centroid scorer's plan holds other scores for the same parameters
    eng.latent_scorer = "cen"
    eng.evaluate("hybrid", metric)
    q = eng._plan("hybrid", metric=metric)
    assert q is not p and not torch.equal(q["scores"][0], p["scores"][0])


@pytest.mark.parametrize("metric", ["AUC", "detection"])
def test_cen_run_equals_a_run_that_never_names_the_option(tmp_path, metric):
    _shrink()
    _, a = _run(_cfg(str(tmp_path / "named"), metric=metric, latent_scorer="cen", knn_k=9))
    _, b = _run(_cfg(str(tmp_path / "plain"), metric=metric))
    _same(a, b, "latent_scorer=cen vs default")


def test_plans_are_keyed_by_scorer_and_k(tmp_path):
    _shrink()
    fed, _ = _run(_cfg(str(tmp_path), metric="AUC"), rounds=1)
    eng = fed.engine
    plans, vals = {}, {}
    for key in (("cen", 5), ("knn", 1), ("knn", 5)):
        eng.latent_scorer, eng.knn_k = key
        plans[key] = eng._plan("hybrid")
        assert eng._plan("hybrid") is plans[key]
    assert len({id(p) for p in plans.values()}) == 3
    eng.latent_scorer, eng.knn_k = "cen", 9            # k is no part of the centroid scorer's plan
    assert eng._plan("hybrid") is plans[("cen", 5)]
    assert eng._plan("autoencoder") is not None
    eng.latent_scorer = "knn"
    assert eng._plan("autoencoder") is eng._plan("autoencoder")
    for rep in range(2):                               # one after the other, twice: each keeps its own results
        for key in plans:
            eng.latent_scorer, eng.knn_k = key
            got = eng.evaluate("hybrid", "AUC").metrics
            if rep == 0:
                vals[key] = got
            else:
                assert_same_bits(got, vals[key], str(key))
    assert not torch.equal(plans[("cen", 5)]["scores"][0], plans[("knn", 5)]["scores"][0])
    assert not torch.equal(plans[("knn", 1)]["scores"][0], plans[("knn", 5)]["scores"][0])
    st = eng.store
    for key in (("knn", 1), ("knn", 5)):
        lat = plans[key]["fwd"].lat_views()
        for c in range(fed.N):
            want = knn_score_numpy(lat[2 * c].cpu().numpy(), lat[2 * c + 1].cpu().numpy(), key[1])
            np.testing.assert_allclose(plans[key]["scores"][c].cpu().numpy(), want, rtol=GPU_TOL, atol=GPU_TOL)
    assert st.num_clients == fed.N
