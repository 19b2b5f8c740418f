"""The nearest-neighbour latent scorer (README "Latent scorers") on the CPU:
``knn_score_numpy``, the oracle of ``knn_score_kernel``, against a brute-force
implementation and hand-worked cases, the construction where the centroid
scorer fails, the sensitivity of the GPU test's fixtures to the last bit of
the fitted scaler, and the option through the config and a TorchEngine
federation.  ``gpu_cases`` / ``mixed_launch`` are the inputs
tests/test_knn_scorer_gpu.py runs on the device."""
import numpy as np
import pytest

from fedmse_decentralized_amd.config import ExperimentConfig
from fedmse_decentralized_amd.data.scaler import StandardScaler
from fedmse_decentralized_amd.engine.torch_engine import cen_score_numpy, knn_score_numpy
from fedmse_decentralized_amd.ops import _host

# kernel against oracle (tests/test_knn_scorer_gpu.py): the project's own
# tolerance for cen_score_kernel (tests/test_kernels_gpu.py), whose scaler
# arithmetic the kNN kernel shares; a k-th order statistic moves no more than
# its inputs do
GPU_TOL = 1e-12


def brute_force(train, query, k):
    """Full float64 distance matrix, columns added in order, ``np.sort``."""
    train, query = np.asarray(train, np.float32), np.asarray(query, np.float32)
    sc = StandardScaler().fit(train)

    def scaled(a):
        t = a.copy()
        t -= sc.mean_
        t /= sc.scale_
        return t.astype(np.float64)

    x, q = scaled(train), scaled(query)
    d2 = np.zeros((q.shape[0], x.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(x.shape[1]):
            df = q[:, c:c + 1] - x[None, :, c]
            d2 += df * df
    d2[np.isnan(d2)] = np.inf
    return np.sqrt(np.sort(d2, axis=1)[:, min(k, x.shape[0]) - 1])


def latents(rng, n, z, spread=1.0):
    """Latent-like rows: columns of unequal offsets and widths."""
    off = np.linspace(-2.0, 3.0, z)
    wid = np.linspace(0.3, 2.5, z)[::-1]
    return (off + spread * wid * rng.normal(size=(n, z))).astype(np.float32)


@pytest.mark.parametrize("z", [1, 7, 15])
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("n", [1, 3, 684])
def test_oracle_equals_brute_force(z, k, n):
    rng = np.random.default_rng(1000 * z + 10 * k + n)
    train, query = latents(rng, n, z), latents(rng, 301, z, 1.5)
    got = knn_score_numpy(train, query, k)
    assert got.dtype == np.float64 and got.shape == (301,)
    np.testing.assert_array_equal(got, brute_force(train, query, k))


def test_oracle_chunks_over_queries():
    """More queries than one chunk of the distance matrix holds."""
    rng = np.random.default_rng(5)
    train, query = latents(rng, 684, 7), latents(rng, 7000, 7, 1.5)
    assert 7000 * 684 > (1 << 22)
    np.testing.assert_array_equal(knn_score_numpy(train, query, 5), brute_force(train, query, 5))


# -- small cases worked by hand ------------------------------------------------
# one column, train {0, 2, 4}: mean 2, variance 8/3; a scaled value is (v - 2) / sqrt(8/3) in float32
def _s(v):
    t0 = np.float32(np.float64(np.float32(v)) - 2.0)
    return np.float64(np.float32(np.float64(t0) / np.sqrt(8.0 / 3.0)))


TRAIN3 = np.array([[0.0], [2.0], [4.0]], dtype=np.float32)


def test_hand_worked_distances():
    q = np.array([[1.0], [5.0]], dtype=np.float32)
    # query 1: distances to 0, 2, 4 are 1, 1, 3 (unscaled); query 5: 5, 3, 1
    want1 = sorted([abs(_s(1) - _s(0)), abs(_s(1) - _s(2)), abs(_s(1) - _s(4))])
    want5 = sorted([abs(_s(5) - _s(0)), abs(_s(5) - _s(2)), abs(_s(5) - _s(4))])
    for k in (1, 2, 3):
        np.testing.assert_array_equal(knn_score_numpy(TRAIN3, q, k), [want1[k - 1], want5[k - 1]])


def test_fewer_train_rows_than_k_uses_k_eff():
    q = np.array([[1.0], [5.0]], dtype=np.float32)
    np.testing.assert_array_equal(knn_score_numpy(TRAIN3, q, 16), knn_score_numpy(TRAIN3, q, 3))
    one = np.array([[3.0, -1.0]], dtype=np.float32)   # one train row: both columns constant, scale 1
    got = knn_score_numpy(one, np.array([[3.0, -1.0], [6.0, 3.0]], dtype=np.float32), 5)
    np.testing.assert_array_equal(got, [0.0, 5.0])


def test_duplicate_train_rows_count_with_multiplicity():
    train = np.array([[0.0], [0.0], [0.0], [4.0]], dtype=np.float32)   # mean 1, variance 3
    q = np.array([[0.0]], dtype=np.float32)
    far = abs(np.float64(np.float32(-1.0 / np.sqrt(3.0))) - np.float64(np.float32(3.0 / np.sqrt(3.0))))
    np.testing.assert_array_equal(knn_score_numpy(train, q, 1), [0.0])
    np.testing.assert_array_equal(knn_score_numpy(train, q, 3), [0.0])   # the three copies, not three distinct rows
    np.testing.assert_array_equal(knn_score_numpy(train, q, 4), [far])


def test_query_equal_to_a_train_row_scores_zero():
    rng = np.random.default_rng(11)
    train = latents(rng, 50, 7)
    np.testing.assert_array_equal(knn_score_numpy(train, train[[0, 17, 49]], 1), np.zeros(3))


def test_constant_train_feature_takes_scale_one():
    train = np.array([[0.0, 7.5], [2.0, 7.5], [4.0, 7.5]], dtype=np.float32)
    sc = StandardScaler().fit(train)
    assert sc.scale_[1] == 1.0 and sc.mean_[1] == 7.5
    q = np.array([[2.0, 9.5]], dtype=np.float32)   # on the middle train row but 2.0 off in the unscaled column
    np.testing.assert_array_equal(knn_score_numpy(train, q, 1), [2.0])


def test_nan_query_scores_inf_and_inf_query_too():
    rng = np.random.default_rng(12)
    train, q = latents(rng, 20, 3), latents(rng, 4, 3)
    q[1, 2] = np.nan
    q[2, 0] = np.inf
    got = knn_score_numpy(train, q, 5)
    assert got[1] == np.inf and got[2] == np.inf and np.isfinite(got[[0, 3]]).all()
    np.testing.assert_array_equal(got[[0, 3]], knn_score_numpy(train, q[[0, 3]], 5))


def test_bad_arguments_raise():
    x = np.zeros((3, 2), dtype=np.float32)
    for k in (0, 17):
        with pytest.raises(ValueError):
            knn_score_numpy(x, x, k)
    with pytest.raises(ValueError):
        knn_score_numpy(x[:0], x, 5)


# -- where the centroid scorer fails ------------------------------------------------
def two_cluster_latents(seed=2024, a=4.0, half_width=0.2, n_train=400, n_test=200, z=3):
    """Normal latents in two tight clusters at +-a e0, anomalies at the origin
    (half as wide): the train centroid lies between the clusters, in empty space."""
    rng = np.random.default_rng(seed)

    def cluster(n, w):
        return rng.uniform(-w, w, size=(n, z))

    e0 = np.zeros(z)
    e0[0] = a
    sign = lambda n: np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]   # noqa: E731
    train = (cluster(n_train, half_width) + sign(n_train) * e0).astype(np.float32)
    normal = (cluster(n_test, half_width) + sign(n_test) * e0).astype(np.float32)
    anomalous = cluster(n_test, half_width / 2).astype(np.float32)
    test = np.concatenate([normal, anomalous])
    labels = np.r_[np.zeros(n_test), np.ones(n_test)].astype(np.int64)
    return train, test, labels


def test_knn_separates_what_the_centroid_cannot():
    train, test, labels = two_cluster_latents()
    cen = _host.roc_auc(cen_score_numpy(train, test), labels)
    knn = _host.roc_auc(knn_score_numpy(train, test, 5), labels)
    print(f"two clusters: CEN AUC {cen:.4f}, kNN AUC {knn:.4f}")
    assert cen < 0.5 and knn > 0.99


# -- the GPU test's inputs ----------------------------------------------------------
def tile_rows():
    from fedmse_decentralized_amd.ops import _hip

    return _hip.knn_tile_rows()


def gpu_cases(T):
    """(name, train [n, Z], query [nq, Z], k): a pruned product of
    Z in {1, 7, 15}, k in {1, 5, 16}, n_train in {1, 3, T, T + 1, 683} and
    n_query in {1, 255, 257, 3900}; every value of every axis appears, and
    T + 1 appears with k = 16."""
    grid = [(7, 5, 683, 3900), (7, 16, T + 1, 257), (1, 1, 1, 1), (15, 16, 3, 255), (15, 5, T, 257),
            (1, 16, T + 1, 255), (7, 1, T, 1), (15, 1, 683, 255), (1, 5, 3, 3900), (7, 16, 1, 257)]
    assert {g[0] for g in grid} == {1, 7, 15} and {g[1] for g in grid} == {1, 5, 16}
    assert {g[2] for g in grid} == {1, 3, T, T + 1, 683} and {g[3] for g in grid} == {1, 255, 257, 3900}
    out = []
    for i, (z, k, n, nq) in enumerate(grid):
        rng = np.random.default_rng(7100 + i)
        out.append((f"Z{z}-k{k}-n{n}-q{nq}", _grid(latents(rng, n, z), n), _grid(latents(rng, nq, z, 1.5), n), k))
    return out


def _grid(a, n_train):
    """Latents of a case with one or three train rows, on a grid of 1/256.
    The mean of so few float32 values is often a 25-bit number (always, for
    one row), and ``v - mean`` of full-mantissa values then lands exactly on
    float32 rounding midpoints: ties, which the last bit of the mean decides
    (test_gpu_fixtures_do_not_sit_on_a_rounding_boundary).  On the grid the
    difference is exact or nowhere near a midpoint."""
    return (np.round(a * 256.0) / 256.0).astype(np.float32) if n_train <= 3 else a


def mixed_launch(T):
    """Descriptors of one launch, (train, query) each, Z = 7: unequal sizes,
    the one-row train set, a train set with a constant column, one beyond a tile."""
    rng = np.random.default_rng(7200)
    sizes = [(683, 3900), (1, 257), (40, 255), (T + 1, 1), (3, 600)]
    out = [(_grid(latents(rng, n, 7), n), _grid(latents(rng, nq, 7, 1.5), n)) for n, nq in sizes]
    out[2][0][:, 4] = np.float32(0.625)
    out[2][1][:, 4] = _grid(out[2][1][:, 4], 1)   # (the constant column's mean is exact: see _grid)
    return out


def _nudged(train, dm, ds):
    sc = StandardScaler().fit(train)
    if dm:
        sc.mean_ = np.nextafter(sc.mean_, np.full_like(sc.mean_, dm * np.inf))
    if ds:
        sc.scale_ = np.nextafter(sc.scale_, np.full_like(sc.scale_, ds * np.inf))
    return sc


def test_gpu_fixtures_do_not_sit_on_a_rounding_boundary():
    """The fitted mean and scale each nudged by +-1 float64 ulp (the kernel
    sums in another order than numpy): the scores of the GPU test's inputs
    stay within its tolerance, so no input sits where such a nudge flips an
    fp32 rounding of a scaled value.  A seed that fails this is changed
    here; the tolerance is not."""
    T = tile_rows()
    items = [(name, tr, qu, k) for name, tr, qu, k in gpu_cases(T)]
    items += [(f"mixed{i}", tr, qu, 5) for i, (tr, qu) in enumerate(mixed_launch(T))]
    for name, tr, qu, k in items:
        want = knn_score_numpy(tr, qu, k)
        for dm in (-1, 0, 1):
            for ds in (-1, 0, 1):
                got = knn_score_numpy(tr, qu, k, scaler=_nudged(tr, dm, ds))
                np.testing.assert_allclose(got, want, rtol=GPU_TOL, atol=GPU_TOL, err_msg=f"{name} {dm} {ds}")


# -- config and federation ----------------------------------------------------------
def test_config_fields():
    cfg = ExperimentConfig()
    assert (cfg.latent_scorer, cfg.knn_k) == ("cen", 5)
    for bad in ("lof", "KNN", ""):
        with pytest.raises(ValueError):
            ExperimentConfig(latent_scorer=bad)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            ExperimentConfig(knn_k=bad)
    ExperimentConfig(latent_scorer="knn", knn_k=1)
    ExperimentConfig(latent_scorer="knn", knn_k=16, compat="reference")   # allowed in both compat modes


def test_command_line_options():
    import argparse

    from fedmse_decentralized_amd.config import add_arguments, from_args

    p = add_arguments(argparse.ArgumentParser())
    cfg = from_args(p.parse_args(["--latent-scorer", "knn", "--knn-k", "3"]))
    assert (cfg.latent_scorer, cfg.knn_k) == ("knn", 3)
    cfg = from_args(p.parse_args([]))
    assert (cfg.latent_scorer, cfg.knn_k) == ("cen", 5)


def test_older_config_snapshot_still_loads():
    import dataclasses
    import json

    old = json.loads(ExperimentConfig().to_json())
    del old["latent_scorer"], old["knn_k"]
    cfg = ExperimentConfig(**old)
    assert dataclasses.asdict(cfg)["latent_scorer"] == "cen" and cfg.knn_k == 5


@pytest.fixture
def shrunk(monkeypatch):
    """Small clients for this test only (restored afterwards, with the prepared-data cache)."""
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    orig = synthetic.SyntheticSpec.resolved

    def resolved(self):
        s = orig(self)
        s.normal_rows, s.abnormal_rows, s.test_normal_rows = (60, 70), (80, 90), 15
        return s

    monkeypatch.setattr(synthetic.SyntheticSpec, "resolved", resolved)
    federation._PREP_CACHE.clear()
    yield
    federation._PREP_CACHE.clear()


def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=4, num_rounds=2, epoch=1, batch_size=12, output_root=out,
                backend="torch", device="cpu", log_level="WARNING", global_early_stop=False, save_checkpoints=False,
                compat="fixed")
    base.update(kw)
    return ExperimentConfig(**base)


def _rounds(cfg, model_type):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.federation import Federation

    federation._PREP_CACHE.clear()
    fed = Federation(cfg, model_type, "avg", 0).setup()
    rs = [fed.run_round() for _ in range(2)]
    fed.finish()
    fed.writer.flush()
    return fed, rs


@pytest.mark.parametrize("metric", ["AUC", "detection"])
def test_torch_federation_with_knn_scorer(tmp_path, shrunk, metric):
    from fedmse_decentralized_amd.eval.evaluator import evaluate_clients

    fed, rs = _rounds(_cfg(str(tmp_path / "knn"), metric=metric, latent_scorer="knn", knn_k=3), "hybrid")
    eng = fed.engine
    assert (eng.latent_scorer, eng.knn_k) == ("knn", 3)
    for r in rs:
        assert r.metrics.shape == (4,) and np.isfinite(r.metrics).all()
        assert ((0.0 <= r.metrics) & (r.metrics <= 1.0)).all()
        assert (r.detection is not None) == (metric == "detection")
    # the round's metric is the evaluator's, which scores by kNN ...
    er = evaluate_clients(eng, list(range(fed.N)), "hybrid", metric)
    np.testing.assert_array_equal(er.metrics, rs[-1].metrics)
    st = eng.store
    items = []
    for c in range(fed.N):
        items += [(c, st.rows("train", c)), (c, st.rows("test", c))]
    _, lat = eng.forward_rows(st.params, items, want_sse=False, want_latent=True)
    scores = eng.latent_scores(lat[0::2], lat[1::2])
    for c in range(fed.N):
        want = knn_score_numpy(lat[2 * c].numpy(), lat[2 * c + 1].numpy(), 3)
        np.testing.assert_array_equal(scores[c].numpy(), want)
    if metric == "AUC":
        np.testing.assert_array_equal(er.metrics, eng.auc(scores, [st.label_view(c) for c in range(fed.N)]))
    # ... and differs from the centroid scorer's on the same parameters
    eng.latent_scorer = "cen"
    assert not np.array_equal(evaluate_clients(eng, list(range(fed.N)), "hybrid", metric).metrics, er.metrics)


@pytest.mark.parametrize("metric", ["AUC", "detection"])
def test_autoencoder_ignores_the_scorer(tmp_path, shrunk, metric):
    _, a = _rounds(_cfg(str(tmp_path / "knn"), metric=metric, latent_scorer="knn"), "autoencoder")
    _, b = _rounds(_cfg(str(tmp_path / "cen"), metric=metric), "autoencoder")
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.metrics, y.metrics)
        assert x.aggregator == y.aggregator
