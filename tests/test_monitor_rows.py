"""Monitoring a deployed detector on the CPU (README "Monitoring a deployed
detector"): the oracle ``monitor_rows_numpy`` against a direct numpy
computation over all rows (masks, ``np.searchsorted``, ``math.fsum``),
``TorchEngine.monitor_rows``, the bundle's baseline (round trip, what the
reader refuses, bundles without one), a small synthetic federation exported
with ``--export-baseline``, a shifted feature showing up as drift, and
``detect --monitor``.

The float64 sums are held to the bound of a sequential sum of ``cnt`` terms,
``cnt * 2^-53 * sum |term|``, against ``math.fsum`` of the same terms."""
import argparse
import dataclasses
import math
import os
import random

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.config import ExperimentConfig, add_arguments, from_args
from fedmse_decentralized_amd.data.prepare import split_sizes
from fedmse_decentralized_amd.deploy.detector import (Baseline, Detector, DriftReport, make_baseline,
                                                      monitor_rows_numpy, score_rows_numpy)
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
from fedmse_decentralized_amd.eval.metrics import calibration_rank
from fedmse_decentralized_amd.models.layout import ModelDims

DIMS = ModelDims(5, 3, 2)
KINDS = [("autoencoder", None), ("hybrid", "cen"), ("hybrid", "knn")]
U = 2.0 ** -53


def make_detector(model_type="autoencoder", scaler="standard", scorer=None, dims=DIMS, seed=0, threshold=0.75):
    rng = np.random.default_rng(seed)
    D, Z = dims.d_in, dims.latent
    if scaler == "standard":
        sc = {"mean_": rng.normal(size=D), "scale_": rng.uniform(0.5, 2.0, size=D)}
    else:
        sc = {"scale_": rng.uniform(0.5, 2.0, size=D), "min_": rng.normal(size=D)}
    kw = {}
    if model_type == "hybrid":
        kw = dict(latent_scorer=scorer, latent_mean=rng.normal(size=Z), latent_scale=rng.uniform(0.5, 2.0, size=Z))
        if scorer == "knn":
            kw.update(knn_k=3, train_latents=rng.normal(size=(9, Z)).astype(np.float32))
    return Detector(dims=dims, model_type=model_type, params=(0.3 * rng.normal(size=dims.num_params)).astype(np.float32),
                    scaler_kind=scaler, scaler=sc, threshold=threshold, detect_quantile=0.9, **kw)


def with_baseline(det, rng, bins=10, n=90):
    """A baseline from random rows of the detector's own input space."""
    x = rng.normal(size=(n, det.dims.d_in)) * 1.5
    s = np.sort(score_rows_numpy(det, x)[0])
    return dataclasses.replace(det, baseline=make_baseline(det.standardise(x), s, bins))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def raw_rows(rng, n, D, special=True):
    x = rng.normal(size=(n, D)) * 2.0
    if special and n > 6:
        x[1, 0] = np.nan
        x[4, D - 1] = np.inf
        x[6, 0] = -np.inf
    return x


def brute_force(det, rows):
    """The report's order-free fields straight from all rows."""
    x = det.standardise(rows)
    fin = np.isfinite(x)
    base = det.baseline
    lo = base.feat_lo if base is not None else np.full(x.shape[1], -np.inf, np.float32)
    hi = base.feat_hi if base is not None else np.full(x.shape[1], np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        out = (fin & ((x < lo) | (x > hi))).sum(axis=0)
    mn = np.where(fin, x, np.float32(np.inf)).min(axis=0, initial=np.float32(np.inf))
    mx = np.where(fin, x, np.float32(-np.inf)).max(axis=0, initial=np.float32(-np.inf))
    s, f, a = score_rows_numpy(det, rows)
    hist = None
    if base is not None:
        hist = np.bincount(np.searchsorted(base.score_edges, s, side="left"), minlength=base.score_edges.shape[0] + 1)
    return x, fin, fin.sum(axis=0), (~fin).sum(axis=0), out, mn, mx, a, hist


def check_sums(rep, x, fin, what):
    """sum / sq within cnt * 2^-53 * sum |term| of math.fsum of the same terms."""
    worst = 0.0
    for d in range(x.shape[1]):
        t = x[fin[:, d], d].astype(np.float64)
        for got, terms in ((rep.sum[d], t), (rep.sq[d], t * t)):
            bound = t.shape[0] * U * float(np.sum(np.abs(terms)))
            err = abs(float(got) - math.fsum(terms.tolist()))
            assert err <= bound, (what, d, got, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    return worst


@pytest.mark.parametrize("n,block_rows", [(0, 64), (1, 64), (15, 64), (16, 64), (17, 64), (63, 64), (64, 64), (65, 64),
                                          (200, 64), (200, 128), (333, 192)])
@pytest.mark.parametrize("model_type,scorer", KINDS)
def test_oracle_against_brute_force(model_type, scorer, n, block_rows):
    rng = np.random.default_rng(n + block_rows)
    for scaler, baseline in (("standard", True), ("minmax", False)):
        det = make_detector(model_type, scaler, scorer, seed=n)
        if baseline:
            det = with_baseline(det, rng, bins=10)
        rows = raw_rows(rng, n, DIMS.d_in)
        rep = monitor_rows_numpy(det, rows, block_rows)
        assert isinstance(rep, DriftReport) and rep.n == n and rep.block_rows == block_rows
        x, fin, cnt, bad, out, mn, mx, alarms, hist = brute_force(det, rows)
        for got, want in ((rep.cnt, cnt), (rep.bad, bad), (rep.out, out)):
            assert got.dtype == np.int64 and got.shape == (DIMS.d_in,) and np.array_equal(got, want)
        assert rep.mn.dtype == np.float32 and np.array_equal(rep.mn, mn) and np.array_equal(rep.mx, mx)
        assert rep.sum.dtype == np.float64 and rep.sq.dtype == np.float64
        assert rep.alarms == alarms == score_rows_numpy(det, rows)[2]
        if baseline:
            assert rep.hist.dtype == np.int64 and np.array_equal(rep.hist, hist) and int(rep.hist.sum()) == n
        else:
            assert rep.hist is None and math.isnan(rep.psi)
        check_sums(rep, x, fin, f"{model_type}/{scorer} n={n} R={block_rows}")
        assert np.all(rep.cnt + rep.bad == n)
        if n == 0:
            assert not rep.sum.any() and not np.signbit(rep.sum).any() and np.all(rep.mn == np.inf) \
                and np.all(rep.mx == -np.inf) and rep.alarms == 0
        # derived values
        with np.errstate(all="ignore"):
            assert np.array_equal(rep.mean, rep.sum / rep.cnt, equal_nan=True)
            assert np.array_equal(rep.out_share, rep.out / np.maximum(rep.cnt, 1))
        assert rep.alarm_rate == alarms / max(n, 1) and rep.expected_alarm_rate == 1.0 - det.detect_quantile


def test_block_rows_changes_only_the_summation_order():
    rng = np.random.default_rng(3)
    det = with_baseline(make_detector("hybrid", "standard", "cen"), rng)
    rows = raw_rows(rng, 700, DIMS.d_in)
    a, b = monitor_rows_numpy(det, rows, 64), monitor_rows_numpy(det, rows, 256)
    for k in ("cnt", "bad", "out", "mn", "mx", "hist"):
        assert same_bits(getattr(a, k), getattr(b, k)), k
    assert a.alarms == b.alarms and (a.block_rows, b.block_rows) == (64, 256)
    x = det.standardise(rows)
    fin = np.isfinite(x)
    check_sums(a, x, fin, "R=64"), check_sums(b, x, fin, "R=256")
    for bad in (0, 100, -64, 64.0, True):
        with pytest.raises(ValueError):
            monitor_rows_numpy(det, rows, bad)


def test_stream_order_is_the_rule():
    """Values whose float64 sums depend on the order, signed zeros among them
    (standard: feature 0; minmax with a negative factor, which gives -0.0:
    feature 1): ``sum``, ``sq``, ``mn`` and ``mx`` equal the rule written out
    as plain loops over blocks, waves, tiles and rows, bit for bit."""
    dims = ModelDims(2, 1, 1)
    det = Detector(dims=dims, model_type="autoencoder", params=np.zeros(dims.num_params, np.float32),
                   scaler_kind="minmax", scaler={"scale_": np.array([1.0, -1.0]), "min_": np.array([0.0, -0.0])})
    rng = np.random.default_rng(8)
    n, R = 200, 64
    rows = (rng.normal(size=(n, 2)) * 10.0 ** rng.integers(-6, 7, size=(n, 2))).astype(np.float32)
    rows[rng.integers(0, n, size=40), rng.integers(0, 2, size=40)] = 0.0
    rows[:, 1] = np.minimum(rows[:, 1], 0.0)    # feature 1: values >= 0 with -0.0 (from +0.0 * -1) as the smallest
    rows[5, 0] = np.nan
    x = det.standardise(rows)
    assert np.signbit(x[rows[:, 1] == 0.0, 1]).all() and (rows[:, 1] == 0.0).sum() >= 2
    rep = monitor_rows_numpy(det, rows, R)
    for d in range(2):
        tot, totq = 0.0, 0.0
        tmn, tmx = np.float32(np.inf), np.float32(-np.inf)
        for b in range(0, n, R):
            parts = []
            for w in range(4):
                s, q, mn, mx = 0.0, 0.0, np.float32(np.inf), np.float32(-np.inf)
                for t in range(w, R // 16, 4):
                    for r in range(b + 16 * t, min(n, b + R, b + 16 * t + 16)):
                        v = x[r, d]
                        if not np.isfinite(v):
                            continue
                        s = s + float(v)
                        q = q + float(v) * float(v)
                        mn = v if v < mn else mn
                        mx = v if v > mx else mx
                parts.append((s, q, mn, mx))
            bs, bq, bmn, bmx = parts[0]
            for s, q, mn, mx in parts[1:]:
                bs, bq = bs + s, bq + q
                bmn = mn if mn < bmn else bmn
                bmx = mx if mx > bmx else bmx
            tot, totq = tot + bs, totq + bq
            tmn = bmn if bmn < tmn else tmn
            tmx = bmx if bmx > tmx else tmx
        assert same_bits(rep.sum[d], np.float64(tot)) and same_bits(rep.sq[d], np.float64(totq)), d
        assert same_bits(rep.mn[d], np.float32(tmn)) and same_bits(rep.mx[d], np.float32(tmx)), d
    assert rep.cnt.tolist() == [n - 1, n] and rep.mn[1] == 0.0


def test_ties_with_the_band_and_the_edges_are_inside_and_low():
    rng = np.random.default_rng(5)
    det = make_detector("autoencoder", "standard", None)
    rows = raw_rows(rng, 40, DIMS.d_in, special=False)
    x = det.standardise(rows)
    s = score_rows_numpy(det, rows)[0]
    edges = np.sort(s[[3, 7, 7, 20]])   # a repeated edge: an empty bin
    base = Baseline(feat_lo=x.min(axis=0), feat_hi=x.max(axis=0), score_edges=edges, score_base=np.zeros(5, np.int64))
    rep = monitor_rows_numpy(dataclasses.replace(det, baseline=base), rows, 64)
    assert not rep.out.any()
    assert np.array_equal(rep.hist, [np.sum(s <= edges[0]), np.sum((s > edges[0]) & (s <= edges[1])),
                                     np.sum((s > edges[1]) & (s <= edges[2])), np.sum((s > edges[2]) & (s <= edges[3])),
                                     np.sum(s > edges[3])])
    assert rep.hist[0] >= 1 and 0 in rep.hist.tolist()
    tight = Baseline(feat_lo=np.nextafter(base.feat_lo, np.float32(np.inf)), feat_hi=base.feat_hi,
                     score_edges=edges[:0], score_base=np.zeros(1, np.int64))
    rep = monitor_rows_numpy(dataclasses.replace(det, baseline=tight), rows, 64)
    assert np.all(rep.out >= 1) and rep.hist.tolist() == [40] and math.isnan(rep.psi)
    nan_tau = monitor_rows_numpy(dataclasses.replace(det, threshold=float("nan")), rows, 64)
    assert nan_tau.alarms == 0 and nan_tau.alarm_rate == 0.0


@pytest.mark.parametrize("model_type,scorer", KINDS)
def test_torch_engine_returns_the_oracles_bits(model_type, scorer):
    rng = np.random.default_rng(11)
    dims2 = ModelDims(7, 4, 3)
    dets = [with_baseline(make_detector(model_type, "standard", scorer), rng),
            make_detector(model_type, "minmax", scorer, dims=dims2, seed=2)]
    rows = [raw_rows(rng, 130, 5), raw_rows(rng, 0, 7).astype(np.float32)]
    eng = TorchEngine(DIMS, torch.device("cpu"))
    got = eng.monitor_rows(dets, rows, block_rows=64)
    for det, x, g in zip(dets, rows, got):
        want = monitor_rows_numpy(det, x, 64)
        for f in dataclasses.fields(DriftReport):
            a, b = getattr(g, f.name), getattr(want, f.name)
            if isinstance(a, np.ndarray):
                assert same_bits(a, b), f.name
            else:
                assert a == b or (a != a and b != b), f.name
    from fedmse_decentralized_amd.ops._hip import score_rows_per_block

    assert eng.monitor_rows(dets, rows)[0].block_rows == score_rows_per_block(130)
    with pytest.raises(ValueError):
        eng.monitor_rows(dets, rows[:1])
    with pytest.raises(ValueError):
        eng.monitor_rows(dets[:1], [rows[1]])
    with pytest.raises(ValueError):
        eng.monitor_rows(dets, rows, block_rows=100)


# ---------------------------------------------------------------------------
# the bundle
# ---------------------------------------------------------------------------
PLAIN_KEYS = {"version", "dims", "model_type", "params", "scaler_kind", "threshold", "detect_quantile", "provenance",
              "scaler_mean_", "scaler_scale_"}
BASE_KEYS = {"baseline_feat_lo", "baseline_feat_hi", "baseline_score_edges", "baseline_score_base"}


def test_bundle_round_trip_with_and_without_a_baseline(tmp_path):
    rng = np.random.default_rng(2)
    plain = make_detector()
    p0 = plain.save(str(tmp_path / "plain.npz"))
    with np.load(p0) as z:
        assert set(z.files) == PLAIN_KEYS   # exactly the arrays a bundle held before baselines existed
    assert Detector.load(p0).baseline is None
    for bins in (2, 10, 16):
        det = with_baseline(plain, rng, bins=bins)
        b = det.baseline
        assert b.feat_lo.dtype == np.float32 and b.score_edges.dtype == np.float64 and b.score_base.dtype == np.int64
        assert b.score_edges.shape == (bins - 1,) and b.score_base.shape == (bins,) and int(b.score_base.sum()) == 90
        p = det.save(str(tmp_path / f"b{bins}.npz"))
        with np.load(p) as z:
            assert set(z.files) == PLAIN_KEYS | BASE_KEYS
        got = Detector.load(p).baseline
        for k in ("feat_lo", "feat_hi", "score_edges", "score_base"):
            assert same_bits(getattr(got, k), getattr(b, k)), k
    # no calibration scores: no edges, one empty bin; a feature without a finite train value
    x = rng.normal(size=(4, 5)).astype(np.float32)
    x[:, 2] = np.nan
    b = make_baseline(x, np.zeros(0), 10)
    assert b.score_edges.shape == (0,) and b.score_base.tolist() == [0]
    assert b.feat_lo[2] == np.inf and b.feat_hi[2] == -np.inf and b.feat_lo[0] == x[:, 0].min()
    got = Detector.load(dataclasses.replace(plain, baseline=b).save(str(tmp_path / "e.npz"))).baseline
    assert got.score_edges.shape == (0,) and got.feat_lo[2] == np.inf


def _resave(path, out, drop=(), **change):
    with np.load(path) as z:
        a = {k: z[k] for k in z.files if k not in drop}
    a.update(change)
    with open(out, "wb") as f:
        np.savez(f, **a)
    return out


def test_malformed_baselines_are_refused(tmp_path):
    det = with_baseline(make_detector(), np.random.default_rng(4))
    good = det.save(str(tmp_path / "good.npz"))
    out = str(tmp_path / "bad.npz")
    b = det.baseline
    cases = [dict(drop=("baseline_feat_hi",)),
             dict(drop=("baseline_feat_lo", "baseline_feat_hi", "baseline_score_base")),
             dict(baseline_feat_lo=b.feat_lo[:4]),
             dict(baseline_feat_hi=b.feat_hi.astype(np.float64)),
             dict(baseline_score_edges=b.score_edges.astype(np.float32)),
             dict(baseline_score_base=b.score_base.astype(np.float64)),
             dict(baseline_score_base=b.score_base[:-1]),
             dict(baseline_score_edges=b.score_edges[::-1].copy()),
             dict(baseline_score_base=-b.score_base - 1),
             dict(baseline_score_edges=np.arange(16.0), baseline_score_base=np.zeros(17, np.int64))]
    for c in cases:
        drop = c.pop("drop", ())
        with pytest.raises(ValueError):
            Detector.load(_resave(good, out, drop=drop, **c))
    assert Detector.load(_resave(good, out)).baseline is not None
    with pytest.raises(ValueError):
        dataclasses.replace(det, baseline=Baseline(b.feat_lo, b.feat_hi, np.arange(16.0), np.zeros(17, np.int64)))
    with pytest.raises(ValueError):
        make_baseline(np.zeros((3, 5), np.float32), np.zeros(3), 17)


def test_config_flags():
    p = add_arguments(argparse.ArgumentParser())
    cfg = from_args(p.parse_args(["--export-detectors", "--export-baseline", "--monitor-bins", "4"]))
    assert cfg.export_baseline is True and cfg.monitor_bins == 4
    d = ExperimentConfig()
    assert d.export_baseline is False and d.monitor_bins == 10
    for bad in (1, 17):
        with pytest.raises(ValueError):
            ExperimentConfig(monitor_bins=bad)
    with pytest.raises(ValueError):
        ExperimentConfig(export_baseline=True)


def test_export_baseline_without_export_detectors_is_refused(capsys):
    import main as entry

    with pytest.raises(SystemExit) as e:
        entry.main(["--export-baseline"])
    assert e.value.code == 2 and "--export-baseline needs --export-detectors" in capsys.readouterr().err


# ---------------------------------------------------------------------------
# a federation's bundles
# ---------------------------------------------------------------------------
def _small(orig):
    def resolved(self):
        s = orig(self)
        s.normal_rows, s.abnormal_rows, s.test_normal_rows = (60, 70), (80, 90), 15
        return s
    return resolved


def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=3, num_rounds=2, epoch=1, batch_size=12, output_root=out,
                backend="torch", device="cpu", log_level="WARNING", global_early_stop=False, save_checkpoints=False,
                compat="fixed", metric="detection", detect_quantile=0.9, export_detectors=True, export_baseline=True,
                monitor_bins=5)
    base.update(kw)
    return ExperimentConfig(**base)


def raw_splits(cfg):
    """Every client's raw train, validation and test rows (with labels), in the
    federation's client order (as tests/test_detector_bundle.py forms them)."""
    from fedmse_decentralized_amd.data.synthetic import SyntheticSpec, generate_client

    spec = SyntheticSpec(kind=cfg.synthetic, n_clients=cfg.network_size, iid=cfg.synthetic_iid,
                         alpha=cfg.synthetic_alpha, seed=cfg.synthetic_seed)
    chosen = random.Random(cfg.data_seed).sample(list(range(cfg.network_size)), cfg.network_size)
    rs = np.random.RandomState(cfg.data_seed)
    out = []
    for i in chosen:
        raw = generate_client(spec, i)
        normal = raw.normal[rs.permutation(raw.normal.shape[0])]
        abnormal = raw.abnormal[rs.permutation(raw.abnormal.shape[0])]
        tr, va, de, _ = split_sizes(normal.shape[0])
        parts = [normal[tr + va + de:]] + ([raw.test_normal] if cfg.new_device else []) + [abnormal]
        labels = np.r_[np.zeros(sum(p.shape[0] for p in parts[:-1]), np.int64), np.ones(abnormal.shape[0], np.int64)]
        out.append((raw.name, normal[:tr], normal[tr:tr + va], np.concatenate(parts, 0), labels))
    return out


@pytest.fixture(scope="module", params=KINDS, ids=lambda k: f"{k[0]}-{k[1]}")
def exported(request, tmp_path_factory):
    """A small synthetic federation run to its end with --export-baseline:
    (federation, cfg, raw splits, loaded bundles)."""
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    model_type, scorer = request.param
    mp = pytest.MonkeyPatch()
    mp.setattr(synthetic.SyntheticSpec, "resolved", _small(synthetic.SyntheticSpec.resolved))
    federation._PREP_CACHE.clear()
    try:
        cfg = _cfg(str(tmp_path_factory.mktemp("fed")), latent_scorer=scorer or "cen", knn_k=3)
        fed = federation.Federation(cfg, model_type, "avg", 0).setup()
        fed.run_all()
        splits = raw_splits(cfg)
        dets = [Detector.load(os.path.join(fed.save_dirs[c], "detector.npz")) for c in range(len(splits))]
        yield fed, cfg, splits, dets
    finally:
        mp.undo()
        federation._PREP_CACHE.clear()


def test_exported_baseline_describes_the_clients_own_data(exported):
    fed, cfg, splits, dets = exported
    assert [s[0] for s in splits] == [c.name for c in fed.clients]
    for c, (det, (name, train_raw, valid_raw, test_raw, labels)) in enumerate(zip(dets, splits)):
        b = det.baseline
        assert b is not None and b.score_edges.shape == (4,) and b.score_base.shape == (5,)
        assert same_bits(det.standardise(train_raw), fed.clients[c].train)
        n_valid = valid_raw.shape[0]
        assert int(b.score_base.sum()) == n_valid
        vs = np.sort(score_rows_numpy(det, valid_raw, engine=fed.engine)[0])
        want = np.array([vs[calibration_rank(n_valid, (i + 1) / 5)] for i in range(4)])
        assert same_bits(b.score_edges, want)
        x = det.standardise(train_raw)
        assert same_bits(b.feat_lo, x.min(axis=0)) and same_bits(b.feat_hi, x.max(axis=0))
        rep = fed.engine.monitor_rows([det], [train_raw])[0]
        assert not rep.out.any() and np.all(rep.cnt == train_raw.shape[0])
        rep = fed.engine.monitor_rows([det], [valid_raw])[0]
        assert np.array_equal(rep.hist, b.score_base) and rep.psi == 0.0


def test_export_without_the_flag_writes_no_baseline(tmp_path):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    mp = pytest.MonkeyPatch()
    mp.setattr(synthetic.SyntheticSpec, "resolved", _small(synthetic.SyntheticSpec.resolved))
    federation._PREP_CACHE.clear()
    try:
        fed = federation.Federation(_cfg(str(tmp_path), export_baseline=False, num_rounds=1), "autoencoder", "avg",
                                    0).setup()
        fed.run_all()
        with np.load(os.path.join(fed.save_dirs[0], "detector.npz")) as z:
            assert set(z.files) == PLAIN_KEYS
    finally:
        mp.undo()
        federation._PREP_CACHE.clear()


def test_a_shifted_feature_shows_as_drift(exported):
    """A condition on the rule (the oracle alone): 4 train standard deviations
    added to one feature of every benign test row."""
    fed, cfg, splits, dets = exported
    det, (_, _, _, test_raw, labels) = dets[0], splits[0]
    benign = test_raw[labels == 0]
    assert benign.shape[0] >= 5 and det.scaler_kind == "standard"
    d_star = 7
    shifted = benign.copy()
    shifted[:, d_star] += 4.0 * det.scaler["scale_"][d_star]
    before = monitor_rows_numpy(det, benign, 64, engine=fed.engine)
    after = monitor_rows_numpy(det, shifted, 64, engine=fed.engine)
    print(f"psi before {before.psi:.4g} after {after.psi:.4g}; out_share[d*] {before.out_share[d_star]:.3f} -> "
          f"{after.out_share[d_star]:.3f}; largest other {np.delete(after.out_share, d_star).max():.3f}")
    assert after.out_share[d_star] > np.delete(after.out_share, d_star).max()
    assert int(np.argmax(after.out_share)) == d_star
    assert abs((after.mean[d_star] - before.mean[d_star]) - 4.0) <= 1e-3
    others = np.delete(np.arange(det.dims.d_in), d_star)
    assert same_bits(after.sum[others], before.sum[others])


# ---------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------
def test_detect_monitor(tmp_path, capsys):
    from fedmse_decentralized_amd import detect

    rng = np.random.default_rng(6)
    det = with_baseline(make_detector(threshold=0.2), rng)
    rows = raw_rows(rng, 75, DIMS.d_in, special=False)
    rows[:, 2] += 40.0   # feature 2 leaves the band in every row
    csv = str(tmp_path / "traffic.csv")
    np.savetxt(csv, rows, delimiter=",", fmt="%.17g")
    bundle = det.save(str(tmp_path / "detector.npz"))
    out0, out1 = str(tmp_path / "plain.npz"), str(tmp_path / "mon.npz")
    assert detect.main(["--detector", bundle, "--input", csv, "--output", out0, "--backend", "torch"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("detect: rows 75")
    with np.load(out0) as z:
        assert set(z.files) == {"scores", "flags", "alarms", "threshold"}   # as before --monitor existed
    assert detect.main(["--detector", bundle, "--input", csv, "--output", out1, "--backend", "torch", "--monitor",
                        "--monitor-top", "2"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("detect: rows 75")
    want = TorchEngine(DIMS, torch.device("cpu")).monitor_rows([det], [rows])[0]
    words = lines[1].split()
    assert words[:2] == ["monitor:", "alarm_rate"] and words[3] == "expected" and words[5] == "psi"
    assert words[7:9] == ["worst", "features"] and len(words) == 11 and "baseline" not in lines[1]
    assert words[9] == f"2:{want.out_share[2]:.4g}" and want.out_share[2] == 1.0
    order = np.argsort(-want.out_share, kind="stable")
    assert words[10].split(":")[0] == str(int(order[1]))
    with np.load(out1) as z:
        keys = set(z.files)
        fields = {f.name for f in dataclasses.fields(DriftReport)}
        assert keys == {"scores", "flags", "alarms", "threshold"} | {"monitor_" + k for k in fields}
        for k in fields:
            assert same_bits(z["monitor_" + k], np.asarray(getattr(want, k))), k
    # a bundle without a baseline: no band, no histogram
    bare = make_detector(threshold=0.2).save(str(tmp_path / "bare.npz"))
    assert detect.main(["--detector", bare, "--input", csv, "--output", out1, "--backend", "torch", "--monitor"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[1].endswith("baseline none") and " psi nan " in lines[1]
    with np.load(out1) as z:
        assert "monitor_hist" not in z.files and "monitor_cnt" in z.files and not z["monitor_out"].any()
