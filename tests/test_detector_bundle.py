"""Deployable detectors on the CPU (README "Deploying a detector"): the
``.npz`` bundle round trip and what its reader refuses, the bundle's
standardisation against ``IoTDataProcessor`` bit for bit, a small synthetic
federation exported with ``--export-detectors`` whose bundles reproduce the
last round's threshold and tp / fp / fn / tn from the clients' *raw* rows, the
flag's off state, and the command-line tool on the torch backend."""
import argparse
import dataclasses
import os
import random

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.config import ExperimentConfig, add_arguments, from_args
from fedmse_decentralized_amd.data.prepare import split_sizes
from fedmse_decentralized_amd.data.scaler import IoTDataProcessor
from fedmse_decentralized_amd.deploy.detector import (FORMAT_VERSION, Detector, cen_scores_stored, clean_and_flag,
                                                      score_rows_numpy)
from fedmse_decentralized_amd.models.layout import ModelDims

DBL_MAX = np.finfo(np.float64).max


def make_detector(model_type="autoencoder", scaler="standard", scorer=None, dims=ModelDims(5, 3, 2), seed=0,
                  threshold=0.75, n_train=9, k=3):
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
            kw.update(knn_k=k, train_latents=rng.normal(size=(n_train, Z)).astype(np.float32))
    return Detector(dims=dims, model_type=model_type, params=(0.3 * rng.normal(size=dims.num_params)).astype(np.float32),
                    scaler_kind=scaler, scaler=sc, threshold=threshold, detect_quantile=0.9,
                    provenance={"client": "c-1", "update_type": "avg", "rounds": "2"}, **kw)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


KINDS = [("autoencoder", None), ("hybrid", "cen"), ("hybrid", "knn")]


# ---------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scaler", ["standard", "minmax"])
@pytest.mark.parametrize("model_type,scorer", KINDS)
def test_round_trip(tmp_path, model_type, scorer, scaler):
    det = make_detector(model_type, scaler, scorer, threshold=float("nan") if scaler == "minmax" else 0.75)
    path = det.save(str(tmp_path / "detector.npz"))
    assert path.endswith("detector.npz") and os.path.exists(path)
    got = Detector.load(path)
    assert (got.dims, got.model_type, got.scaler_kind, got.latent_scorer, got.knn_k, got.version) == \
        (det.dims, det.model_type, det.scaler_kind, det.latent_scorer, det.knn_k, FORMAT_VERSION)
    assert same_bits(got.params, det.params) and got.params.dtype == np.float32
    assert set(got.scaler) == set(det.scaler)
    for k in det.scaler:
        assert same_bits(got.scaler[k], det.scaler[k]) and got.scaler[k].dtype == np.float64
    assert same_bits(np.float64(got.threshold), np.float64(det.threshold))
    assert got.detect_quantile == det.detect_quantile and got.provenance == det.provenance
    for name in ("latent_mean", "latent_scale", "train_latents"):
        a, b = getattr(got, name), getattr(det, name)
        assert (a is None) == (b is None) and (a is None or same_bits(a, b)), name
    with np.load(path, allow_pickle=False) as z:   # plain arrays: nothing needs pickle
        assert all(z[k].dtype.kind in "fiuU" for k in z.files)


def _resave(path, out, **changes):
    with np.load(path, allow_pickle=False) as z:
        a = {k: z[k] for k in z.files}
    for k, v in changes.items():
        if v is None:
            a.pop(k)
        else:
            a[k] = v
    with open(out, "wb") as f:
        np.savez(f, **a)
    return out


def test_load_refuses_bad_files(tmp_path):
    good = make_detector("hybrid", "standard", "knn").save(str(tmp_path / "good.npz"))
    bad = str(tmp_path / "bad.npz")
    with pytest.raises(ValueError, match="version"):
        Detector.load(_resave(good, bad, version=np.array(FORMAT_VERSION + 1, dtype=np.int64)))
    # a pickle-bearing member
    with open(bad, "wb") as f:
        np.savez(f, **{**dict(np.load(good)), "provenance": np.array({"a": 1}, dtype=object)})
    with pytest.raises(ValueError):
        Detector.load(bad)
    for changes in (dict(params=np.zeros(7, np.float32)),                      # wrong parameter count
                    dict(scaler_mean_=np.zeros(4)),                           # scaler shorter than d_in
                    dict(scaler_scale_=None),                                 # a missing vector
                    dict(latent_mean_=np.zeros(3)),                           # latent scaler longer than Z
                    dict(train_latents=np.zeros((4, 3), np.float32)),         # latents of another width
                    dict(knn_k=np.array(17, dtype=np.int64)),                 # beyond the kernel's list
                    dict(dims=np.array([5, 3], dtype=np.int64)),
                    dict(dims=np.array([200, 3, 2], dtype=np.int64)),
                    dict(model_type=np.array("forest")),
                    dict(scaler_kind=np.array("robust")),
                    dict(params=np.zeros(ModelDims(5, 3, 2).num_params, np.float64))):   # not the stored type
        with pytest.raises(ValueError):
            Detector.load(_resave(good, bad, **changes))
    with open(bad, "wb") as f:
        f.write(b"not a zip file")
    with pytest.raises(ValueError):
        Detector.load(bad)
    with pytest.raises(ValueError):   # the dataclass checks too, not only the reader
        dataclasses.replace(make_detector(), scaler_kind="minmax")
    with pytest.raises(ValueError):
        dataclasses.replace(make_detector(), latent_scorer="cen")


# ---------------------------------------------------------------------------
# standardisation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["standard", "minmax"])
def test_standardisation_matches_the_processor(tmp_path, kind):
    from fedmse_decentralized_amd.data.prepare import fitted_scaler_arrays

    rng = np.random.default_rng(11)
    D = 9
    fit = rng.normal(size=(200, D)) * rng.uniform(0.1, 30.0, size=D) + rng.normal(size=D)
    fit[:, 3] = 4.25                                      # a constant column
    fit[:, 6] = rng.uniform(1e15, 1e17, size=200)         # one huge-magnitude column
    proc = IoTDataProcessor(kind)
    proc.fit_transform(fit)
    X = rng.normal(size=(257, D)) * rng.uniform(0.1, 30.0, size=D) + rng.normal(size=D)
    X[:, 3] = 4.25
    X[5, 3] = 4.5
    X[:, 6] = rng.uniform(-1e17, 1e17, size=257)
    arrays = fitted_scaler_arrays(proc, kind)
    assert arrays.pop("kind") == kind
    dims = ModelDims(D, 3, 2)
    det = Detector(dims=dims, model_type="autoencoder", params=np.zeros(dims.num_params, np.float32),
                   scaler_kind=kind, scaler=arrays)
    det = Detector.load(det.save(str(tmp_path / "d.npz")))
    want = proc.transform(X)[0].astype(np.float32)
    assert same_bits(det.standardise(X), want)
    # fp32 raw rows are widened exactly first
    X32 = X.astype(np.float32)
    assert same_bits(det.standardise(X32), proc.transform(X32.astype(np.float64))[0].astype(np.float32))
    with pytest.raises(ValueError):
        det.standardise(X[:, :D - 1])


def test_scoring_rule_pieces():
    lat = np.array([[1.0, 2.0, -3.0], [np.nan, 0.0, 0.0], [np.inf, 1.0, 1.0]], dtype=np.float32)
    mean, scale = np.array([0.5, -1.0, 0.25]), np.array([2.0, 0.5, 3.0])
    s = cen_scores_stored(lat, mean, scale)
    t = ((lat[0].astype(np.float64) - mean).astype(np.float32).astype(np.float64) / scale).astype(np.float32)
    assert s[0] == np.sqrt(float(t[0]) ** 2 + float(t[1]) ** 2 + float(t[2]) ** 2)
    assert np.isnan(s[1]) and s[2] == np.inf
    c, f, a = clean_and_flag(np.array([np.nan, np.inf, -np.inf, 1.0, 2.0]), 1.0)
    assert c.tolist() == [0.0, DBL_MAX, -DBL_MAX, 1.0, 2.0] and f.tolist() == [0, 1, 0, 0, 1] and a == 2
    assert f.dtype == np.uint8
    c, f, a = clean_and_flag(np.array([np.inf, 1.0]), float("nan"))   # a NaN threshold flags nothing
    assert f.tolist() == [0, 0] and a == 0


@pytest.mark.parametrize("model_type,scorer", KINDS)
def test_torch_engine_score_rows(model_type, scorer):
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine

    det = make_detector(model_type, "minmax", scorer)
    other = make_detector(model_type, "standard", scorer, dims=ModelDims(6, 4, 3), seed=3)
    rng = np.random.default_rng(5)
    rows = [rng.normal(size=(37, 5)), rng.normal(size=(0, 6)), rng.normal(size=(12, 6)).astype(np.float32)]
    eng = TorchEngine(det.dims, torch.device("cpu"))
    out = eng.score_rows([det, other, other], rows, want_latents=True)
    for (s, f, a, lat), d, x in zip(out, [det, other, other], rows):
        n = x.shape[0]
        assert s.shape == (n,) and s.dtype == np.float64 and f.shape == (n,) and f.dtype == np.uint8
        assert a == int(f.sum()) and np.array_equal(f, (s > d.threshold).astype(np.uint8))
        assert (lat is None) == (model_type == "autoencoder")
        if lat is not None:
            assert lat.shape == (n, d.dims.latent) and lat.dtype == np.float32
        want = score_rows_numpy(d, x)
        assert same_bits(s, want[0]) and same_bits(f, want[1]) and a == want[2]
    assert len(eng.score_rows([det], [rows[0]])[0]) == 3
    with pytest.raises(ValueError):
        eng.score_rows([det], [rows[2]])


# ---------------------------------------------------------------------------
# a federation's bundles
# ---------------------------------------------------------------------------
def _small(orig):
    def resolved(self):
        s = orig(self)
        s.normal_rows, s.abnormal_rows, s.test_normal_rows = (60, 70), (80, 90), 15
        return s
    return resolved


@pytest.fixture
def shrunk(monkeypatch):
    """Small clients for this test only (the prepared-data cache holds data of the patched sizes)."""
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    monkeypatch.setattr(synthetic.SyntheticSpec, "resolved", _small(synthetic.SyntheticSpec.resolved))
    federation._PREP_CACHE.clear()
    yield
    federation._PREP_CACHE.clear()


def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=3, num_rounds=2, epoch=1, batch_size=12, output_root=out,
                backend="torch", device="cpu", log_level="WARNING", global_early_stop=False, save_checkpoints=False,
                compat="fixed", metric="detection", detect_quantile=0.9, export_detectors=True)
    base.update(kw)
    return ExperimentConfig(**base)


def raw_splits(cfg):
    """Every client's raw validation rows and raw test rows (with labels), in
    the federation's client order: the device sample and the permutations
    ``prepare_client`` draws, from the same seeds, applied to the same
    ``ClientRaw`` -- nothing is un-scaled."""
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
        out.append((raw.name, normal[tr:tr + va], np.concatenate(parts, 0), labels))
    return out


@pytest.mark.parametrize("scaler", ["standard", "minmax"])
@pytest.mark.parametrize("model_type,scorer", KINDS)
def test_exported_bundles_reproduce_the_last_round(tmp_path, shrunk, model_type, scorer, scaler):
    from fedmse_decentralized_amd.eval.metrics import calibration_rank
    from fedmse_decentralized_amd.federation import Federation

    cfg = _cfg(str(tmp_path), scaler=scaler, latent_scorer=scorer or "cen", knn_k=3)
    fed = Federation(cfg, model_type, "avg", 0).setup()
    rounds = []
    while True:
        r = fed.begin_step()
        if r is not None:
            rounds.append(r)
        if fed.end_step(r):
            break
    fed.conclude()
    assert len(rounds) == 2
    last = rounds[-1].detection
    splits = raw_splits(cfg)
    assert [s[0] for s in splits] == [c.name for c in fed.clients]
    for c, (name, valid_raw, test_raw, labels) in enumerate(splits):
        path = os.path.join(fed.save_dirs[c], "detector.npz")
        assert os.path.exists(path), path
        det = Detector.load(path)
        assert (det.model_type, det.scaler_kind, det.latent_scorer) == (model_type, scaler, scorer)
        assert det.dims == fed.dims and det.detect_quantile == 0.9
        assert det.provenance["client"] == name and det.provenance["update_type"] == "avg" \
            and det.provenance["rounds"] == "2"
        # the bundle's standardisation gives the rows the federation trained and evaluated on
        assert same_bits(det.standardise(valid_raw), fed.clients[c].valid)
        assert same_bits(det.standardise(test_raw), fed.clients[c].test)
        assert np.array_equal(labels, fed.clients[c].test_label)
        # threshold: the last round's, to the bit, and the rank rule on the raw validation rows
        assert same_bits(np.float64(det.threshold), np.float64(last["threshold"][c]))
        vs, vf, va = score_rows_numpy(det, valid_raw)
        assert det.threshold == np.sort(vs)[calibration_rank(vs.shape[0], 0.9)]
        assert va == int(np.sum(vs > det.threshold))
        # flags on the raw test rows: the round's counts
        s, f, a = fed.engine.score_rows([det], [test_raw])[0]
        y = labels != 0
        got = (int(np.sum(f[y])), int(np.sum(f[~y])), int(np.sum(1 - f[y])), int(np.sum(1 - f[~y])))
        want = tuple(int(last[k][c]) for k in ("tp", "fp", "fn", "tn"))
        assert got == want, (name, got, want)
        assert a == got[0] + got[1]


def test_flag_off_writes_no_bundle(tmp_path, shrunk):
    from fedmse_decentralized_amd.federation import Federation

    assert ExperimentConfig().export_detectors is False
    fed = Federation(_cfg(str(tmp_path), export_detectors=False, num_rounds=1), "autoencoder", "avg", 0).setup()
    fed.run_all()
    found = [f for _, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith(".npz")]
    assert found == []
    assert fed.clients[0].meta["scaler"]["kind"] == "standard"   # kept by prepare_client either way
    ns = add_arguments(argparse.ArgumentParser()).parse_args(["--export-detectors"])
    assert from_args(ns).export_detectors is True
    ns = add_arguments(argparse.ArgumentParser()).parse_args(["--export-detectors", "false"])
    assert from_args(ns).export_detectors is False


# ---------------------------------------------------------------------------
# the command-line tool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("as_dir", [False, True])
def test_cli_on_the_torch_backend(tmp_path, capsys, as_dir):
    from fedmse_decentralized_amd import detect

    det = make_detector("hybrid", "standard", "cen", threshold=1.5)
    bundle = det.save(str(tmp_path / "detector.npz"))
    rng = np.random.default_rng(2)
    rows = rng.normal(size=(41, 5)) * 3.0
    src = tmp_path / "traffic"
    src.mkdir()
    np.savetxt(str(src / "a.csv"), rows[:30], delimiter=",", fmt="%.17g")
    np.savetxt(str(src / "b.csv"), rows[30:], delimiter=",", fmt="%.17g")
    inp, n = (str(src), 41) if as_dir else (str(src / "a.csv"), 30)
    out = str(tmp_path / "alarms.npz")
    assert detect.main(["--detector", bundle, "--input", inp, "--output", out, "--backend", "torch"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    want = score_rows_numpy(det, rows[:n])
    words = line.split()
    assert words[0] == "detect:" and words[words.index("rows") + 1] == str(n)
    assert words[words.index("alarms") + 1] == str(want[2]) and "rows_per_s" in words
    with np.load(out, allow_pickle=False) as z:
        assert same_bits(z["scores"], want[0]) and same_bits(z["flags"], want[1])
        assert int(z["alarms"]) == want[2] and float(z["threshold"]) == 1.5
    with pytest.raises(FileNotFoundError):
        detect.main(["--detector", bundle, "--input", str(tmp_path / "missing.csv"), "--backend", "torch"])
