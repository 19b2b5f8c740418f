"""End-to-end federation on CPU (BASELINE config 1 plumbing): report schemas,
checkpoint artefacts, resume, determinism across in-process ranks, fault
injection."""
import json
import os
import threading

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.config import ExperimentConfig
from fedmse_decentralized_amd.federation import Federation
from fedmse_decentralized_amd.parallel.comm import ThreadComm

SMALL = dict(normal_rows=(90, 100), abnormal_rows=(120, 130), test_normal_rows=20)


def _cfg(tmp_path, **kw):
    base = dict(synthetic="nbaiot", network_size=4, num_rounds=3, epoch=2, batch_size=12,
                output_root=str(tmp_path), backend="torch", device="cpu", log_level="WARNING",
                model_types=["hybrid"], update_types=["mse_avg"])
    base.update(kw)
    return ExperimentConfig(**base)


@pytest.fixture(autouse=True)
def _small_synthetic(monkeypatch):
    # shrink the synthetic clients so CPU tests stay fast
    from fedmse_decentralized_amd.data import synthetic

    orig = synthetic.SyntheticSpec.resolved

    def resolved(self):
        s = orig(self)
        s.normal_rows, s.abnormal_rows, s.test_normal_rows = SMALL["normal_rows"], SMALL["abnormal_rows"], \
            SMALL["test_normal_rows"]
        return s
    monkeypatch.setattr(synthetic.SyntheticSpec, "resolved", resolved)
    from fedmse_decentralized_amd import federation
    federation._PREP_CACHE.clear()


def test_reports_and_artifacts(tmp_path):
    cfg = _cfg(tmp_path, global_early_stop=False)
    fed = Federation(cfg, "hybrid", "mse_avg", 0).setup()
    best = fed.run_all()
    assert 0.5 < best <= 1.0
    res = os.path.join(cfg.checkpoint_dir, "Run_0", "AUC", "FL-IoT_0.5_hybrid_mse_avg_results.json")
    lines = [json.loads(l) for l in open(res)]
    assert [l["round"] for l in lines] == [1, 2, 3]
    for l in lines:
        assert set(l) == {"round", "client_metrics", "update_type", "model_type", "global_loss"}
        assert len(l["client_metrics"]) == 4 and l["global_loss"] == min(l["client_metrics"])
    ver = [json.loads(l) for l in open(os.path.join(cfg.checkpoint_dir, "Run_0", "verification_results.json"))]
    for v in ver:
        assert len(v["verification_results"]) == 3     # everyone but the aggregator
        for r in v["verification_results"]:
            assert set(r) == {"client_id", "rejected_updates", "is_verified"}
    # model.cpt of every client trained at least once, loadable with weights_only
    cpts = []
    for root, _, files in os.walk(os.path.join(str(tmp_path), "Checkpoint", "4")):
        if "model.cpt" in files:
            cpts.append(os.path.join(root, "model.cpt"))
    assert cpts
    sd = torch.load(cpts[0], weights_only=True)
    assert list(sd.keys())[0] == "encoder.encoder_network.0.weight" and sd[list(sd.keys())[0]].shape == (27, 115)


def test_model_cpt_bytes_match_reference_writer(tmp_path):
    from fedmse_decentralized_amd.io.checkpoint import save_model_cpt
    from fedmse_decentralized_amd.models.layout import canonical_to_padded, state_dict_to_canonical
    from fedmse_decentralized_amd.models.reference import ReferenceSAE

    m = ReferenceSAE()
    ref = tmp_path / "ref.cpt"
    torch.save(m.state_dict(), ref, _use_new_zipfile_serialization=False)
    ours = save_model_cpt(str(tmp_path / "ours"), canonical_to_padded(state_dict_to_canonical(m.state_dict())))
    # the legacy format keys (and orders) storages by memory address, so two
    # saves of the same state differ only there: compare size, pickle header
    # and content
    ra, rb_ = open(ours, "rb").read(), open(ref, "rb").read()
    assert len(ra) == len(rb_) and ra[:200] == rb_[:200]
    a = torch.load(ours, weights_only=True)
    b = torch.load(ref, weights_only=True)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("compat,variant", [("reference", "code"), ("fixed", "code"), ("fixed", "thesis")])
def test_resume_reproduces_trajectory(tmp_path, compat, variant):
    """Resume from a per-round snapshot: both the reference-RNG replay and the
    fixed mode's seeded tie-break noise stream continue where they stopped."""
    cfg = _cfg(tmp_path, global_early_stop=False, num_rounds=4, save_checkpoints=False, compat=compat,
               protocol_variant=variant)
    a = Federation(cfg, "hybrid", "avg", 0).setup()
    for _ in range(2):
        a.run_round()
    snap = a.save_snapshot(str(tmp_path / "snap.pt"))
    noise_at_snap = a.noise.get_state() if compat == "fixed" else None
    fb_at_snap = a.fallback_rng.getstate() if variant == "thesis" else None
    ra = [a.run_round().metrics for _ in range(2)]
    cfg2 = _cfg(tmp_path, global_early_stop=False, num_rounds=4, save_checkpoints=False, resume=snap, compat=compat,
                protocol_variant=variant)
    b = Federation(cfg2, "hybrid", "avg", 0).setup()
    assert b.round_idx == 2
    if compat == "fixed":
        assert b.noise.get_state() == noise_at_snap
    if variant == "thesis":
        assert b.fallback_rng.getstate() == fb_at_snap
    rb = [b.run_round().metrics for _ in range(2)]
    for x, y in zip(ra, rb):
        np.testing.assert_array_equal(x, y)


def _run_threads(world, cfg, rounds):
    comms = ThreadComm.group(world)
    out = [None] * world
    errs = []

    def worker(r):
        try:
            f = Federation(cfg, "hybrid", "mse_avg", 0, comm=comms[r], device=torch.device("cpu")).setup()
            out[r] = [f.run_round() for _ in range(rounds)] + [f.engine.store.params.clone(), f.local]
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append(traceback.format_exc())
            for c in comms:
                c.g.barrier.abort()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs[0]
    return out


@pytest.mark.parametrize("compat", ["reference", "fixed"])
def test_sharded_federation_matches_single_rank(tmp_path, compat):
    cfg = _cfg(tmp_path, global_early_stop=False, save_checkpoints=False, compat=compat, network_size=5)
    single = _run_threads(1, cfg, 3)[0]
    for world in (2, 3):
        outs = _run_threads(world, cfg, 3)
        for r in range(3):
            for o in outs:
                assert o[r].aggregator == single[r].aggregator
                assert o[r].selected == single[r].selected
                np.testing.assert_array_equal(o[r].metrics, single[r].metrics)
        # every rank's shard equals the same clients' params of the single-rank run
        for o in outs:
            params, local = o[3], o[4]
            assert torch.equal(params, single[3][local[0]:local[-1] + 1])


def test_malicious_client_gets_rejected(tmp_path):
    cfg = _cfg(tmp_path, global_early_stop=False, save_checkpoints=False, num_participants=1.0, network_size=3,
               malicious_clients=[0, 1, 2], malicious_scale=50.0, num_rounds=3, update_types=["avg"])
    fed = Federation(cfg, "hybrid", "avg", 0).setup()
    results = [fed.run_round() for _ in range(3)]
    later = [v for r in results[1:] for v in r.verification]
    assert any(not v["is_verified"] for v in later)


def test_global_early_stop_compat(tmp_path):
    cfg = _cfg(tmp_path, num_rounds=10, save_checkpoints=False)
    fed = Federation(cfg, "hybrid", "avg", 0).setup()
    fed.run_all()
    assert fed.round_idx < 10   # AUC compared like a loss stops early (Q8)


def test_fast_model_cpt_writer(tmp_path):
    from fedmse_decentralized_amd.io.checkpoint import save_model_cpt_fast
    from fedmse_decentralized_amd.models.layout import state_dict_to_canonical
    from fedmse_decentralized_amd.models.reference import ReferenceSAE

    m = ReferenceSAE()
    ref = tmp_path / "ref.cpt"
    torch.save(m.state_dict(), ref, _use_new_zipfile_serialization=False)
    p = save_model_cpt_fast(str(tmp_path / "fast"), state_dict_to_canonical(m.state_dict()).numpy())
    # sizes may differ by a few bytes: legacy storage keys are decimal addresses
    assert abs(os.path.getsize(p) - os.path.getsize(ref)) <= 64
    a = torch.load(p, weights_only=True)
    b = torch.load(ref, weights_only=True)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert open(p, "rb").read() == open(save_model_cpt_fast(str(tmp_path / "again"),
                                                           state_dict_to_canonical(m.state_dict()).numpy()),
                                         "rb").read()


def test_csv_config_path_end_to_end(tmp_path):
    """Synthetic dataset written in the reference's on-disk layout, loaded
    through the device-list JSON + CSV reader path."""
    from fedmse_decentralized_amd.data.synthetic import SyntheticSpec, write_dataset

    spec = SyntheticSpec(kind="nbaiot", n_clients=3, seed=5, normal_rows=(60, 70), abnormal_rows=(80, 90),
                         test_normal_rows=15)
    path = write_dataset(str(tmp_path / "ds"), spec)
    cfg = _cfg(tmp_path, synthetic=None, config_file=path, network_size=3, num_rounds=2, global_early_stop=False,
               save_checkpoints=False)
    fed = Federation(cfg, "hybrid", "avg", 0).setup()
    assert len(fed.clients) == 3
    r = fed.run_round()
    assert r.metrics.shape == (3,) and np.all((r.metrics >= 0) & (r.metrics <= 1))


def test_replica_check_passes_and_detects_divergence(tmp_path):
    cfg = _cfg(tmp_path, global_early_stop=False, save_checkpoints=False, network_size=4, debug_replica_check=True)
    outs = _run_threads(2, cfg, 2)          # identical replicas: the check passes every round
    assert outs[0][0].aggregator == outs[1][0].aggregator
    fed = Federation(cfg, "hybrid", "avg", 0).setup()
    comms = ThreadComm.group(2)
    errs = []

    def worker(r):
        f = Federation(cfg, "hybrid", "avg", 0, comm=comms[r], device=torch.device("cpu")).setup()
        try:
            f.check_replicas(0, [0, 1], r, np.zeros(4))   # rank-dependent aggregator
        except RuntimeError as e:
            errs.append(str(e))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert len(errs) == 2 and "diverged" in errs[0]


def test_baseline_config1_reference_csvs_cpu(tmp_path, reference_root):
    """BASELINE.json config 1: 2-client SAE FedAvg on CPU from the reference's
    own scen2 N-BaIoT device list and the first rows of the two sampled
    clients' CSVs (tests/golden/reference), through main.run_sweep."""
    import main as driver

    ref_cfg = os.path.join(reference_root, "src/Configuration/scen2-nba-iot-10clients.json")
    cfg = ExperimentConfig(config_file=ref_cfg, network_size=2, num_rounds=2, epoch=1, batch_size=12,
                           model_types=["hybrid"], update_types=["avg"], backend="torch", device="cpu",
                           output_root=str(tmp_path), log_level="WARNING", save_checkpoints=False)
    best = driver.run_sweep(cfg)
    assert 0.5 < best["hybrid"]["avg"] <= 1.0
    summ = json.load(open(os.path.join(cfg.checkpoint_dir, "training_summary.json")))
    assert summ["best_metrics"]["hybrid"]["avg"] == best["hybrid"]["avg"]
