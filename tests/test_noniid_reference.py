"""The reference's own N-BaIoT non-IID device list (VERDICT r4 Next #2).

The reference's `src/Configuration/scen2-nba-iot-10clients_noniid.json`
lists ten clients; clients 6, 9 and 10 ship without ``abnormal/`` data
(its `.MISSING_LARGE_BLOBS:4-6`).  tests/golden/reference holds the device
lists as shipped and the first rows of every CSV they name that ships
(conftest's ``reference_root`` unpacks them).  The loader accepts them: they
train, vote and verify like the others, and since their test sets hold normal
rows only their AUC is undefined -- written as null in the per-round report
and left out of every mean / min / max (global early stop, the summary's
best metric).  CPU engine, two rounds.
"""
import json
import os

import numpy as np
import pytest

REF_CFG = "src/Configuration/scen2-nba-iot-10clients_noniid.json"
MISSING = {"NBa-Scen2-Client-6", "NBa-Scen2-Client-9", "NBa-Scen2-Client-10"}


def test_noniid_device_list_with_abnormal_less_clients(tmp_path, reference_root):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.config import ExperimentConfig
    from fedmse_decentralized_amd.federation import Federation, metric_stats

    federation._PREP_CACHE.clear()
    cfg = ExperimentConfig(config_file=os.path.join(reference_root, REF_CFG), network_size=10, num_rounds=2,
                           epoch=1, lr_rate=1e-3, shrink_lambda=1, output_root=str(tmp_path), backend="torch", device="cpu",
                           compat="fixed", global_early_stop=False, save_checkpoints=False, log_level="WARNING",
                           model_types=["hybrid"], update_types=["mse_avg"])
    fed = Federation(cfg, "hybrid", "mse_avg", 0).setup()
    names = [c.name for c in fed.clients]
    # the reference's device sampling order (random.Random(1234).sample, src/main.py:116,126)
    assert [n.split("-")[-1] for n in names] == ["8", "2", "1", "10", "5", "7", "6", "4", "9", "3"]
    for c in fed.clients:
        if c.name in MISSING:
            assert c.n_abnormal == 0 and int(c.test_label.sum()) == 0
        else:
            assert c.n_abnormal > 0
    rs = [fed.run_round() for _ in range(2)]
    fed.finish()
    fed.writer.flush()
    for r in rs:
        m = np.asarray(r.metrics, dtype=np.float64)
        undefined = {names[i] for i in np.flatnonzero(np.isnan(m))}
        assert undefined == MISSING
        mean, lo, hi = metric_stats(m)
        assert 0.5 < lo <= mean <= hi <= 1.0
    path = os.path.join(cfg.checkpoint_dir, "Run_0", "AUC", "FL-IoT_0.5_hybrid_mse_avg_results.json")
    rows = [json.loads(line) for line in open(path)]
    assert [r["round"] for r in rows] == [1, 2]
    for r in rows:
        vals = r["client_metrics"]
        assert {names[i] for i, v in enumerate(vals) if v is None} == MISSING
        assert r["global_loss"] == min(v for v in vals if v is not None)


KIT_CFG = "src/Configuration/kitsune-iot-10clients_noniid.json"


def test_kitsune_noniid_device_list_missing_clients(tmp_path, reference_root):
    """VERDICT r5 Next #6b: the Kitsune non-IID list.  Client 5 ships without
    ``abnormal/`` (loads; AUC null), client 7 without ``abnormal/`` and
    ``normal/`` (no training data: the loader names the missing directory).
    The list without client 7 -- the run of profiles/r6_noniid_kitsune.md
    uses the 8 complete clients -- trains one round on the CPU engine."""
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.config import ExperimentConfig
    from fedmse_decentralized_amd.federation import Federation

    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    from noniid_supervised_ceiling import derived_config

    kit_cfg = os.path.join(reference_root, KIT_CFG)
    full = derived_config(kit_cfg, [])
    with pytest.raises(FileNotFoundError, match="Client-7/normal"):
        federation._PREP_CACHE.clear()
        Federation(ExperimentConfig(config_file=full, network_size=10, output_root=str(tmp_path / "a"),
                                    backend="torch", device="cpu", log_level="WARNING"), "hybrid", "avg", 0).setup()
    os.unlink(full)
    path = derived_config(kit_cfg, [7])
    try:
        federation._PREP_CACHE.clear()
        cfg = ExperimentConfig(config_file=path, network_size=9, num_rounds=1, epoch=1, lr_rate=1e-3,
                               shrink_lambda=1, output_root=str(tmp_path / "b"), backend="torch", device="cpu",
                               compat="fixed", global_early_stop=False, save_checkpoints=False,
                               log_level="WARNING", model_types=["hybrid"], update_types=["avg"])
        fed = Federation(cfg, "hybrid", "avg", 0).setup()
        by_name = {c.name: c for c in fed.clients}
        assert len(by_name) == 9 and "Kitsune-Client-7" not in by_name
        assert by_name["Kitsune-Client-5"].n_abnormal == 0
        assert all(c.n_abnormal > 0 for n, c in by_name.items() if n != "Kitsune-Client-5")
        r = fed.run_round()
        m = np.asarray([np.nan if v is None else v for v in r.metrics], dtype=np.float64)
        pos5 = [c.name for c in fed.clients].index("Kitsune-Client-5")
        assert np.isnan(m[pos5]) and np.all(np.isfinite(np.delete(m, pos5)))
        fed.finish()
    finally:
        os.unlink(path)
