"""Experiment configuration.

Same knobs, names and defaults as the module constants of the reference
driver (`src/main.py:37-71`), plus the protocol constants that the
reference hard-codes in ``ClientTrainer``/``ModelVerifier``
(`src/Trainer/client_trainer.py:47-95`, `src/Trainer/model_verifier.py:14`)
and the new framework's own switches (backend, compat mode, sharding,
synthetic data).  Every field can be overridden from the command line
(``main.py --help``).
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
from dataclasses import dataclass, field
from typing import List, Optional

DEFAULT_EXP_TEMPLATE = (
    "nonIID_Exp21_Rerun_{epoch}epoch_10client_lr0001_lamda{shrink_lambda}_ratio{ratio}"
)


LATENT_SCORERS = ("cen", "knn")
KNN_MAX_K = 16   # neighbours the kNN scorer's kernel keeps in registers


@dataclass
class ExperimentConfig:
    # --- reference constants (src/main.py:37-71) --------------------------
    num_participants: float = 0.5
    epoch: int = 5
    num_rounds: int = 3
    lr_rate: float = 1e-3
    shrink_lambda: float = 5
    network_size: int = 10
    data_seed: int = 1234
    no_exp: Optional[str] = None
    verification_method: str = "val"     # "val" | "dev"
    num_runs: int = 1
    batch_size: int = 12
    new_device: bool = True
    global_patience: int = 1
    metric: str = "AUC"                  # "AUC" | "classification" | "time" | "detection" | "tpr_at_fpr"
    model_types: List[str] = field(default_factory=lambda: ["hybrid", "autoencoder"])
    update_types: List[str] = field(default_factory=lambda: ["avg", "fedprox", "mse_avg"])
    dim_features: int = 115
    scen_name: str = "FL-IoT"
    config_file: str = "Configuration/kitsune-iot-10clients.json"
    # --- ClientTrainer / ModelVerifier constants --------------------------
    hidden_neus: int = 27
    latent_dim: int = 7
    fedprox_mu: float = 0.001
    verification_threshold: float = 3.0
    performance_threshold: float = 0.002
    # > 0 (fixed-mode option, not the reference): the verifier's drift limit is
    #   RELATIVE, drift <= drift_threshold_rel x sum_tensors ||history||_2,
    #   instead of the absolute verification_threshold.  The absolute 3.0
    #   (model_verifier.py:72-75) was tuned for the reference's 10 clients;
    #   a large federation's early aggregates move further and were rejected
    #   by nearly every receiver (profiles/r4_adoption_ablation.md).
    drift_threshold_rel: float = 0.0
    max_aggregation: int = 3
    max_rejected_updates: int = 3
    vote_batch_size: int = 128
    scaler: str = "standard"
    # --- new-framework switches -------------------------------------------
    compat: str = "reference"            # "reference" (reproduce quirks) | "fixed"
    backend: str = "auto"                # "auto" | "hip" | "torch"
    device: str = "auto"                 # "auto" | "cpu" | "cuda"
    synthetic: Optional[str] = None      # None (CSV via config_file) | "nbaiot" | "kitsune"
    synthetic_iid: bool = True
    synthetic_alpha: Optional[float] = None
    synthetic_seed: int = 2025
    output_root: str = "."
    save_checkpoints: bool = True        # model.cpt / training_tracking.pkl per client
    save_latents: bool = False           # LatentData pickles
    global_early_stop: bool = True
    trace_file: Optional[str] = None     # per-phase JSONL telemetry
    resume: Optional[str] = None         # resume snapshot path
    snapshot_every: int = 0              # write a resume snapshot every k rounds (0 = never)
    log_level: str = "INFO"
    malicious_clients: List[int] = field(default_factory=list)  # fault injection (tests)
    malicious_scale: float = 10.0
    dropped_clients: List[int] = field(default_factory=list)    # fault injection: never vote / aggregate
    # update type "trimmed_mean": per coordinate, the floor(ratio * k) lowest and
    # as many highest of the k selected models' values are dropped before the
    # mean (at most (k - 1) // 2 per side; protocol/aggregation.py trim_count).
    # "krum" / "multi_krum": the share of the selected models assumed poisoned,
    # f = floor(ratio * k), at most (k - 3) // 2 (krum_counts)
    robust_trim_ratio: float = 0.2
    # update type "geomed": smoothed Weiszfeld iterations towards the geometric
    # median of the selected models (0..64; 0 is the mean over the rows without
    # NaN / infinity) and the smoothing, a finite distance > 0 below which a
    # model's weight stops growing (protocol/aggregation.py geomed_check)
    geomed_iters: int = 3
    geomed_nu: float = 1e-6
    # metric "detection": the alarm threshold is the smallest validation score
    # (the client's own held-back normal rows, under the evaluated model) with
    # at least this share of them at or below it; in (0, 1]
    detect_quantile: float = 0.95
    # metric "tpr_at_fpr": the threshold is that quantile, 1 - target_fpr, of
    # the test set's normal scores, and the metric the recall there; in [0, 1)
    target_fpr: float = 0.01
    # what scores a ``hybrid`` model's latents (README "Latent scorers"): "cen",
    # the reference's distance to the train latents' centroid, or "knn", the
    # distance to the knn_k-th nearest train latent (1 <= knn_k <= 16);
    # ``autoencoder`` models score by reconstruction error and ignore both
    latent_scorer: str = "cen"
    knn_k: int = 5
    # at the end of a combination, write every hosted client's deployable
    # detector (deploy/detector.py: model, feature scaler, latent scorer state,
    # threshold at detect_quantile) as detector.npz beside its model.cpt
    export_detectors: bool = False
    # with export_detectors: also record in each bundle what "normal" looked
    # like (README "Monitoring a deployed detector"): the band of the
    # standardised train features and monitor_bins - 1 edges, order statistics
    # of the validation scores, with the scores' own bin counts (2..16 bins)
    export_baseline: bool = False
    monitor_bins: int = 10
    # --- protocol variants ---------------------------------------------------
    # "first_voter": the reference's decentralised election (first selected
    #   voter that finds an eligible candidate decides, client_trainer.py:249-285);
    # "majority": the legacy centralised GlobalAggregator.select_aggregator
    #   (every selected client votes, most votes wins).
    election: str = "first_voter"
    # "decentralized": receivers verify the broadcast aggregate (reference);
    # "centralized": server push, every client adopts the aggregate (legacy
    #   GlobalAggregator.update);
    # "local": ablation, no aggregation at all (selected clients train, every
    #   client is evaluated; profiles/r4_adoption_ablation.md).
    aggregation_mode: str = "decentralized"
    # "code": ModelVerifier rule (drift <= 3.0 and dperf >= -0.002);
    # "thesis": the thesis variant (Thesis p.20-26): loss-ratio acceptance
    #   new <= old * (1 + thesis_loss_ratio) with a NaN/inf check, candidates
    #   with vote MSE > thesis_vote_mse_cap are not voted for, and a random
    #   eligible aggregator is used when no valid one exists.
    protocol_variant: str = "code"
    thesis_loss_ratio: float = 0.1
    thesis_vote_mse_cap: float = 3.0
    # initial client models: "per_client" builds one independently initialised
    #   model per client (the reference, src/main.py:228-236); "shared" gives
    #   every client a copy of client 0's initial model (one global init, as
    #   the FedMSE paper's server does).  "auto": per_client under
    #   compat=reference, shared under compat=fixed — averaging k independent
    #   inits cancels the latent layer by ~sqrt(k), which large federations
    #   never recover from (profiles/r3_collapse_diag.md).
    init_mode: str = "auto"
    fusion_max_rows: int = 1024          # dev rows used by the fusion_avg KDE similarity
    fedavg_sample_weighted: bool = False  # FedAvg weights ∝ training-set size (reference: plain mean, Q13)
    # experiment-level parallelism: with N ranks, combination
    # i of the model_type x update_type x run sweep runs on rank i % N (each
    # as a single-rank federation on that rank's GPU) instead of every
    # combination being sharded over all ranks.
    parallel_combos: bool = False
    # one process, one GPU: build every combination's federation up front and
    # run their rounds interleaved, each federation on its own HIP stream and
    # launch rings (ops/_hip.Runtime(private=True)), so their kernels overlap
    # on the GPU's idle CUs and one federation's host work overlaps another's
    # GPU work.  compat=fixed only (the reference's global early-stop state is
    # shared across combinations in sequence); reports and the
    # summary are identical to the sequential sweep.
    concurrent_combos: bool = False
    # fixed compat + HIP engine: run the round's protocol decisions on the
    # device (engine/device_round.py) so rounds need no host synchronisation
    device_protocol: bool = True
    # debug: all-gather a hash of the replicated protocol state every round
    # and fail on divergence between ranks
    debug_replica_check: bool = False
    # multi-rank transport of the device protocol's per-round collectives:
    # "rccl" (torch.distributed: RCCL on the GPU) or "ipc" (one-shot kernels
    # over peer-mapped memory, parallel/ipc.py; SURVEY §5.8's --comm ipc|rccl);
    # None: FEDMX_COMM, else rccl
    comm: Optional[str] = None

    # -----------------------------------------------------------------------
    @property
    def experiment_name(self) -> str:
        if self.no_exp:
            return self.no_exp
        return DEFAULT_EXP_TEMPLATE.format(
            epoch=self.epoch, shrink_lambda=_fmt_num(self.shrink_lambda), ratio=self.num_participants * 100,
            network_size=self.network_size, num_rounds=self.num_rounds, lr_rate=self.lr_rate,
            data_seed=self.data_seed)

    @property
    def checkpoint_dir(self) -> str:
        return os.path.join(self.output_root, f"Checkpoint/Results/Update/{self.network_size}/{self.experiment_name}")

    def client_save_dir(self, run: int, model_type: str, update_type: str, device_name: str) -> str:
        return os.path.join(self.output_root, f"Checkpoint/{self.network_size}/{self.experiment_name}/{run}/ClientModel",
                            self.scen_name, model_type, update_type, device_name)

    def __post_init__(self):
        # fixed-mode-only options (the reference's rules otherwise): the
        # relative drift rule replaces model_verifier.py:72-75's absolute 3.0
        if self.drift_threshold_rel > 0 and self.compat != "fixed":
            raise ValueError("drift_threshold_rel > 0 replaces the reference's absolute drift rule "
                             "(src/Trainer/model_verifier.py:72-75): it needs compat='fixed'")
        if not 0.0 < self.detect_quantile <= 1.0:
            raise ValueError(f"detect_quantile must lie in (0, 1], got {self.detect_quantile!r}")
        if not 0.0 <= self.target_fpr < 1.0:
            raise ValueError(f"target_fpr must lie in [0, 1), got {self.target_fpr!r}")
        if self.latent_scorer not in LATENT_SCORERS:
            raise ValueError(f"latent_scorer must be one of {' | '.join(LATENT_SCORERS)}, got {self.latent_scorer!r}")
        if isinstance(self.knn_k, bool) or not isinstance(self.knn_k, int) or not 1 <= self.knn_k <= KNN_MAX_K:
            raise ValueError(f"knn_k must be an integer in 1..{KNN_MAX_K}, got {self.knn_k!r}")
        if isinstance(self.monitor_bins, bool) or not isinstance(self.monitor_bins, int) \
                or not 2 <= self.monitor_bins <= 16:
            raise ValueError(f"monitor_bins must be an integer in 2..16, got {self.monitor_bins!r}")
        from .protocol.aggregation import geomed_check

        geomed_check(self.geomed_iters, self.geomed_nu)
        if self.export_baseline and not self.export_detectors:
            raise ValueError("export_baseline records the baseline in the exported bundles: it needs export_detectors")

    def resolved_init_mode(self) -> str:
        if self.init_mode == "auto":
            return "per_client" if self.compat == "reference" else "shared"
        if self.init_mode not in ("per_client", "shared"):
            raise ValueError(f"init_mode must be auto | per_client | shared, got {self.init_mode!r}")
        return self.init_mode

    def resolved_device(self) -> str:
        if self.device == "auto":
            import torch

            return "cuda" if torch.cuda.is_available() else "cpu"
        return self.device

    def to_json(self) -> str:
        return json.dumps(dataclasses.asdict(self), indent=2, sort_keys=True)


def _fmt_num(v):
    # the reference formats shrink_lambda as an int literal (5, 10)
    if isinstance(v, float) and v.is_integer():
        return int(v)
    return v


def _str2bool(s):
    if isinstance(s, bool):
        return s
    return s.lower() in ("1", "true", "yes", "y", "on")


_HELP = {
    "metric": "AUC | classification (F1 at score > 0.5) | time | detection (F1 at the threshold calibrated on "
              "each client's validation scores, --detect-quantile) | tpr_at_fpr (recall at the threshold that "
              "leaves --target-fpr of the normal test rows flagged)",
    "detect_quantile": "metric detection: quantile of a client's validation scores used as its alarm "
                       "threshold, in (0, 1] (default 0.95)",
    "target_fpr": "metric tpr_at_fpr: false-positive rate on the normal test rows at which recall is "
                  "reported, in [0, 1) (default 0.01)",
    "latent_scorer": "what scores a hybrid model's latents: cen (distance to the train latents' centroid, the "
                     "reference) | knn (distance to the --knn-k-th nearest train latent); autoencoder models "
                     "ignore it (default cen)",
    "export_detectors": "write each hosted client's deployable detector (detector.npz: model, feature scaler, "
                        "latent scorer state, threshold at --detect-quantile) beside its model.cpt when the "
                        "combination ends; score traffic with python -m fedmse_decentralized_amd.detect "
                        "(default false)",
    "export_baseline": "with --export-detectors: also record the monitoring baseline in each detector.npz (band of "
                       "the standardised train features, score edges and counts; python -m "
                       "fedmse_decentralized_amd.detect --monitor compares live traffic with it) (default false)",
    "monitor_bins": "--export-baseline: number of score bins of the baseline, 2..16 (default 10)",
    "knn_k": "latent scorer knn: which nearest train latent's distance is the score, 1..16 (default 5)",
    "update_types": "any of: avg fedprox mse_avg fusion_avg trimmed_mean median krum multi_krum geomed",
    "robust_trim_ratio": "share of the selected models assumed poisoned, in [0, 0.5): trimmed_mean drops that "
                         "fraction at each end of every coordinate's order, krum / multi_krum discard that "
                         "fraction of whole models by distance (default 0.2)",
    "geomed_iters": "update type geomed: smoothed Weiszfeld iterations towards the geometric median of the "
                    "selected models, 0..64 (0: the mean of the models without NaN / infinity; default 3)",
    "geomed_nu": "update type geomed: smoothing of the Weiszfeld weights 1 / max(distance, nu), finite and > 0 "
                 "(default 1e-6)",
}


def add_arguments(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    d = ExperimentConfig()
    for f in dataclasses.fields(ExperimentConfig):
        name = "--" + f.name.replace("_", "-")
        default = getattr(d, f.name)
        if isinstance(default, bool):
            # (`--flag` alone reads as `--flag true`)
            p.add_argument(name, type=_str2bool, nargs="?", const=True, default=None, metavar="BOOL",
                           help=_HELP.get(f.name))
        elif isinstance(default, list):
            elem = int if f.name in ("malicious_clients", "dropped_clients") else str
            p.add_argument(name, type=elem, nargs="*", default=None, help=_HELP.get(f.name))
        elif isinstance(default, int) and not isinstance(default, bool):
            p.add_argument(name, type=int, default=None, help=_HELP.get(f.name))
        elif isinstance(default, float):
            p.add_argument(name, type=float, default=None, help=_HELP.get(f.name))
        elif default is None and str(f.type) in ("Optional[float]", "float"):   # e.g. synthetic_alpha
            p.add_argument(name, type=float, default=None)
        elif default is None and str(f.type) in ("Optional[int]", "int"):
            p.add_argument(name, type=int, default=None)
        else:
            p.add_argument(name, type=str, default=None, help=_HELP.get(f.name))
    # reference spelling alias
    p.add_argument("--no-Exp", dest="no_exp", type=str, default=None)
    return p


def from_args(ns: argparse.Namespace, base: Optional[ExperimentConfig] = None) -> ExperimentConfig:
    cfg = base or ExperimentConfig()
    kw = {}
    for f in dataclasses.fields(ExperimentConfig):
        v = getattr(ns, f.name, None)
        if v is not None:
            kw[f.name] = v
    return dataclasses.replace(cfg, **kw)


# --- device-list JSON (src/Configuration/*.json) ---------------------------

@dataclass
class DeviceEntry:
    id: int
    name: str
    normal_data_path: str
    abnormal_data_path: str
    test_normal_data_path: Optional[str] = None


@dataclass
class DeviceListConfig:
    data_path: str
    devices_list: List[DeviceEntry]
    base_dir: str = "."

    def resolve(self, rel: str) -> str:
        p = os.path.join(self.data_path, rel)
        if not os.path.isabs(p):
            p = os.path.join(self.base_dir, p)
        return os.path.normpath(p)


def load_device_list(path: str, base_dir: Optional[str] = None) -> DeviceListConfig:
    """Load a reference device-list JSON verbatim.

    ``data_path`` is relative to the directory the reference is run from
    (``src/``); by default it is resolved relative to the JSON's parent's
    parent (``src/Configuration/x.json`` -> ``src/``), which reproduces that.
    """
    with open(path, "r") as f:
        raw = json.load(f)
    if base_dir is None:
        base_dir = os.path.dirname(os.path.dirname(os.path.abspath(path)))
    devs = []
    for d in raw["devices_list"]:
        devs.append(DeviceEntry(
            id=int(d.get("id", len(devs) + 1)), name=d["name"],
            normal_data_path=d["normal_data_path"], abnormal_data_path=d["abnormal_data_path"],
            test_normal_data_path=d.get("test_normal_data_path")))
    return DeviceListConfig(data_path=raw["data_path"], devices_list=devs, base_dir=base_dir)
