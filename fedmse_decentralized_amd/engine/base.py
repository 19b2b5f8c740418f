"""Engine interface and the device-resident client store.

An *engine* owns the clients hosted by one rank (one GPU): their datasets,
parameters and optimiser state, all resident on the device in
structure-of-arrays form, and exposes the compute the federated protocol
needs.  Two levels:

Primitives
  * ``train_launch`` / ``train_collect`` – local training of a set of clients
    (reference ``ClientTrainer.run``, `src/Trainer/client_trainer.py:360-419`);
  * ``forward_rows``   – per-row squared reconstruction error and/or latents of
    (parameter-vector, dataset) pairs (`client_trainer.py:208-247`, `:115-130`,
    `src/Trainer/model_verifier.py:86-99`, `src/Evaluator/evaluator.py:52-94`);
  * ``weighted_sum``   – FedAvg / MSEAvg reduction (`client_trainer.py:107-134`);
  * ``param_drift``    – verifier drift (`model_verifier.py:79-84`);
  * ``cen_scores`` + ``auc`` – SAE-CEN scoring and ROC-AUC
    (`src/Model/Centroid.py:15-35`, `src/Evaluator/evaluator.py:21-28`).

Round operations (what the federation calls; results stay on the device
until one ``fetch`` per protocol phase):
  * ``vote_scores`` – vote score on the standardised vote data + dev-set MSE
    for each given client;
  * ``verify_stats`` – MSE of the aggregate on the verification sets + drift
    against the previously received aggregates;
  * ``adopt`` – copy the aggregate into accepted clients (+ FedProx anchor);
  * ``evaluate`` – detection metric of every hosted client.

``TorchEngine`` implements the primitives with reference-exact PyTorch math;
``HipEngine`` runs everything on hand-written gfx950 kernels and never falls
back to torch for them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..models.layout import DP, P_PAD, ModelDims, DEFAULT_DIMS, canonical_to_padded, padded_to_canonical


@dataclass
class TrainHParams:
    epochs: int
    batch_size: int = 12
    lr: float = 1e-3
    shrink_lambda: float = 0.0      # 0 for the plain AE
    fedprox_mu: float = 0.0         # 0 unless update_type == "fedprox"
    patience: int = 1
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8


@dataclass
class TrainResult:
    local_ids: List[int]
    epochs_run: np.ndarray               # int [k]
    tracking: List[List[Tuple[float, float]]]  # per client: [(train_loss, valid_loss)] per epoch
    best_epoch: np.ndarray               # int [k] (-1 if never improved)


@dataclass
class TrainHandle:
    local_ids: List[int]
    tensors: List[torch.Tensor] = field(default_factory=list)   # device results to fetch
    result: Optional[TrainResult] = None                        # filled synchronously by eager engines


def pad_features(x: np.ndarray) -> np.ndarray:
    """[n, D] -> [n, DP] float32, zero padded (aligned 512-byte rows)."""
    n, d = x.shape
    out = np.zeros((n, DP), dtype=np.float32)
    out[:, :d] = x
    return out


class ClientStore:
    """Structure-of-arrays state of the clients hosted by this rank.

    Parameters use the padded layout (``models/layout.py``).  Sized once per
    combination: ~37 KB x 5 state vectors per client plus its data
    (~2.2 MB per N-BaIoT client) — trivially resident in 288 GB of HBM.
    """

    def __init__(self, num_clients: int, device: torch.device):
        C = num_clients
        f32 = dict(dtype=torch.float32, device=device)
        self.num_clients = C
        self.device = device
        self.params = torch.zeros(C, P_PAD, **f32)
        self.adam_m = torch.zeros(C, P_PAD, **f32)
        self.adam_v = torch.zeros(C, P_PAD, **f32)
        self.adam_step = torch.zeros(C, dtype=torch.int32, device=device)
        self.anchor = torch.zeros(C, P_PAD, **f32)
        self.best = torch.zeros(C, P_PAD, **f32)
        self.train = self.valid = self.test = None
        self.train_off = self.valid_off = self.test_off = None
        self.test_label = None

    # zero rows after the last client's training rows: the helper-wave
    # kernel's batch loads read whole 12-row (batch <= 12) or 16-row (larger
    # batches) chunks without clamping rows past a client's end (those
    # columns are masked).  Contract checked by ops/_hip.TrainBuffers before
    # the first launch on a store: >= 15 rows after the last client, column
    # DP-1 of train/valid holding 1
    # (``bias_column_rows`` records which buffers _concat filled).
    TRAIN_TAIL_ROWS = 16

    @staticmethod
    def _concat(arrays: Sequence[np.ndarray], device, bias_column: bool = False, tail_rows: int = 0):
        offs = np.zeros(len(arrays) + 1, dtype=np.int64)
        for i, a in enumerate(arrays):
            offs[i + 1] = offs[i] + a.shape[0]
        parts = [pad_features(a) for a in arrays] + [np.zeros((tail_rows, DP), np.float32)]
        buf = np.concatenate(parts, 0)
        if bias_column:
            # the training kernels read X's padded column DP-1 as the constant 1
            # that feeds W1a's bias column: stored, so the helper-wave kernel
            # need not overwrite it after every batch load.  Every other reader
            # ignores the column (forward SSEs sum d < d_in, the oracle slices).
            buf[:, DP - 1] = 1.0
        return torch.from_numpy(buf).to(device), offs

    def load_data(self, train: Sequence[np.ndarray], valid: Sequence[np.ndarray],
                  test: Sequence[np.ndarray], test_label: Sequence[np.ndarray]):
        self.train, self.train_off = self._concat(train, self.device, bias_column=True,
                                                  tail_rows=self.TRAIN_TAIL_ROWS)
        self.valid, self.valid_off = self._concat(valid, self.device, bias_column=True)
        self.bias_column_rows = ("train", "valid")
        self.test, self.test_off = self._concat(test, self.device)
        lab = np.concatenate([np.asarray(l, dtype=np.int32) for l in test_label]) if test_label else np.zeros(0, np.int32)
        self.test_label = torch.from_numpy(lab).to(self.device)
        self.test_label_np = lab

    def rows(self, split: str, c: int) -> torch.Tensor:
        buf = getattr(self, split)
        off = getattr(self, split + "_off")
        return buf[int(off[c]):int(off[c + 1])]

    def labels(self, c: int) -> np.ndarray:
        return self.test_label_np[int(self.test_off[c]):int(self.test_off[c + 1])]

    def label_view(self, c: int) -> torch.Tensor:
        return self.test_label[int(self.test_off[c]):int(self.test_off[c + 1])]


def batch_mean_scores(sse: torch.Tensor, bs: int, d_in: int) -> Tuple[float, float]:
    """(mean over batches of the batch MSE, overall MSE) of a per-row SSE vector
    (`src/Trainer/client_trainer.py:226-241`)."""
    x = sse.detach().double().cpu().numpy()
    n = x.shape[0]
    if n == 0:
        return float("inf"), float("nan")
    tot, nb = 0.0, 0
    for s in range(0, n, bs):
        seg = x[s:s + bs]
        tot += float(seg.sum() / (seg.shape[0] * d_in))
        nb += 1
    return tot / nb, float(x.sum() / (n * d_in))


class Engine:
    name = "abstract"
    # operating point of the "detection" / "tpr_at_fpr" metrics (the
    # federation sets them from cfg.detect_quantile / cfg.target_fpr)
    detect_quantile = 0.95
    target_fpr = 0.01
    # what scores a ``hybrid`` model's latents: "cen" (distance to the train
    # centroid) or "knn" (distance to the knn_k-th nearest train latent); the
    # federation sets them from cfg.latent_scorer / cfg.knn_k
    latent_scorer = "cen"
    knn_k = 5

    def __init__(self, dims: ModelDims = DEFAULT_DIMS, device: Optional[torch.device] = None):
        self.dims = dims
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.store: Optional[ClientStore] = None

    # -- setup -----------------------------------------------------------------
    def setup(self, train, valid, test, test_label, init_canonical: torch.Tensor):
        C = len(train)
        self.store = ClientStore(C, self.device)
        self.store.load_data(train, valid, test, test_label)
        p = canonical_to_padded(init_canonical.to(torch.float32), self.dims).to(self.device)
        self.store.params.copy_(p)
        self.store.anchor.copy_(p)  # FedProx anchor starts at the init weights (Q11)
        self.store.best.copy_(p)

    def to_device(self, x: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(pad_features(np.asarray(x, dtype=np.float32))).to(self.device)

    def canonical(self, padded: torch.Tensor) -> torch.Tensor:
        return padded_to_canonical(padded, self.dims)

    def fetch(self, tensors: Sequence[torch.Tensor]) -> List[np.ndarray]:
        """Device -> host for several results with (at most) one synchronisation."""
        return [t.detach().cpu().numpy() for t in tensors]

    # -- primitives (implemented by subclasses) --------------------------------
    def train(self, local_ids: Sequence[int], hp: TrainHParams) -> TrainResult:
        return self.train_collect(self.train_launch(local_ids, hp))

    def train_launch(self, local_ids: Sequence[int], hp: TrainHParams) -> TrainHandle:
        raise NotImplementedError

    def train_collect(self, handle: TrainHandle, host: Optional[List[np.ndarray]] = None) -> TrainResult:
        raise NotImplementedError

    def forward_rows(self, params: torch.Tensor, items: Sequence[Tuple[int, torch.Tensor]],
                     want_sse: bool = True, want_latent: bool = False):
        """For each (param_row, data[n, DP]) item: per-row SSE over the real
        D columns and/or latents [n, Z].  Returns (sse_list, latent_list)."""
        raise NotImplementedError

    def weighted_sum(self, stack: torch.Tensor, weights: Sequence[float]) -> torch.Tensor:
        raise NotImplementedError

    def robust_aggregate(self, stack: torch.Tensor, t: int) -> torch.Tensor:
        """[k, P] -> [P]: per coordinate, the mean of the values ranked
        t .. k-t-1 (total order with ties by row; ``protocol/aggregation.py``),
        added in row order."""
        raise NotImplementedError

    def krum_aggregate(self, stack: torch.Tensor, f: int, m: int):
        """[k, P] -> ([P], kept row positions in ascending order): the mean of
        the ``m`` rows with the lowest Krum scores (sum of a row's
        ``max(k - f - 2, 0)`` smallest chunk-ordered f64 squared distances;
        ``protocol/aggregation.py``), added in row order."""
        raise NotImplementedError

    def geomed_aggregate(self, stack: torch.Tensor, iters: int, nu: float):
        """[k, P] -> ([P], the k final weights as floats in row order): the
        smoothed geometric median of the rows after ``iters`` Weiszfeld
        iterations, weights 1 / max(distance, nu) normalised in f64, rows with
        a NaN or an infinity weighted 0 (``protocol/aggregation.py``)."""
        raise NotImplementedError

    def param_drift(self, hist: torch.Tensor, new: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def cen_scores(self, train_lat: Sequence[torch.Tensor], test_lat: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        raise NotImplementedError

    def knn_scores(self, train_lat: Sequence[torch.Tensor], query_lat: Sequence[torch.Tensor],
                   k: int) -> List[torch.Tensor]:
        """float64 [n_query] per (train latents, query latents) pair: the
        distance of each query row to its ``min(k, n_train)``-th nearest train
        row (README "Latent scorers").  The scaler is CEN's fit on the train
        latents; train and query rows are both scaled as CEN scales a test row
        (``fp32((double)v - mean)``, then ``fp32((double)t0 / scale)``); the
        squared distance is summed in float64 over the columns in order from
        0, a NaN sum counts as +inf, train rows equal to each other count with
        multiplicity and a query equal to a train row is not excluded.
        ``1 <= k <= 16``; an empty train set raises ``ValueError``."""
        raise NotImplementedError

    def latent_scores(self, train_lat: Sequence[torch.Tensor], query_lat: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """The scores of the configured latent scorer (``latent_scorer``, ``knn_k``)."""
        if self.latent_scorer == "knn":
            return self.knn_scores(train_lat, query_lat, self.knn_k)
        if self.latent_scorer != "cen":
            raise ValueError(f"unknown latent_scorer {self.latent_scorer!r}")
        return self.cen_scores(train_lat, query_lat)

    def auc(self, scores: Sequence[torch.Tensor], labels: Sequence[torch.Tensor]) -> np.ndarray:
        raise NotImplementedError

    def detect_metrics(self, calib: Sequence[torch.Tensor], scores: Sequence[torch.Tensor],
                       labels: Sequence[torch.Tensor], ranks: Sequence[int],
                       calib_labels: Optional[Sequence[torch.Tensor]] = None, score_scale: float = 1.0,
                       value: str = "f1") -> np.ndarray:
        """float64 [8, k] (value, threshold, tp, fp, fn, tn, precision, recall)
        per (calibration vector, test scores, labels, rank) item: the threshold
        is the ``ranks[i]``-th smallest (0-based) cleaned calibration value
        (of the rows whose ``calib_labels`` entry is 0, when given; NaN for a
        rank of -1), row ``s`` is flagged iff ``s > threshold``.  float32
        vectors are multiplied by ``score_scale`` in float32 first; NaN reads
        as 0 and +-inf as +-DBL_MAX.  ``value``: "f1" or "recall" in row 0
        (README "Detection thresholds", eval/metrics.py)."""
        raise NotImplementedError

    def score_rows(self, detectors: Sequence, rows: Sequence, want_latents: bool = False) -> List[tuple]:
        """Score raw traffic with deployed detectors (``deploy.Detector``;
        README "Deploying a detector").  ``rows[i]``: the raw feature rows
        ``[n_i, D]`` for ``detectors[i]``, float64 or float32 (numpy, or a
        tensor).  Returns per detector ``(scores float64 [n], flags uint8 [n],
        alarms int)`` as numpy arrays: the cleaned score of every row, 1 where
        ``score > threshold``, and the number of flagged rows; with
        ``want_latents`` a fourth entry, the fp32 latents ``[n, Z]`` (None for
        an autoencoder).  The detectors' dimensions need not be the engine's."""
        raise NotImplementedError

    def explain_rows(self, detectors: Sequence, rows: Sequence, top_k: int = 5, which: Optional[Sequence] = None,
                     dense: bool = False) -> List:
        """Which features a deployed detector could not reconstruct (README
        "Explaining an alarm").  ``rows[i]``: the raw feature rows ``[n_i, D]``
        for ``detectors[i]`` as in ``score_rows``; ``which[i]``: the indices of
        the rows to explain (any order, repeats allowed; None, or ``which``
        None: every row).  Returns per detector a ``deploy.detector.Explanation``
        of numpy arrays: ``rows`` int64 [m]; ``idx`` int32 [m, top_k], the
        features by falling squared residual (NaN first, equal ones by rising
        index, -1 past ``min(top_k, D)``); ``resid`` float32 [m, top_k], their
        residuals ``y - x`` in standardised units (0 where idx is -1); ``sse``
        float32 [m] with ``forward_rows``' bits; ``resid_full`` float32 [m, D]
        with ``dense``, else None; ``latent_terms`` float64 [m, Z] for
        ``hybrid`` + ``cen`` (the score is the root of their sum from column
        0), else None.  ``top_k`` outside 1..16, an index outside ``[0, n_i)``
        or rows of the wrong shape raise ValueError."""
        raise NotImplementedError

    def monitor_rows(self, detectors: Sequence, rows: Sequence, block_rows: Optional[int] = None) -> List:
        """Is a deployed detector still looking at the traffic it was trained
        for (README "Monitoring a deployed detector")?  ``rows[i]``: the raw
        feature rows ``[n_i, D]`` for ``detectors[i]`` as in ``score_rows``;
        dimensions, types, scalers, scorers and row counts may differ within
        one call.  Returns per detector a ``deploy.detector.DriftReport``: per
        feature the counts of finite (``cnt``) and non-finite (``bad``)
        standardised values and of those outside the baseline's band
        (``out``), their float64 ``sum`` and sum of squares ``sq`` in the
        rule's fixed order, fp32 ``mn`` / ``mx``; the alarm count; the score
        histogram over the baseline's edges (None without a baseline); and the
        derived mean, variance, shares, alarm rates and PSI.  ``block_rows``
        (a multiple of 64; None: ``score_rows_per_block`` of all rows) fixes
        the summation order and is reported back."""
        raise NotImplementedError

    def incidents(self, flags: Sequence, scores: Sequence, window: int, min_alarms: int, hold: int = 0) -> List:
        """Group row-level alarms into incidents (README "Incidents").  One
        ``(flags[i], scores[i])`` pair per item: vectors of one length ``n_i``
        (numpy arrays or tensors on any device; the lengths may differ within
        a call), rows in time order; a non-zero flag counts as 1, scores are
        cleaned (NaN -> 0, +-inf -> +-DBL_MAX).  A row is hot when at least
        ``min_alarms`` of the last ``window`` rows are flagged; hot rows with
        at most ``hold`` other rows between them form one incident.  Returns
        per item a ``deploy.detector.Incidents`` of numpy arrays: ``start``,
        ``end``, ``alarms``, ``peak_row`` int64 [k], ``peak_score`` float64
        [k], and the totals ``hot_rows``, ``count``, ``rows_covered``,
        ``longest``.  An item without rows gives an empty one.  ``window``
        outside 1..4096, ``min_alarms`` outside 1..window, ``hold`` outside
        0..4096, lengths that differ and inputs that are no vectors raise
        ValueError."""
        raise NotImplementedError

    def score_incidents(self, detectors: Sequence, rows: Sequence, window: int, min_alarms: int,
                        hold: int = 0) -> List[tuple]:
        """``score_rows`` and ``incidents`` of its flags and scores in one call:
        per detector ``(scores, flags, alarms, incidents)``, the first three
        exactly what ``score_rows`` returns."""
        from ..deploy.detector import check_incident_params

        check_incident_params(window, min_alarms, hold)
        res = self.score_rows(detectors, rows)
        inc = self.incidents([r[1] for r in res], [r[0] for r in res], window, min_alarms, hold)
        return [(r[0], r[1], r[2], i) for r, i in zip(res, inc)]

    def incident_signatures(self, detectors: Sequence, rows: Sequence, flags: Sequence, incidents: Sequence,
                            top_k: int = 5, which: Optional[Sequence] = None,
                            block_rows: Optional[int] = None) -> List:
        """What each incident is about (README "Incident signatures").  Per
        detector: the raw rows ``[n_i, D]`` as in ``score_rows``, their flags
        (``[n_i]``; non-zero counts as 1), the ``deploy.detector.Incidents`` of
        those flags and ``which[i]``, the strictly rising indices of the
        incidents to summarise (None, or ``which`` None: all; at most 4096).
        Returns per detector a ``deploy.detector.Signatures``: per summarised
        incident the number of flagged rows inside it, per feature the float64
        sums ``err_sum`` of ``fp32(r * r)`` and ``resid_sum`` of the residual
        ``r = y - x`` over those rows in the rule's fixed order and the count
        ``bad`` of rows left out (a NaN or infinite square), and derived from
        them the ``top_k`` features by ``err_sum`` with their share of the
        total and their mean residual.  ``block_rows`` (a multiple of 64; None:
        ``score_rows_per_block`` of all list positions) fixes the summation
        order and is reported back.  ``top_k`` outside 1..16, a bad ``which``
        and rows or flags of the wrong shape raise ValueError."""
        raise NotImplementedError

    def standardize_ddof1(self, x: torch.Tensor) -> torch.Tensor:
        """(x - mean) / (std_ddof1 + 1e-8) over the real D columns
        (`src/Trainer/client_trainer.py:220-223`); the padded columns of the
        result are 0.  A single row has no unbiased standard deviation:
        ``torch.std`` gives NaN there, as in the reference, so every real
        column of the result is NaN (and the padding still 0) on every engine."""
        raise NotImplementedError

    # -- round operations (defaults in terms of the primitives) -----------------
    def vote_scores(self, local_rows: Sequence[int], vote_data: torch.Tensor, dev_set: Optional[torch.Tensor],
                    vote_bs: int) -> torch.Tensor:
        """float64 [k, 2]: (vote score on standardised vote data, dev-set MSE or nan)."""
        k = len(local_rows)
        out = torch.full((k, 2), float("nan"), dtype=torch.float64)
        if k == 0:
            return out
        vs = self.standardize_ddof1(vote_data)
        items = [(c, vs) for c in local_rows]
        if dev_set is not None:
            items += [(c, dev_set) for c in local_rows]
        sse, _ = self.forward_rows(self.store.params, items, want_sse=True)
        D = self.dims.d_in
        for i in range(k):
            out[i, 0] = batch_mean_scores(sse[i], vote_bs, D)[0]
            if dev_set is not None:
                out[i, 1] = batch_mean_scores(sse[k + i], 1 << 30, D)[1]
        return out

    def verify_stats(self, agg: torch.Tensor, datasets: Sequence[torch.Tensor], hist: Optional[torch.Tensor]):
        """(MSE of ``agg`` on each dataset [float64], drift of each hist row vs agg)."""
        aggp = agg.unsqueeze(0)
        sse, _ = self.forward_rows(aggp, [(0, x) for x in datasets], want_sse=True) if datasets else ([], None)
        D = self.dims.d_in
        mse = torch.tensor([batch_mean_scores(s, 1 << 30, D)[1] for s in sse], dtype=torch.float64)
        drift = self.param_drift(hist, agg) if hist is not None and hist.shape[0] else torch.zeros(0)
        return mse, drift

    def model_mse(self, local_rows: Sequence[int], datasets: Sequence[torch.Tensor]) -> np.ndarray:
        """float64 [k]: MSE of each local row's own current model on its dataset
        (thesis verification's old loss)."""
        if not len(local_rows):
            return np.zeros(0)
        sse, _ = self.forward_rows(self.store.params, list(zip(local_rows, datasets)), want_sse=True)
        D = self.dims.d_in
        return np.array([batch_mean_scores(s, 1 << 30, D)[1] for s in sse], dtype=np.float64)

    def adopt(self, local_rows: Sequence[int], agg: torch.Tensor, anchor: bool = True) -> None:
        st = self.store
        if not len(local_rows):
            return
        idx = torch.tensor(list(local_rows), dtype=torch.long, device=st.params.device)
        rows = agg.unsqueeze(0).expand(len(local_rows), -1)
        st.params.index_copy_(0, idx, rows)
        if anchor:
            st.anchor.index_copy_(0, idx, rows)

    def evaluate(self, model_type: str, metric: str = "AUC", keep_latents: bool = False):
        from ..eval.evaluator import evaluate_clients

        return evaluate_clients(self, list(range(self.store.num_clients)), model_type, metric, keep_latents)

    def synchronize(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
