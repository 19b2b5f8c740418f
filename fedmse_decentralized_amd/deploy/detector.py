"""A trained client as a deployable detector (README "Deploying a detector").

A ``Detector`` bundles everything needed to turn *raw* traffic rows into
anomaly scores and alarms: the model's dimensions, type and canonical
parameter vector, the per-client feature scaler that ``data.prepare`` fits on
the client's train split, for ``hybrid`` models the latent scorer with its
state (the latent ``StandardScaler`` for ``cen``; ``knn_k`` and the train
latents for ``knn``), and the calibrated alarm threshold.  ``save`` / ``load``
use a plain ``.npz`` of arrays and scalars (no pickle; loads with
``allow_pickle=False``).

``score_rows_numpy`` is the scoring rule written out literally (the oracle of
``score_rows_kernel``):

1. standardise: ``IoTDataProcessor.transform(rows).astype(float32)``;
2. forward: the engine's ``forward_rows`` on the zero-padded fp32 rows;
3. score: ``autoencoder`` ``(double)(sse * fp32(1 / D))`` with the product in
   fp32; ``hybrid`` + ``cen`` the CEN per-row loop under the stored latent
   scaler; ``hybrid`` + ``knn`` ``Engine.knn_scores`` against the stored
   train latents;
4. clean (NaN -> 0, +-inf -> +-DBL_MAX) and flag iff ``score > threshold``
   (a tie is normal; a NaN threshold flags nothing).
"""
from __future__ import annotations

import json
import zipfile
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..data.scaler import IoTDataProcessor, StandardScaler
from ..eval.metrics import calibration_rank
from ..models.layout import ModelDims, canonical_to_padded

FORMAT_VERSION = 1
MODEL_TYPES = ("autoencoder", "hybrid")
SCALER_KINDS = ("standard", "minmax")
LATENT_SCORERS = ("cen", "knn")
# the scaler vectors each kind stores, in the order the kernel reads them
SCALER_FIELDS = {"standard": ("mean_", "scale_"), "minmax": ("scale_", "min_")}
KNN_MAX_K = 16
MONITOR_MAX_EDGES = 15   # score edges a baseline holds at most (monitor_bins - 1)
BASELINE_FIELDS = ("feat_lo", "feat_hi", "score_edges", "score_base")


@dataclass
class Baseline:
    """What "normal" looked like when the detector was exported (README
    "Monitoring a deployed detector")."""
    feat_lo: np.ndarray       # float32 [D]: smallest finite standardised train value per feature (+inf: none)
    feat_hi: np.ndarray       # float32 [D]: largest (-inf: none)
    score_edges: np.ndarray   # float64 [B], 0 <= B <= 15, non-decreasing: order statistics of the calibration scores
    score_base: np.ndarray    # int64 [B + 1]: the calibration scores' own bin counts

    def validate(self, d_in: int) -> None:
        self.feat_lo = _arr(self.feat_lo, np.float32, (d_in,), "baseline feat_lo")
        self.feat_hi = _arr(self.feat_hi, np.float32, (d_in,), "baseline feat_hi")
        e = np.asarray(self.score_edges)
        if e.ndim != 1 or e.shape[0] > MONITOR_MAX_EDGES:
            raise ValueError(f"baseline score_edges must be a vector of at most {MONITOR_MAX_EDGES} values, "
                             f"got shape {e.shape}")
        self.score_edges = _arr(e, np.float64, e.shape, "baseline score_edges")
        if np.isnan(self.score_edges).any() or np.any(np.diff(self.score_edges) < 0):
            raise ValueError("baseline score_edges must be non-decreasing numbers")
        b = np.asarray(self.score_base)
        if b.dtype.kind not in "iu" or b.shape != (e.shape[0] + 1,):
            raise ValueError(f"baseline score_base must be {e.shape[0] + 1} integers, got {b.dtype} {b.shape}")
        self.score_base = np.ascontiguousarray(b, dtype=np.int64)
        if np.any(self.score_base < 0):
            raise ValueError("baseline score_base holds counts: none may be negative")


def score_bins(scores: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """int64 [B + 1] bin counts of cleaned scores: ``bin(s) = #{i : edge_i <
    s}`` (a score equal to an edge falls in the lower bin)."""
    b = np.searchsorted(np.asarray(edges, dtype=np.float64), np.asarray(scores, dtype=np.float64), side="left")
    return np.bincount(b, minlength=len(edges) + 1).astype(np.int64)


def make_baseline(train_std: np.ndarray, calib_sorted: np.ndarray, bins: int) -> Baseline:
    """The baseline of fp32 standardised train rows ``[n, D]`` and the sorted
    cleaned calibration scores, with ``bins`` score bins (2..16)."""
    if isinstance(bins, bool) or not 2 <= int(bins) <= MONITOR_MAX_EDGES + 1:
        raise ValueError(f"monitor_bins must be an integer in 2..{MONITOR_MAX_EDGES + 1}, got {bins!r}")
    x = np.asarray(train_std, dtype=np.float32)
    fin = np.isfinite(x)
    lo = np.where(fin, x, np.float32(np.inf)).min(axis=0, initial=np.float32(np.inf)).astype(np.float32)
    hi = np.where(fin, x, np.float32(-np.inf)).max(axis=0, initial=np.float32(-np.inf)).astype(np.float32)
    c = np.asarray(calib_sorted, dtype=np.float64)
    n_c = c.shape[0]
    edges = np.array([c[calibration_rank(n_c, (i + 1) / bins)] for i in range(int(bins) - 1)] if n_c else [],
                     dtype=np.float64)
    return Baseline(feat_lo=lo, feat_hi=hi, score_edges=edges, score_base=score_bins(c, edges))


@dataclass
class Detector:
    dims: ModelDims
    model_type: str                       # "autoencoder" | "hybrid"
    params: np.ndarray                    # float32 [dims.num_params], canonical order
    scaler_kind: str                      # "standard" | "minmax"
    scaler: Dict[str, np.ndarray]         # SCALER_FIELDS[scaler_kind] -> float64 [D]
    threshold: float = float("nan")       # alarm iff score > threshold; NaN: no alarms
    detect_quantile: float = float("nan")  # the quantile the threshold was calibrated at
    latent_scorer: Optional[str] = None   # hybrid: "cen" | "knn"
    latent_mean: Optional[np.ndarray] = None    # hybrid: float64 [Z], StandardScaler of the train latents
    latent_scale: Optional[np.ndarray] = None   # hybrid: float64 [Z]
    knn_k: int = 0                        # knn: which nearest train latent's distance is the score
    train_latents: Optional[np.ndarray] = None  # knn: float32 [n, Z]
    provenance: Dict[str, str] = field(default_factory=dict)
    version: int = FORMAT_VERSION
    baseline: Optional[Baseline] = None   # what monitor_rows compares live traffic with

    def __post_init__(self):
        self.validate()

    # -- consistency ---------------------------------------------------------------
    def validate(self) -> None:
        """ValueError unless every field has the type and shape the others imply."""
        d = self.dims
        if self.version != FORMAT_VERSION:
            raise ValueError(f"detector format version {self.version!r} is not supported (this reader: "
                             f"{FORMAT_VERSION})")
        if self.model_type not in MODEL_TYPES:
            raise ValueError(f"model_type must be one of {' | '.join(MODEL_TYPES)}, got {self.model_type!r}")
        if self.scaler_kind not in SCALER_KINDS:
            raise ValueError(f"scaler kind must be one of {' | '.join(SCALER_KINDS)}, got {self.scaler_kind!r}")
        self.params = _arr(self.params, np.float32, (d.num_params,), "params")
        want = SCALER_FIELDS[self.scaler_kind]
        if set(self.scaler) != set(want):
            raise ValueError(f"a {self.scaler_kind} scaler holds {want}, got {sorted(self.scaler)}")
        self.scaler = {k: _arr(self.scaler[k], np.float64, (d.d_in,), f"scaler {k}") for k in want}
        self.threshold = float(self.threshold)
        self.detect_quantile = float(self.detect_quantile)
        self.provenance = {str(k): str(v) for k, v in dict(self.provenance).items()}
        if self.baseline is not None:
            if not isinstance(self.baseline, Baseline):
                raise ValueError(f"baseline must be a Baseline, got {type(self.baseline).__name__}")
            self.baseline.validate(d.d_in)
        if self.model_type == "autoencoder":
            if self.latent_scorer is not None or self.latent_mean is not None or self.latent_scale is not None \
                    or self.train_latents is not None or self.knn_k:
                raise ValueError("an autoencoder detector scores by reconstruction error: no latent scorer state")
            return
        if self.latent_scorer not in LATENT_SCORERS:
            raise ValueError(f"latent_scorer must be one of {' | '.join(LATENT_SCORERS)}, got {self.latent_scorer!r}")
        if self.latent_mean is None or self.latent_scale is None:
            raise ValueError("a hybrid detector holds the latent scaler's mean_ and scale_")
        self.latent_mean = _arr(self.latent_mean, np.float64, (d.latent,), "latent mean_")
        self.latent_scale = _arr(self.latent_scale, np.float64, (d.latent,), "latent scale_")
        if self.latent_scorer == "knn":
            if isinstance(self.knn_k, bool) or not 1 <= int(self.knn_k) <= KNN_MAX_K:
                raise ValueError(f"knn_k must lie in 1..{KNN_MAX_K}, got {self.knn_k!r}")
            self.knn_k = int(self.knn_k)
            if self.train_latents is None:
                raise ValueError("a knn detector holds its train latents")
            tl = np.asarray(self.train_latents)
            if tl.ndim != 2 or tl.shape[0] < 1:
                raise ValueError("a knn detector needs at least one train latent row")
            self.train_latents = _arr(tl, np.float32, (tl.shape[0], d.latent), "train latents")
        elif self.train_latents is not None or self.knn_k:
            raise ValueError("a cen detector holds no knn state")

    # -- file ----------------------------------------------------------------------
    def save(self, path: str) -> str:
        """Write the bundle as ``.npz`` (numeric and string arrays only)."""
        arrays = {
            "version": np.array(self.version, dtype=np.int64),
            "dims": np.array([self.dims.d_in, self.dims.hidden, self.dims.latent], dtype=np.int64),
            "model_type": np.array(self.model_type),
            "params": self.params,
            "scaler_kind": np.array(self.scaler_kind),
            "threshold": np.array(self.threshold, dtype=np.float64),
            "detect_quantile": np.array(self.detect_quantile, dtype=np.float64),
            "provenance": np.array(json.dumps(self.provenance, sort_keys=True)),
        }
        for k, v in self.scaler.items():
            arrays["scaler_" + k] = v
        if self.model_type == "hybrid":
            arrays["latent_scorer"] = np.array(self.latent_scorer)
            arrays["latent_mean_"] = self.latent_mean
            arrays["latent_scale_"] = self.latent_scale
            if self.latent_scorer == "knn":
                arrays["knn_k"] = np.array(self.knn_k, dtype=np.int64)
                arrays["train_latents"] = self.train_latents
        if self.baseline is not None:
            for k in BASELINE_FIELDS:
                arrays["baseline_" + k] = getattr(self.baseline, k)
        with open(path, "wb") as f:   # (a file object: numpy appends no suffix)
            np.savez(f, **arrays)
        return path

    @classmethod
    def load(cls, path: str) -> "Detector":
        """Read a bundle; ValueError for an unknown version, a file that needs
        pickle, a missing array or shapes that contradict each other."""
        try:
            with np.load(path, allow_pickle=False) as z:
                a = {k: z[k] for k in z.files}
        except (zipfile.BadZipFile, OSError, EOFError) as e:
            if isinstance(e, FileNotFoundError):
                raise
            raise ValueError(f"{path}: not a detector bundle ({e})") from e
        except ValueError as e:   # numpy: "Object arrays cannot be loaded when allow_pickle=False"
            raise ValueError(f"{path}: not a detector bundle ({e})") from e

        def need(k):
            if k not in a:
                raise ValueError(f"{path}: detector bundle lacks {k!r}")
            return a[k]

        version = _scalar(need("version"), int, "version")
        if version != FORMAT_VERSION:
            raise ValueError(f"{path}: detector format version {version} is not supported (this reader: "
                             f"{FORMAT_VERSION})")
        dv = np.asarray(need("dims"))
        if dv.shape != (3,) or dv.dtype.kind not in "iu":
            raise ValueError(f"{path}: dims must be three integers")
        dims = ModelDims(*(int(v) for v in dv))
        model_type = _scalar(need("model_type"), str, "model_type")
        kind = _scalar(need("scaler_kind"), str, "scaler_kind")
        if kind not in SCALER_KINDS:
            raise ValueError(f"{path}: unknown scaler kind {kind!r}")
        try:
            prov = json.loads(_scalar(need("provenance"), str, "provenance"))
        except json.JSONDecodeError as e:
            raise ValueError(f"{path}: provenance is not a JSON object ({e})") from e
        if not isinstance(prov, dict):
            raise ValueError(f"{path}: provenance is not a JSON object")
        kw = {}
        if model_type == "hybrid":
            kw["latent_scorer"] = _scalar(need("latent_scorer"), str, "latent_scorer")
            kw["latent_mean"], kw["latent_scale"] = need("latent_mean_"), need("latent_scale_")
            if kw["latent_scorer"] == "knn":
                kw["knn_k"] = _scalar(need("knn_k"), int, "knn_k")
                kw["train_latents"] = need("train_latents")
        have = [k for k in BASELINE_FIELDS if "baseline_" + k in a]
        if have and len(have) != len(BASELINE_FIELDS):
            raise ValueError(f"{path}: a baseline holds {BASELINE_FIELDS}, the bundle only {tuple(have)}")
        if have:
            kw["baseline"] = Baseline(feat_lo=_exact(a["baseline_feat_lo"], np.float32, "baseline feat_lo"),
                                      feat_hi=_exact(a["baseline_feat_hi"], np.float32, "baseline feat_hi"),
                                      score_edges=_exact(a["baseline_score_edges"], np.float64,
                                                         "baseline score_edges"),
                                      score_base=_exact(a["baseline_score_base"], np.int64, "baseline score_base"))
        return cls(dims=dims, model_type=model_type, params=_exact(need("params"), np.float32, "params"),
                   scaler_kind=kind,
                   scaler={k: _exact(need("scaler_" + k), np.float64, "scaler " + k) for k in SCALER_FIELDS[kind]},
                   threshold=_scalar(need("threshold"), float, "threshold"),
                   detect_quantile=_scalar(need("detect_quantile"), float, "detect_quantile"),
                   provenance=prov, version=version, **kw)

    # -- scoring pieces --------------------------------------------------------------
    def processor(self) -> IoTDataProcessor:
        """The fitted ``IoTDataProcessor`` this bundle's scaler came from."""
        proc = IoTDataProcessor(self.scaler_kind)
        for k, v in self.scaler.items():
            setattr(proc.scaler, k, v)
        return proc

    def standardise(self, rows: np.ndarray) -> np.ndarray:
        """Raw rows [n, D] (float64, or float32 widened exactly) -> the fp32
        rows the model was trained on."""
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != self.dims.d_in:
            raise ValueError(f"rows must be [n, {self.dims.d_in}], got {rows.shape}")
        with np.errstate(all="ignore"):
            return self.processor().transform(rows.astype(np.float64))[0].astype(np.float32)

    def padded_params(self) -> torch.Tensor:
        return canonical_to_padded(torch.from_numpy(self.params), self.dims)

    # -- export ------------------------------------------------------------------------
    @classmethod
    def from_federation(cls, fed, client_id: int, baseline: bool = False) -> "Detector":
        """Client ``client_id``'s detector under its current parameters (the
        ones the evaluation evaluates); the client must be hosted by this
        rank.  The threshold is README "Detection thresholds"' tau: the
        ``calibration_rank(n_valid, detect_quantile)``-th smallest cleaned
        validation score under these parameters (NaN without validation rows).
        ``baseline``: also record the monitoring baseline (README "Monitoring
        a deployed detector") from the same train rows and validation scores;
        no further launch."""
        eng, cfg = fed.engine, fed.cfg
        st, dims = eng.store, fed.dims
        if client_id not in fed.local:
            raise ValueError(f"client {client_id} is not hosted by this rank")
        loc = fed._loc(client_id)
        client = fed.clients[client_id]
        sc = client.meta.get("scaler")
        if sc is None:
            raise ValueError(f"client {client.name}: the prepared data carries no fitted scaler")
        params = eng.canonical(st.params[loc]).detach().cpu().numpy().astype(np.float32)
        valid = st.rows("valid", loc)
        kw = {}
        if fed.model_type == "hybrid":
            _, lat = eng.forward_rows(st.params, [(loc, st.rows("train", loc)), (loc, valid)],
                                      want_sse=False, want_latent=True)
            train_lat = eng.fetch([lat[0]])[0].astype(np.float32)
            zs = StandardScaler().fit(train_lat)
            kw = dict(latent_scorer=eng.latent_scorer, latent_mean=zs.mean_, latent_scale=zs.scale_)
            if eng.latent_scorer == "knn":
                kw.update(knn_k=int(eng.knn_k), train_latents=train_lat)
            calib = eng.fetch([eng.latent_scores([lat[0]], [lat[1]])[0]])[0].astype(np.float64)
        else:
            sse, _ = eng.forward_rows(st.params, [(loc, valid)], want_sse=True, want_latent=False)
            calib = _ae_scores(eng.fetch([sse[0]])[0], dims.d_in)
        calib = np.sort(np.nan_to_num(calib))
        j = calibration_rank(calib.shape[0], cfg.detect_quantile)
        tau = float(calib[j]) if j >= 0 else float("nan")
        if tau == 0.0:
            tau = 0.0   # a selected -0.0 is reported as +0.0
        prov = {"client": client.name, "client_id": str(client_id), "model_type": fed.model_type,
                "update_type": fed.update_type, "rounds": str(fed.round_idx), "run": str(fed.run),
                "experiment": cfg.experiment_name}
        if baseline:
            train_std = eng.fetch([st.rows("train", loc)])[0][:, :dims.d_in]
            kw["baseline"] = make_baseline(train_std, calib, cfg.monitor_bins)
        return cls(dims=dims, model_type=fed.model_type, params=params, scaler_kind=sc["kind"],
                   scaler={k: np.asarray(sc[k], dtype=np.float64) for k in SCALER_FIELDS[sc["kind"]]},
                   threshold=tau, detect_quantile=float(cfg.detect_quantile), provenance=prov, **kw)


def _arr(a, dtype, shape: Tuple[int, ...], what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype.kind not in "fiu" or a.shape != shape:
        raise ValueError(f"{what} must be a numeric array of shape {shape}, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=dtype)


def _exact(a, dtype, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.dtype(dtype):
        raise ValueError(f"{what} must be stored as {np.dtype(dtype).name}, got {a.dtype}")
    return a


def _scalar(a, typ, what: str):
    a = np.asarray(a)
    kinds = {int: "iu", float: "f", str: "U"}[typ]
    if a.shape != () or a.dtype.kind not in kinds:
        raise ValueError(f"{what} must be one {typ.__name__}, got {a.dtype} {a.shape}")
    return typ(a[()])


def _ae_scores(sse: np.ndarray, d_in: int) -> np.ndarray:
    """(double)(sse * fp32(1 / D)), the product in fp32: how auc_kernel and
    detect_kernel read an autoencoder score."""
    with np.errstate(all="ignore"):
        return (np.asarray(sse, dtype=np.float32) * np.float32(1.0 / d_in)).astype(np.float64)


def cen_terms_stored(lat: np.ndarray, mean: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """The squares cen_score_kernel's per-row loop adds up, float64 [n, Z]:
    per column ``t0 = fp32((double)z - mean)``, ``t1 = fp32((double)t0 /
    scale)``, ``(double)t1 * (double)t1``."""
    with np.errstate(all="ignore"):
        t = np.asarray(lat, dtype=np.float32).copy()
        t -= mean          # numpy in-place: computed in float64, stored as float32
        t /= scale
        t64 = t.astype(np.float64)
        return t64 * t64


def cen_scores_stored(lat: np.ndarray, mean: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """cen_score_kernel's per-row loop under a stored scaler: the terms of
    ``cen_terms_stored`` accumulated in float64 in column order from 0, then
    the root."""
    with np.errstate(all="ignore"):
        terms = cen_terms_stored(lat, mean, scale)
        acc = np.zeros(terms.shape[0], dtype=np.float64)
        for j in range(terms.shape[1]):
            acc += terms[:, j]
        return np.sqrt(acc)


def clean_and_flag(scores: np.ndarray, threshold: float):
    """(cleaned float64 scores, uint8 flags, alarm count)."""
    s = np.nan_to_num(np.asarray(scores, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        flags = (s > threshold).astype(np.uint8)
    return s, flags, int(flags.sum())


def score_rows_numpy(detector: Detector, rows: np.ndarray, engine=None, want_latents: bool = False):
    """The scoring rule, step by step, on the host: ``(scores float64 [n],
    flags uint8 [n], alarms)`` (plus the fp32 latents with ``want_latents``;
    None for an autoencoder).  ``engine``: whose ``forward_rows`` (and, for
    knn, ``knn_scores``) run steps 2 and 3; default a ``TorchEngine`` on the CPU."""
    from ..engine.base import pad_features

    det = detector
    if engine is None:
        from ..engine.torch_engine import TorchEngine

        engine = TorchEngine(det.dims, torch.device("cpu"))
    if engine.dims != det.dims:
        raise ValueError(f"the engine's dimensions {engine.dims} are not the detector's {det.dims}")
    x = det.standardise(rows)
    n = x.shape[0]
    hybrid = det.model_type == "hybrid"
    if n == 0:
        lat0 = np.zeros((0, det.dims.latent), np.float32) if hybrid else None
        out = (np.zeros(0, np.float64), np.zeros(0, np.uint8), 0)
        return out + (lat0,) if want_latents else out
    params = det.padded_params().unsqueeze(0).to(engine.device)
    xt = torch.from_numpy(pad_features(x)).to(engine.device)
    sse, lat = engine.forward_rows(params, [(0, xt)], want_sse=not hybrid, want_latent=hybrid)
    lat_np = None
    if not hybrid:
        scores = _ae_scores(engine.fetch([sse[0]])[0], det.dims.d_in)
    else:
        lat_np = engine.fetch([lat[0]])[0].astype(np.float32)
        if det.latent_scorer == "cen":
            scores = cen_scores_stored(lat_np, det.latent_mean, det.latent_scale)
        else:
            tr = torch.from_numpy(det.train_latents).to(engine.device)
            scores = engine.fetch([engine.knn_scores([tr], [lat[0]], det.knn_k)[0]])[0].astype(np.float64)
    out = clean_and_flag(scores, det.threshold)
    return out + (lat_np,) if want_latents else out


# ---------------------------------------------------------------------------
# explaining an alarm (README "Explaining an alarm")
EXPLAIN_MAX_K = 16


@dataclass
class Explanation:
    """What ``Engine.explain_rows`` returns per detector, as numpy arrays."""
    rows: np.ndarray                        # int64 [m]: the explained indices into the raw rows
    idx: np.ndarray                         # int32 [m, K]: features by falling squared residual; -1 unused
    resid: np.ndarray                       # float32 [m, K]: y - x in standardised units; 0 unused
    sse: np.ndarray                         # float32 [m]: forward_rows' per-row sum of squared residuals
    resid_full: Optional[np.ndarray] = None     # float32 [m, D] (dense mode)
    latent_terms: Optional[np.ndarray] = None   # float64 [m, Z] (hybrid + cen): score = sqrt(sum over j from 0)


def check_top_k(top_k) -> int:
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= int(top_k) <= EXPLAIN_MAX_K:
        raise ValueError(f"explain_rows: top_k must be an integer in 1..{EXPLAIN_MAX_K}, got {top_k!r}")
    return int(top_k)


def check_which(which, n: int) -> np.ndarray:
    """The explained row indices as int64 [m]: ``which`` (any order, repeats
    allowed, every entry in ``[0, n)``) or, for None, ``0..n-1``."""
    if which is None:
        return np.arange(n, dtype=np.int64)
    if torch.is_tensor(which):
        which = which.detach().cpu().numpy()
    w = np.asarray(which)
    if w.ndim != 1 or (w.size and w.dtype.kind not in "iu"):
        raise ValueError(f"explain_rows: which must be a vector of row indices, got {w.dtype} {w.shape}")
    w = w.astype(np.int64)
    if w.size and (int(w.min()) < 0 or int(w.max()) >= n):
        raise ValueError(f"explain_rows: which must lie in [0, {n})")
    return w


def select_top_k(resid: np.ndarray, top_k: int):
    """The selection rule on fp32 residual rows [m, D] -> ``(idx int32 [m, K],
    resid float32 [m, K])``: key ``fp32(r * r)`` with NaN ranked as +inf,
    descending, equal keys by ascending feature; slots past ``min(K, D)``
    hold -1 and 0."""
    k = check_top_k(top_k)
    r = np.asarray(resid, dtype=np.float32)
    if r.ndim != 2:
        raise ValueError(f"residual rows must be [m, D], got {r.shape}")
    m, D = r.shape
    idx = np.full((m, k), -1, dtype=np.int32)
    out = np.zeros((m, k), dtype=np.float32)
    kk = min(k, D)
    with np.errstate(all="ignore"):
        e = r * r
    key = np.where(np.isnan(e), np.float32(np.inf), e)
    for i in range(m):
        order = np.argsort(-key[i], kind="stable")[:kk]
        idx[i, :kk] = order
        out[i, :kk] = r[i, order]
    return idx, out


def explain_rows_numpy(detector: Detector, rows: np.ndarray, top_k: int, which=None, dense: bool = False,
                       engine=None) -> Explanation:
    """The explanation rule, step by step, on the host (the oracle of
    ``TorchEngine.explain_rows``): standardise the chosen raw rows, run the
    fp32 ``functional_forward``, ``resid = y - x``, take ``sse`` (and, for
    ``hybrid`` + ``cen``, the latents) from the engine's ``forward_rows`` on
    the same rows, rank by ``select_top_k``.  ``engine``: default a
    ``TorchEngine`` on the CPU."""
    from ..engine.base import pad_features
    from ..models.reference import functional_forward, unflatten

    det = detector
    k = check_top_k(top_k)
    if engine is None:
        from ..engine.torch_engine import TorchEngine

        engine = TorchEngine(det.dims, torch.device("cpu"))
    if engine.dims != det.dims:
        raise ValueError(f"the engine's dimensions {engine.dims} are not the detector's {det.dims}")
    rows = np.asarray(rows)
    D, Z = det.dims.d_in, det.dims.latent
    if rows.ndim != 2 or rows.shape[1] != D:
        raise ValueError(f"rows must be [n, {D}], got {rows.shape}")
    w = check_which(which, rows.shape[0])
    m = w.shape[0]
    cen = det.model_type == "hybrid" and det.latent_scorer == "cen"
    if m == 0:
        return Explanation(rows=w, idx=np.zeros((0, k), np.int32), resid=np.zeros((0, k), np.float32),
                           sse=np.zeros(0, np.float32), resid_full=np.zeros((0, D), np.float32) if dense else None,
                           latent_terms=np.zeros((0, Z), np.float64) if cen else None)
    x = det.standardise(rows[w])
    xp = torch.from_numpy(pad_features(x))
    with torch.no_grad():
        xt = xp[:, :D]
        _, y = functional_forward(unflatten(torch.from_numpy(det.params), det.dims), xt)
        resid = (y - xt).numpy().astype(np.float32)
    params = det.padded_params().unsqueeze(0).to(engine.device)
    sse, lat = engine.forward_rows(params, [(0, xp.to(engine.device))], want_sse=True, want_latent=cen)
    sse = engine.fetch([sse[0]])[0].astype(np.float32)
    terms = None
    if cen:
        terms = cen_terms_stored(engine.fetch([lat[0]])[0].astype(np.float32), det.latent_mean, det.latent_scale)
    idx, top = select_top_k(resid, k)
    return Explanation(rows=w, idx=idx, resid=top, sse=sse, resid_full=resid if dense else None, latent_terms=terms)


def expected_raw(detector: Detector, x_std: np.ndarray, resid: np.ndarray, idx: Optional[np.ndarray] = None):
    """What the model expected, in raw units (float64): the reconstruction
    ``y = (double)x_std + (double)resid`` put through the inverse of the
    feature scaler (``standard``: ``y * scale_ + mean_``; ``minmax``: ``(y -
    min_) / scale_``).  ``x_std`` and ``resid`` are whole rows ``[m, D]``, or,
    with ``idx`` (``[m, K]`` feature indices; -1: NaN), their entries at those
    features."""
    det = detector
    y = np.asarray(x_std).astype(np.float64) + np.asarray(resid).astype(np.float64)
    sc = det.scaler
    a, b = (sc["scale_"], sc["mean_"]) if det.scaler_kind == "standard" else (sc["scale_"], sc["min_"])
    if idx is None:
        if y.ndim != 2 or y.shape[1] != det.dims.d_in:
            raise ValueError(f"x_std and resid must be [m, {det.dims.d_in}], got {y.shape}")
        sa, sb = a, b
    else:
        idx = np.asarray(idx)
        if idx.shape != y.shape:
            raise ValueError(f"idx {idx.shape} must match x_std and resid {y.shape}")
        safe = np.where(idx >= 0, idx, 0)
        sa, sb = a[safe], b[safe]
    with np.errstate(all="ignore"):
        out = y * sa + sb if det.scaler_kind == "standard" else (y - sb) / sa
    if idx is not None:
        out = np.where(idx >= 0, out, np.nan)
    return out


# ---------------------------------------------------------------------------
# monitoring a deployed detector (README "Monitoring a deployed detector")
MONITOR_CHUNK_ROWS = 64   # block_rows is a multiple of it: four waves, one 16-row tile each
MONITOR_TILE = 16
MONITOR_WAVES = 4


@dataclass
class DriftReport:
    """What ``Engine.monitor_rows`` returns per detector (numpy).  The first
    block is what the rule fixes to the bit; the second is derived from it on
    the host in float64 (``drift_report``)."""
    n: int
    block_rows: int
    cnt: np.ndarray                     # int64 [D]: finite standardised values
    bad: np.ndarray                     # int64 [D]: NaN / +-inf ones
    out: np.ndarray                     # int64 [D]: finite ones outside the baseline's band
    sum: np.ndarray                     # float64 [D]
    sq: np.ndarray                      # float64 [D]
    mn: np.ndarray                      # float32 [D]
    mx: np.ndarray                      # float32 [D]
    alarms: int
    hist: Optional[np.ndarray]          # int64 [B + 1], None without a baseline
    mean: np.ndarray                    # sum / cnt
    var: np.ndarray                     # max(sq / cnt - mean^2, 0)
    out_share: np.ndarray               # out / max(cnt, 1)
    bad_share: np.ndarray               # bad / max(n, 1)
    alarm_rate: float                   # alarms / max(n, 1)
    expected_alarm_rate: float          # 1 - detect_quantile
    psi: float                          # population stability index of hist against score_base; NaN without


def check_block_rows(block_rows) -> int:
    if isinstance(block_rows, bool) or not isinstance(block_rows, (int, np.integer)) or int(block_rows) < 1 \
            or int(block_rows) % MONITOR_CHUNK_ROWS:
        raise ValueError(f"monitor_rows: block_rows must be a positive multiple of {MONITOR_CHUNK_ROWS}, "
                         f"got {block_rows!r}")
    return int(block_rows)


def drift_report(detector: Detector, n: int, block_rows: int, cnt, bad, out, sum_, sq, mn, mx, alarms,
                 hist) -> DriftReport:
    """The report of the rule's results, with the derived float64 values."""
    cnt, bad, out = (np.ascontiguousarray(v, dtype=np.int64) for v in (cnt, bad, out))
    sum_, sq = np.ascontiguousarray(sum_, dtype=np.float64), np.ascontiguousarray(sq, dtype=np.float64)
    mn, mx = np.ascontiguousarray(mn, dtype=np.float32), np.ascontiguousarray(mx, dtype=np.float32)
    hist = None if hist is None else np.ascontiguousarray(hist, dtype=np.int64)
    with np.errstate(all="ignore"):
        c = cnt.astype(np.float64)
        mean = sum_ / c
        var = np.maximum(sq / c - mean * mean, 0.0)
        out_share = out / np.maximum(c, 1.0)
        bad_share = bad / float(max(n, 1))
    psi = float("nan")
    base = detector.baseline
    if base is not None and hist is not None and base.score_edges.shape[0] > 0:
        k = hist.shape[0]
        p = (hist + 0.5) / (float(n) + 0.5 * k)
        q = (base.score_base + 0.5) / (float(base.score_base.sum()) + 0.5 * k)
        psi = float(np.sum((p - q) * np.log(p / q)))
    return DriftReport(n=int(n), block_rows=int(block_rows), cnt=cnt, bad=bad, out=out, sum=sum_, sq=sq, mn=mn, mx=mx,
                       alarms=int(alarms), hist=hist, mean=mean, var=var, out_share=out_share, bad_share=bad_share,
                       alarm_rate=int(alarms) / max(int(n), 1), expected_alarm_rate=1.0 - detector.detect_quantile,
                       psi=psi)


def monitor_feature_stats(x_std: np.ndarray, block_rows: int, lo: Optional[np.ndarray], hi: Optional[np.ndarray]):
    """The per-feature part of the monitoring rule on fp32 standardised rows
    ``[n, D]``: ``(cnt, bad, out, sum, sq, mn, mx)``.  Every stream (block b,
    wave w: the block's 16-row tiles w, w + 4, ... in rising order) is
    accumulated row by row (all streams side by side, one row of each per
    step), then the streams fold in wave order, the blocks in block order."""
    R = check_block_rows(block_rows)
    x = np.asarray(x_std, dtype=np.float32)
    n, D = x.shape
    lo = np.full(D, -np.inf, np.float32) if lo is None else np.asarray(lo, dtype=np.float32)
    hi = np.full(D, np.inf, np.float32) if hi is None else np.asarray(hi, dtype=np.float32)
    nb = -(-n // R)
    W = MONITOR_WAVES
    shape = (nb, W, D)
    cnt, bad, out = (np.zeros(shape, np.int64) for _ in range(3))
    s, q = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    mn, mx = np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    b0 = (np.arange(nb, dtype=np.int64) * R)[:, None]
    end = np.minimum(n, b0 + R)
    w = np.arange(W, dtype=np.int64)[None, :]
    with np.errstate(all="ignore"):
        for p in range(R // W if nb else 0):   # position in the stream
            row = b0 + (W * (p // MONITOR_TILE) + w) * MONITOR_TILE + p % MONITOR_TILE   # [nb, W]
            live = row < end
            if not live.any():
                break
            t = x[np.where(live, row, 0)]                       # [nb, W, D]
            fin = np.isfinite(t) & live[:, :, None]
            t64 = t.astype(np.float64)
            bad += live[:, :, None] & ~fin
            cnt += fin
            s = np.where(fin, s + t64, s)
            q = np.where(fin, q + t64 * t64, q)
            mn = np.where(fin & (t < mn), t, mn)
            mx = np.where(fin & (t > mx), t, mx)
            out += fin & ((t < lo) | (t > hi))
        # streams -> block: ((p0 + p1) + p2) + p3
        S, Q, MN, MX = s[:, 0], q[:, 0], mn[:, 0], mx[:, 0]
        for k in range(1, W):
            S, Q = S + s[:, k], Q + q[:, k]
            MN = np.where(mn[:, k] < MN, mn[:, k], MN)
            MX = np.where(mx[:, k] > MX, mx[:, k], MX)
        # blocks -> total, in block order from +0.0
        T, TQ = np.zeros(D, np.float64), np.zeros(D, np.float64)
        tmn, tmx = np.full(D, np.inf, np.float32), np.full(D, -np.inf, np.float32)
        for b in range(nb):
            T, TQ = T + S[b], TQ + Q[b]
            tmn = np.where(MN[b] < tmn, MN[b], tmn)
            tmx = np.where(MX[b] > tmx, MX[b], tmx)
    return cnt.sum(axis=(0, 1)), bad.sum(axis=(0, 1)), out.sum(axis=(0, 1)), T, TQ, tmn, tmx


def monitor_rows_numpy(detector: Detector, rows: np.ndarray, block_rows: int, engine=None) -> DriftReport:
    """The monitoring rule, step by step, on the host (the oracle of
    ``monitor_rows_kernel`` and what ``TorchEngine.monitor_rows`` runs):
    ``monitor_feature_stats`` on the standardised rows, ``score_rows_numpy``
    for the cleaned scores and the alarm count, ``score_bins`` for the
    histogram.  ``engine``: as in ``score_rows_numpy``."""
    det = detector
    R = check_block_rows(block_rows)
    rows = np.asarray(rows)
    x = det.standardise(rows)
    base = det.baseline
    stats = monitor_feature_stats(x, R, base.feat_lo if base is not None else None,
                                  base.feat_hi if base is not None else None)
    scores, _, alarms = score_rows_numpy(det, rows, engine=engine)
    hist = score_bins(scores, base.score_edges) if base is not None else None
    return drift_report(det, x.shape[0], R, *stats, alarms, hist)


# ---------------------------------------------------------------------------
# grouping alarms into incidents (README "Incidents")
INCIDENT_MAX_WINDOW = 4096
INCIDENT_MAX_HOLD = 4096
INCIDENT_MAX_ROWS = (1 << 31) - 16384   # n stays below it: a row index plus one span and its halo fits 32 bits


@dataclass
class Incidents:
    """What ``Engine.incidents`` returns per item (numpy): the incidents of one
    row sequence under the rule of README "Incidents", in row order."""
    n: int
    window: int
    min_alarms: int
    hold: int
    start: np.ndarray        # int64 [k]: first hot row of incident k
    end: np.ndarray          # int64 [k]: last hot row
    alarms: np.ndarray       # int64 [k]: flagged rows in [max(0, start - window + 1), end]
    peak_row: np.ndarray     # int64 [k]: the smallest row of [start, end] holding the range's largest score
    peak_score: np.ndarray   # float64 [k]: scores[peak_row], its bits as stored
    hot_rows: int
    count: int
    rows_covered: int        # sum of end - start + 1
    longest: int             # largest end - start + 1 (0 without an incident)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_incident_params(window, min_alarms, hold=0):
    """``(window, min_alarms, hold)`` as ints; ValueError outside ``1 <= window
    <= 4096``, ``1 <= min_alarms <= window``, ``0 <= hold <= 4096``."""
    if not _is_int(window) or not 1 <= int(window) <= INCIDENT_MAX_WINDOW:
        raise ValueError(f"incidents: window must be an integer in 1..{INCIDENT_MAX_WINDOW}, got {window!r}")
    if not _is_int(min_alarms) or not 1 <= int(min_alarms) <= int(window):
        raise ValueError(f"incidents: min_alarms must be an integer in 1..window ({int(window)}), got {min_alarms!r}")
    if not _is_int(hold) or not 0 <= int(hold) <= INCIDENT_MAX_HOLD:
        raise ValueError(f"incidents: hold must be an integer in 0..{INCIDENT_MAX_HOLD}, got {hold!r}")
    return int(window), int(min_alarms), int(hold)


def check_incident_rows(flags_shape, scores_shape) -> int:
    """The row count of one ``(flags, scores)`` item; ValueError unless both
    are vectors of one length below ``INCIDENT_MAX_ROWS``."""
    fs, ss = tuple(flags_shape), tuple(scores_shape)
    if len(fs) != 1 or len(ss) != 1:
        raise ValueError(f"incidents: flags and scores must be vectors, got shapes {fs} and {ss}")
    if fs != ss:
        raise ValueError(f"incidents: {fs[0]} flags for {ss[0]} scores")
    if fs[0] >= INCIDENT_MAX_ROWS:
        raise ValueError(f"incidents: at most {INCIDENT_MAX_ROWS - 1} rows per item, got {fs[0]}")
    return int(fs[0])


def incident_bound(n: int, hold: int) -> int:
    """The most incidents ``n`` rows can hold: starts lie at least ``hold + 2`` apart."""
    return (int(n) + int(hold) + 1) // (int(hold) + 2)


def empty_incidents(n: int, window: int, min_alarms: int, hold: int, hot_rows: int = 0) -> Incidents:
    z = np.zeros(0, np.int64)
    return Incidents(n=int(n), window=window, min_alarms=min_alarms, hold=hold, start=z, end=z.copy(),
                     alarms=z.copy(), peak_row=z.copy(), peak_score=np.zeros(0, np.float64), hot_rows=int(hot_rows),
                     count=0, rows_covered=0, longest=0)


def incidents_numpy(flags, scores, window, min_alarms, hold=0) -> Incidents:
    """The incident rule on the host, with cumulative sums (the oracle of the
    kernels in fedmx_incident.hip and what ``TorchEngine.incidents`` runs).
    ``flags``: any non-zero value counts as 1; ``scores`` are cleaned first
    (NaN -> 0, +-inf -> +-DBL_MAX).  With ``P`` the prefix count of the flags
    and ``H`` that of the hot rows: ``cnt[i] = P[i + 1] - P[max(0, i - w + 1)]``,
    ``hot = cnt >= m``, a start is a hot row with ``H[i] == H[max(0, i - h -
    1)]``, an end one with ``H[min(n, i + h + 2)] == H[i + 1]``; per incident
    ``alarms = P[end + 1] - P[max(0, start - w + 1)]`` and the peak is the
    first row of ``[start, end]`` whose score equals the range's maximum
    (compared by value: -0.0 equals +0.0)."""
    w, m, h = check_incident_params(window, min_alarms, hold)
    f = np.asarray(flags)
    s = np.asarray(scores)
    n = check_incident_rows(f.shape, s.shape)
    if n == 0:
        return empty_incidents(0, w, m, h)
    s = np.nan_to_num(s.astype(np.float64))
    idx = np.arange(n, dtype=np.int64)
    P = np.concatenate([np.zeros(1, np.int64), np.cumsum(f != 0, dtype=np.int64)])
    hot = P[idx + 1] - P[np.maximum(idx - w + 1, 0)] >= m
    H = np.concatenate([np.zeros(1, np.int64), np.cumsum(hot, dtype=np.int64)])
    start = np.flatnonzero(hot & (H[idx] == H[np.maximum(idx - h - 1, 0)])).astype(np.int64)
    end = np.flatnonzero(hot & (H[np.minimum(idx + h + 2, n)] == H[idx + 1])).astype(np.int64)
    k = int(start.shape[0])
    if end.shape[0] != k or k > incident_bound(n, h):
        raise AssertionError("incidents: starts and ends do not pair up")   # (the rule excludes it)
    if k == 0:
        return empty_incidents(n, w, m, h, hot_rows=int(H[n]))
    alarms = P[end + 1] - P[np.maximum(start - w + 1, 0)]
    # the range maxima: reduceat over [s0, e0 + 1, s1, e1 + 1, ...] (strictly rising; a sentinel covers e + 1 == n)
    cuts = np.stack([start, end + 1], axis=1).reshape(-1)
    top = np.maximum.reduceat(np.concatenate([s, [-np.inf]]), cuts)[0::2]
    # rows inside an incident, and which: starts at or before the row, ends before it
    n_start = np.cumsum(np.bincount(start, minlength=n))
    n_end = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.bincount(end, minlength=n))[:-1]])
    inside = n_start > n_end
    cand = np.flatnonzero(inside & (s == top[np.maximum(n_start - 1, 0)]))
    which, first = np.unique(n_start[cand] - 1, return_index=True)
    if which.shape[0] != k:
        raise AssertionError("incidents: an incident without a peak")
    peak_row = cand[first].astype(np.int64)
    length = end - start + 1
    return Incidents(n=n, window=w, min_alarms=m, hold=h, start=start, end=end, alarms=alarms.astype(np.int64),
                     peak_row=peak_row, peak_score=s[peak_row].copy(), hot_rows=int(H[n]), count=k,
                     rows_covered=int(length.sum()), longest=int(length.max()))


def incident_min_alarms(window, rate, tail) -> int:
    """The smallest ``m`` in ``1..window`` with ``P[Binomial(window, rate) >=
    m] <= tail``, in float64 on the host (``window`` if no m reaches ``tail``).

    The model behind it: benign flags are independent draws at ``rate = 1 -
    detect_quantile``.  Real traffic is correlated in time, so the value is a
    starting point for tuning ``min_alarms``, not a guarantee on the rate of
    false incidents."""
    import math

    if not _is_int(window) or not 1 <= int(window) <= INCIDENT_MAX_WINDOW:
        raise ValueError(f"incident_min_alarms: window must be an integer in 1..{INCIDENT_MAX_WINDOW}, got {window!r}")
    w, rate, tail = int(window), float(rate), float(tail)
    if not 0.0 <= rate <= 1.0:
        raise ValueError(f"incident_min_alarms: rate must lie in [0, 1], got {rate!r}")
    if not 0.0 < tail < 1.0:
        raise ValueError(f"incident_min_alarms: tail must lie in (0, 1), got {tail!r}")
    if rate == 0.0:
        return 1
    if rate == 1.0:
        return w
    lr, lq = math.log(rate), math.log1p(-rate)
    lg = math.lgamma
    best, sf = w + 1, 0.0
    for j in range(w, 0, -1):   # the tail grows as j falls: summed from its small end
        sf += math.exp(lg(w + 1) - lg(j + 1) - lg(w - j + 1) + j * lr + (w - j) * lq)
        if sf > tail:
            break
        best = j
    return min(best, w)


# ---------------------------------------------------------------------------
# what an incident is about (README "Incident signatures")
SIGNATURE_MAX_INCIDENTS = 4096
SIGNATURE_TILE = 16
SIGNATURE_WAVES = 4


@dataclass
class Signatures:
    """What ``Engine.incident_signatures`` returns per detector (numpy).  The
    first block is what the rule fixes to the bit; the second is derived from
    it on the host in float64 (``signatures_report``)."""
    incidents: np.ndarray     # int64 [s]: the summarised incidents, indices into the Incidents result
    rows: np.ndarray          # int64 [s]: flagged rows inside [start, end] of each
    block_rows: int
    err_sum: np.ndarray       # float64 [s, D]: sum of fp32(r * r) over those rows, per feature
    resid_sum: np.ndarray     # float64 [s, D]: sum of r = y - x
    bad: np.ndarray           # int64 [s, D]: rows whose fp32(r * r) is NaN or +-inf (in neither sum)
    idx: np.ndarray           # int32 [s, K]: features by falling err_sum, equal ones by rising index; -1 unused
    share: np.ndarray         # float64 [s, K]: err_sum[idx] / sum of the incident's err_sum (NaN: zero total)
    mean_resid: np.ndarray    # float64 [s, K]: resid_sum[idx] / max(rows - bad[idx], 1)

    def similarity(self) -> np.ndarray:
        """float64 [s, s]: the cosines between the incidents' ``err_sum`` rows
        (NaN where a row is all zero)."""
        e = self.err_sum
        with np.errstate(all="ignore"):
            norm = np.sqrt(np.sum(e * e, axis=1))
            return (e @ e.T) / (norm[:, None] * norm[None, :])


def check_signature_which(which, count: int) -> np.ndarray:
    """The summarised incidents as int64 [s]: ``which`` (strictly rising
    indices in ``[0, count)``) or, for None, ``0..count-1``; at most
    SIGNATURE_MAX_INCIDENTS of them."""
    if which is None:
        w = np.arange(count, dtype=np.int64)
    else:
        if torch.is_tensor(which):
            which = which.detach().cpu().numpy()
        w = np.asarray(which)
        if w.ndim != 1 or (w.size and w.dtype.kind not in "iu"):
            raise ValueError(f"incident_signatures: which must be a vector of incident indices, got {w.dtype} "
                             f"{w.shape}")
        w = w.astype(np.int64)
        if w.size and (int(w.min()) < 0 or int(w.max()) >= count):
            raise ValueError(f"incident_signatures: which must lie in [0, {count})")
        if np.any(np.diff(w) <= 0):
            raise ValueError("incident_signatures: which must be strictly rising")
    if w.shape[0] > SIGNATURE_MAX_INCIDENTS:
        raise ValueError(f"incident_signatures: at most {SIGNATURE_MAX_INCIDENTS} incidents per call, got "
                         f"{w.shape[0]}")
    return w


def signature_list(flags, incidents: Incidents, which=None):
    """Step 1 of the signature rule: ``(L int64 [m], seg int32 [m], rows int64
    [s])``.  ``L``: the rising rows ``i`` with ``flags[i] != 0`` inside
    ``[start_k, end_k]`` of a chosen incident ``k``; ``seg[p]``: the position
    in ``which`` of ``L[p]``'s incident; ``rows[j]``: how many entries incident
    ``which[j]`` has.  ``which``: ``check_signature_which``."""
    f = np.asarray(flags)
    if f.ndim != 1 or f.shape[0] != incidents.n:
        raise ValueError(f"incident_signatures: flags must be a vector of the incidents' {incidents.n} rows, got "
                         f"shape {f.shape}")
    w = check_signature_which(which, incidents.count)
    s, n = int(w.shape[0]), int(f.shape[0])
    # the chosen incident of every row (-1: none): the incidents' ranges are disjoint
    step = np.zeros(n + 1, dtype=np.int64)
    np.add.at(step, incidents.start[w], np.arange(1, s + 1, dtype=np.int64))
    np.add.at(step, incidents.end[w] + 1, -np.arange(1, s + 1, dtype=np.int64))
    owner = np.cumsum(step[:n]) - 1
    L = np.flatnonzero((f != 0) & (owner >= 0)).astype(np.int64)
    seg = owner[L].astype(np.int32)
    return L, seg, np.bincount(seg, minlength=s).astype(np.int64)


def signature_sums(resid: np.ndarray, seg: np.ndarray, s: int, block_rows: int):
    """Steps 3 and 4 of the signature rule on fp32 residual rows ``[m, D]``
    (one per list position) and their incidents' positions ``seg`` (rising, in
    ``[0, s)``): ``(err_sum float64 [s, D], resid_sum float64 [s, D], bad int64
    [s, D])``.  Every stream (block b, wave w: the block's 16-position tiles
    w, w + 4, ... in rising order) is accumulated position by position into
    the partial of (b, incident, w) (all streams side by side, one position of
    each per step; pair (b, j) in slot b + j), then each pair's streams fold in
    wave order and each incident's blocks in block order."""
    R = check_block_rows(block_rows)
    r = np.asarray(resid, dtype=np.float32)
    if r.ndim != 2:
        raise ValueError(f"residual rows must be [m, D], got {r.shape}")
    m, D = r.shape
    s = int(s)
    sg = np.asarray(seg, dtype=np.int64)
    if sg.shape != (m,) or (m and (int(sg.min()) < 0 or int(sg.max()) >= s or np.any(np.diff(sg) < 0))):
        raise ValueError(f"seg must hold {m} rising incident positions in [0, {s})")
    err, res, bad = np.zeros((s, D), np.float64), np.zeros((s, D), np.float64), np.zeros((s, D), np.int64)
    if m == 0 or s == 0:
        return err, res, bad
    nb = -(-m // R)
    W = SIGNATURE_WAVES
    pe, pr = np.zeros((nb + s, W, D), np.float64), np.zeros((nb + s, W, D), np.float64)
    pb = np.zeros((nb + s, W, D), np.int64)
    blk = np.broadcast_to(np.arange(nb, dtype=np.int64)[:, None], (nb, W))
    wv = np.broadcast_to(np.arange(W, dtype=np.int64)[None, :], (nb, W))
    with np.errstate(all="ignore"):
        for p in range(R // W):   # position in the stream
            pos = blk * R + (W * (p // SIGNATURE_TILE) + wv) * SIGNATURE_TILE + p % SIGNATURE_TILE   # [nb, W]
            live = pos < np.minimum(m, (blk + 1) * R)
            if not live.any():
                break
            q = pos[live]
            slot, w_ = blk[live] + sg[q], wv[live]   # (one slot per stream: blocks and incidents both rise)
            t = r[q]
            e = t * t
            fin = np.isfinite(e)
            ce, cr = pe[slot, w_], pr[slot, w_]
            pe[slot, w_] = np.where(fin, ce + e.astype(np.float64), ce)
            pr[slot, w_] = np.where(fin, cr + t.astype(np.float64), cr)
            pb[slot, w_] += ~fin
        # streams -> (block, incident): ((p0 + p1) + p2) + p3
        E, S, B = pe[:, 0], pr[:, 0], pb[:, 0]
        for k in range(1, W):
            E, S, B = E + pe[:, k], S + pr[:, k], B + pb[:, k]
        # blocks -> incident, in block order from +0.0
        cnt = np.bincount(sg, minlength=s)
        off = np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt)])
        first, last = off[:-1] // R, np.where(cnt > 0, (off[1:] - 1) // R, off[:-1] // R - 1)
        j = np.arange(s, dtype=np.int64)
        for k in range(int((last - first).max()) + 1 if s else 0):
            on = first + k <= last
            sl = first[on] + k + j[on]
            err[on] = err[on] + E[sl]
            res[on] = res[on] + S[sl]
            bad[on] += B[sl]
    return err, res, bad


def signatures_report(incidents, rows, block_rows: int, err_sum, resid_sum, bad, top_k) -> Signatures:
    """Step 5: the ``Signatures`` of the rule's results, with the derived
    float64 values (one function for every engine)."""
    k = check_top_k(top_k)
    err = np.ascontiguousarray(err_sum, dtype=np.float64)
    res = np.ascontiguousarray(resid_sum, dtype=np.float64)
    bad = np.ascontiguousarray(bad, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    s, D = err.shape
    kk = min(k, D)
    idx = np.full((s, k), -1, dtype=np.int32)
    share, mean = np.zeros((s, k), np.float64), np.zeros((s, k), np.float64)
    if s:
        # K rounds of "the largest left, the lowest feature among equals" (argmax: the first maximum); the sums
        # are finite and not negative, so -inf marks a taken feature
        left, every = err.copy(), np.arange(s)
        order = np.zeros((s, kk), dtype=np.int64)
        for i in range(kk):
            order[:, i] = np.argmax(left, axis=1)
            left[every, order[:, i]] = -np.inf
        idx[:, :kk] = order
        with np.errstate(all="ignore"):
            share[:, :kk] = np.take_along_axis(err, order, axis=1) / err.sum(axis=1)[:, None]
            live = np.maximum(rows[:, None] - np.take_along_axis(bad, order, axis=1), 1)
            mean[:, :kk] = np.take_along_axis(res, order, axis=1) / live
    return Signatures(incidents=np.ascontiguousarray(incidents, dtype=np.int64), rows=rows, block_rows=int(block_rows),
                      err_sum=err, resid_sum=res, bad=bad, idx=idx, share=share, mean_resid=mean)


def incident_signatures_numpy(detector: Detector, rows: np.ndarray, flags, incidents: Incidents, top_k: int,
                              which=None, block_rows: Optional[int] = None, engine=None) -> Signatures:
    """The signature rule, step by step, on the host (the oracle of the
    kernels in fedmx_signature.hip and what ``TorchEngine.incident_signatures``
    runs): ``signature_list``, ``explain_rows_numpy(dense=True, which=L)``'s
    residuals, ``signature_sums``, ``signatures_report``.  ``block_rows``:
    default ``score_rows_per_block`` of the list's length.  ``engine``: as in
    ``explain_rows_numpy``."""
    k = check_top_k(top_k)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != detector.dims.d_in or rows.shape[0] != incidents.n:
        raise ValueError(f"rows must be [{incidents.n}, {detector.dims.d_in}], got {rows.shape}")
    L, seg, cnt = signature_list(flags, incidents, which)
    w = check_signature_which(which, incidents.count)
    if block_rows is None:
        from ..ops._hip import score_rows_per_block

        block_rows = score_rows_per_block(L.shape[0])
    R = check_block_rows(block_rows)
    resid = explain_rows_numpy(detector, rows, k, which=L, dense=True, engine=engine).resid_full
    return signatures_report(w, cnt, R, *signature_sums(resid, seg, w.shape[0], R), k)
