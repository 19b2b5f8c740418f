"""HIP engine: every compute primitive on hand-written gfx950 kernels.

* ``train_launch``  -> ``fedmx_train`` (persistent fused local training, one
                       workgroup per client, all selected clients in one launch;
                       results stay on the device until the next ``fetch``)
                       -- the reference's per-client epoch loop with Adam,
                       validation and patience, src/Trainer/client_trainer.py:360-419
* ``forward_rows``  -> ``fedmx_forward_rows`` (any list of model x row-block pairs)
* ``vote_scores``   -> ``fedmx_standardize_lds`` + ``fedmx_forward_rows`` +
                       ``fedmx_score_reduce`` (3 launches, no host sync)
                       -- src/Trainer/client_trainer.py:220-238 (standardised
                       voter data, batches of 128)
* ``verify_stats``  -> ``fedmx_forward_rows`` + ``fedmx_score_reduce`` + ``fedmx_param_drift``
                       -- src/Trainer/model_verifier.py:79-99
* ``adopt``         -> ``fedmx_broadcast_rows``
* ``evaluate``      -> cached plans: ``fedmx_forward_rows`` (latents / SSE of every
                       hosted client) + ``fedmx_cen_score`` (``fedmx_knn_score`` with
                       ``latent_scorer="knn"``; not in the reference) + ``fedmx_auc``
                       -- src/Evaluator/evaluator.py:56-94
                       (``detection`` / ``tpr_at_fpr``: ``fedmx_detect`` in
                       ``fedmx_auc``'s place; not in the reference)
* ``detect_metrics`` -> ``fedmx_detect`` (calibrated threshold + counts at it)
* ``score_rows``    -> ``fedmx_score_rows`` (deployed detectors: raw rows -> scores, alarm
                       flags and counts in one launch; ``fedmx_knn_score`` after it for
                       kNN detectors; not in the reference)
* ``explain_rows``  -> ``fedmx_explain_rows`` (deployed detectors: per-feature residuals of the
                       chosen raw rows and their top K in one launch; not in the reference)
* ``monitor_rows``  -> ``fedmx_monitor_rows`` (deployed detectors: per-feature statistics of the
                       standardised rows, alarm count and score histogram in one launch plus
                       the fold of the block partials; not in the reference)
* ``incidents``     -> ``fedmx_incidents`` (alarms grouped into incidents: mark, scan, emit, peak
                       and finish launches of fedmx_incident.hip; ``score_incidents`` runs them
                       behind ``fedmx_score_rows`` on the same stream; not in the reference)
* ``incident_signatures`` -> ``fedmx_incident_signatures`` (per incident and feature the float64 sums
                       of the squared and signed residuals over the incident's flagged rows:
                       ``incident_sig_kernel`` and ``incident_sig_fold_kernel``; not in the reference)
* ``weighted_sum``  -> ``fedmx_weighted_sum`` -- src/Trainer/client_trainer.py:107-130
* ``robust_aggregate`` -> ``fedmx_robust_agg`` (trimmed mean / median; not in the reference)
* ``krum_aggregate`` -> ``fedmx_krum_agg`` (Krum / Multi-Krum; not in the reference)
* ``geomed_aggregate`` -> ``fedmx_geomed_agg`` (geometric median by smoothed Weiszfeld iterations;
                       not in the reference)

Descriptor arrays are cached on the device for static work and streamed
through a pinned ring otherwise; device->host traffic goes through a pinned
stage with one event wait per protocol phase.  There is no PyTorch fallback:
a missing or failing library raises.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ..eval.metrics import DETECT_METRICS, detect_value_is_recall
from ..models.layout import P_PAD, segment_ids_padded
from ..ops import _hip, _host
from .base import Engine, TrainHandle, TrainHParams, TrainResult


class HipEngine(Engine):
    name = "hip"

    def __init__(self, dims, device):
        super().__init__(dims, device)
        if self.device.type != "cuda":
            raise RuntimeError("HipEngine requires a GPU device")
        _hip.lib()  # load (and fail loudly) up front
        self._seg = segment_ids_padded(dims).to(self.device)
        self._rt = _hip.runtime(self.device)
        self._eval_plans: Dict[str, dict] = {}
        self._vs = None

    def setup(self, *a, **k):
        super().setup(*a, **k)
        self._eval_plans = {}
        self.store._train_bufs = None

    # -- transfers -----------------------------------------------------------------
    def fetch(self, items: Sequence) -> List[np.ndarray]:
        """One stream synchronisation, then host copies.  Items are host views
        written by kernels (mapped pinned memory) or device tensors."""
        self._rt.sync()
        out = []
        for t in items:
            if isinstance(t, (np.ndarray, _VoteView, _ColView)):
                out.append(t.copy())
            else:
                out.append(t.detach().cpu().numpy())
        return out

    # -- training ------------------------------------------------------------------
    # device address of an int32 the training kernel sets to 1 when a launch
    # fails (engine/device_round.py points it at the round's error word)
    train_err_ptr = 0

    def train_launch(self, local_ids: Sequence[int], hp: TrainHParams) -> TrainHandle:
        trk, er, be = _hip.train(self.store, list(local_ids), hp, self.dims, err=self.train_err_ptr)
        return TrainHandle(list(local_ids), [trk, er, be])

    def train_collect(self, handle: TrainHandle, host: Optional[List[np.ndarray]] = None) -> TrainResult:
        if host is None:
            host = self.fetch(handle.tensors)
        tr, er, be = host
        er = er.astype(np.int64)
        if bool(np.any(er < 0)):
            # fedmx_train_hw.hip: an LDS flag hand-off or a trainer's wait for its
            # validator workgroup's decision ran out its bounded wait
            raise RuntimeError(f"fused training kernel failed (epochs_run {er.tolist()}): a wave's flag wait "
                               "or a validator decision wait timed out; results of this launch are invalid")
        track = [[(float(tr[i, e, 0]), float(tr[i, e, 1])) for e in range(int(er[i]))]
                 for i in range(len(handle.local_ids))]
        return TrainResult(handle.local_ids, er, track, be.astype(np.int64))

    def train_async(self, local_ids: Sequence[int], hp: TrainHParams):
        """Launch without reading results back (benchmarks)."""
        return self.train_launch(local_ids, hp)

    # -- primitives ----------------------------------------------------------------
    def forward_rows(self, params, items, want_sse=True, want_latent=False):
        if not items:
            return [], []
        return _hip.forward_rows(params, items, self.dims, want_sse, want_latent)

    def weighted_sum(self, stack, weights):
        return _hip.weighted_sum(stack, weights)

    def robust_aggregate(self, stack, t):
        return _hip.robust_aggregate_stack(stack, int(t))

    def krum_aggregate(self, stack, f, m):
        kept = torch.empty(int(stack.shape[0]), dtype=torch.int32, device=stack.device)
        agg = _hip.krum_aggregate_stack(stack, int(f), int(m), kept_out=kept)
        return agg, [int(i) for i in torch.nonzero(kept).flatten().tolist()]

    def geomed_aggregate(self, stack, iters, nu):
        w = torch.empty(int(stack.shape[0]), dtype=torch.float64, device=stack.device)
        agg = _hip.geomed_aggregate_stack(stack, iters, nu, weights_out=w)
        return agg, [float(x) for x in w.tolist()]

    def param_drift(self, hist, new):
        return _hip.param_drift(hist, new, self._seg)

    def cen_scores(self, train_lat, test_lat):
        return _hip.cen_scores(train_lat, test_lat, self.dims.latent)

    def knn_scores(self, train_lat, query_lat, k):
        return _hip.knn_scores(train_lat, query_lat, self.dims.latent, int(k))

    def _scorer_plan(self, train_lat, query_lat, scores_all):
        """The configured latent scorer's part of an evaluation plan:
        (descriptor blob on the device, its launcher, per-item score views)."""
        if self.latent_scorer == "knn":
            k = int(self.knn_k)
            desc, views = _hip.knn_desc(train_lat, query_lat, scores_all, self.dims.latent, k)
            n, y = len(desc), _hip.knn_grid_y(query_lat)
            blob = torch.from_numpy(desc.view(np.uint8).copy()).to(self.device)
            return blob, (lambda: _hip.launch_knn(blob, n, self.device, k=k, y=y)), views
        if self.latent_scorer != "cen":
            raise ValueError(f"unknown latent_scorer {self.latent_scorer!r}")
        desc, views = _hip.cen_desc(train_lat, query_lat, scores_all, self.dims.latent)
        n = len(desc)
        blob = torch.from_numpy(desc.view(np.uint8).copy()).to(self.device)
        return blob, (lambda: _hip.launch_cen(blob, n, self.device)), views

    def _scorer_key(self, model_type: str) -> tuple:
        """(latent_scorer, knn_k) as far as they change ``model_type``'s plan."""
        if model_type != "hybrid" or self.latent_scorer == "cen":
            return ("cen", 0)
        return (self.latent_scorer, int(self.knn_k))

    def auc(self, scores, labels):
        # the descriptors carry raw pointers: contiguous copies of strided views, made
        # once, kept until the fetch has completed and reused by the large path
        scores = [s.detach().contiguous() for s in scores]
        labels = list(labels)
        out = self.fetch([_hip.auc(scores, labels)])[0]
        return self._auc_fixup(out, scores, labels)

    def _auc_fixup(self, out, scores, labels, f32_scale: float = 1.0):
        """Entries ``auc_kernel`` answered -1 (class too large for its LDS
        sort): recomputed by the multi-workgroup path (one more launch
        sequence and fetch), read with the same ``f32_scale``; a pair beyond
        its 2^26 rows keeps the exact host path."""
        bad = np.flatnonzero(out == -1.0)
        big = [i for i in bad if int(scores[i].shape[0]) <= _hip.AUC_LARGE_MAX_ROWS]
        if big:
            vals = self.fetch([_hip.auc_large([scores[i].detach().contiguous() for i in big],
                                              [labels[i] for i in big], f32_scale)])[0]
            out[big] = vals
        for i in bad:
            if int(scores[i].shape[0]) > _hip.AUC_LARGE_MAX_ROWS:
                s = scores[i].detach().double().cpu().numpy()
                out[i] = _host.roc_auc(np.nan_to_num(s), labels[i].cpu().numpy())
        return out

    def _auc_large_plan(self, scores, labels, f32_scale: float, aucs_buf) -> Optional[dict]:
        """The large-path part of an AUC plan: the clients whose smaller test
        class is beyond ``auc_kernel``'s LDS sort (the labels are fixed, so the
        classes are counted once, here), their descriptors, one workspace and
        the launch's grid.  None when no client is large: nothing is allocated
        and nothing more is launched."""
        st = self.store
        big, m, npr = [], [], []
        for c in range(len(scores)):
            y = st.labels(c)
            P = int(np.count_nonzero(y))
            N = int(y.shape[0]) - P
            if min(P, N) > _hip.AUC_MAX_SORT and P + N <= _hip.AUC_LARGE_MAX_ROWS:
                big.append(c)
                m.append(min(P, N))
                npr.append(max(P, N))
        if not big:
            return None
        rows = [m[i] + npr[i] for i in range(len(big))]
        ws = torch.empty(sum(rows), dtype=torch.float64, device=self.device)
        ctr = torch.zeros(_hip.AUC_LARGE_CTR_WORDS * len(big), dtype=torch.int64, device=self.device)
        desc = _hip.auc_large_desc([scores[c] for c in big], [labels[c] for c in big], aucs_buf.dev_ptr,
                                   ws.data_ptr(), ctr.data_ptr(), f32_scale, out_index=big)
        chunks, slices = _hip.auc_large_grid(m, npr)
        return dict(clients=big, desc=torch.from_numpy(desc.view(np.uint8).copy()).to(self.device), ws=ws, ctr=ctr,
                    max_rows=max(rows), chunks=chunks, slices=slices)

    def store_device(self) -> torch.device:
        """The device with its index, as tensors moved to ``self.device`` report it."""
        return self._seg.device

    def _score_state(self, det):
        """The detector's constants on the device (uploaded once per detector
        object): score_rows_kernel's state and, for knn, the train latents."""
        hit = getattr(det, "_hip_state", None)
        if hit is not None and hit[0].device == self.store_device():
            hit[0].threshold = float(det.threshold)   # (the one field a user re-tunes in place)
            return hit
        sc = det.scaler
        a, b = (sc["mean_"], sc["scale_"]) if det.scaler_kind == "standard" else (sc["scale_"], sc["min_"])
        cen = det.model_type == "hybrid" and det.latent_scorer == "cen"
        kind = _hip.SCORE_KIND_AE if det.model_type == "autoencoder" else (_hip.SCORE_KIND_CEN if cen else 0)
        state = _hip.ScoreState(det.padded_params().to(self.device).contiguous(), det.dims, a, b,
                                det.scaler_kind == "minmax", kind, det.threshold,
                                det.latent_mean if cen else None, det.latent_scale if cen else None)
        train = torch.from_numpy(det.train_latents).to(self.device) if kind == 0 else None
        det._hip_state = (state, train)
        return det._hip_state

    def _rows_on_device(self, x, det=None):
        """Raw rows (numpy or a tensor; float32 / float64, anything else as
        float64) as a contiguous tensor on the device; with ``det``, checked
        to be ``[n, det.dims.d_in]``."""
        if not torch.is_tensor(x):
            x = np.ascontiguousarray(x)
            if x.dtype not in (np.float32, np.float64):
                x = x.astype(np.float64)
            x = torch.from_numpy(x)
        if det is not None and (x.dim() != 2 or x.shape[1] != det.dims.d_in):
            raise ValueError(f"rows must be [n, {det.dims.d_in}], got {tuple(x.shape)}")
        return x.to(self.device).contiguous()

    def _knn_scores_grouped(self, detectors, train_lats, lats, which):
        """``knn_score_kernel`` for the items ``which`` (indices into the three
        lists), one launch per (k, latent size): ``{item: scores on the device}``."""
        scores = {}
        for k in sorted({detectors[j].knn_k for j in which}):
            for z in sorted({detectors[j].dims.latent for j in which if detectors[j].knn_k == k}):
                js = [j for j in which if detectors[j].knn_k == k and detectors[j].dims.latent == z]
                views = _hip.knn_scores([train_lats[j] for j in js], [lats[j] for j in js], z, k)
                scores.update(zip(js, views))
        return scores

    def score_rows(self, detectors, rows, want_latents=False):
        """One ``score_rows_kernel`` launch over every detector's rows; a knn
        detector's rows leave it as latents and take ``knn_score_kernel`` after
        it (one launch per k), the clean-and-compare of those on the host."""
        from ..deploy.detector import clean_and_flag

        if len(detectors) != len(rows):
            raise ValueError("score_rows: one block of rows per detector")
        xs = [self._rows_on_device(x) for x in rows]
        out: List[Optional[tuple]] = [None] * len(detectors)
        live = [i for i, x in enumerate(xs) if x.shape[0] > 0]
        for i in set(range(len(xs))) - set(live):   # no rows: nothing to launch
            hyb = detectors[i].model_type == "hybrid"
            lat0 = (np.zeros((0, detectors[i].dims.latent), np.float32) if hyb else None,) if want_latents else ()
            if xs[i].dim() != 2 or xs[i].shape[1] != detectors[i].dims.d_in:
                raise ValueError(f"rows must be [n, {detectors[i].dims.d_in}], got {tuple(xs[i].shape)}")
            out[i] = (np.zeros(0, np.float64), np.zeros(0, np.uint8), 0) + lat0
        if not live:
            return out
        states = [self._score_state(detectors[i]) for i in live]
        res, alarms = _hip.score_rows([s for s, _ in states], [xs[i] for i in live],
                                      want_latents=want_latents)
        knn_scores = self._knn_scores_grouped([detectors[i] for i in live], [t for _, t in states],
                                              [r[2] for r in res],
                                              [j for j, (s, _) in enumerate(states) if s.kind == 0])
        self._rt.sync()
        counts = alarms.cpu().numpy()
        for j, i in enumerate(live):
            sc, fl, la = res[j]
            la = la.cpu().numpy() if (la is not None and want_latents) else None
            if j in knn_scores:
                s, f, a = clean_and_flag(knn_scores[j].cpu().numpy(), detectors[i].threshold)
            else:
                s, f, a = sc.cpu().numpy(), fl.cpu().numpy(), int(counts[j])
            if want_latents and detectors[i].model_type != "hybrid":
                la = None
            out[i] = (s, f, a) + ((la,) if want_latents else ())
        return out

    def explain_rows(self, detectors, rows, top_k=5, which=None, dense=False):
        """One ``explain_rows_kernel`` launch over every detector's chosen rows
        (``_hip.explain_rows`` checks ``top_k`` and ``which``; an item with
        nothing to explain gets no workgroup, and nothing at all launches nothing)."""
        from ..deploy.detector import Explanation

        which = list(which) if which is not None else [None] * len(detectors)
        if len(detectors) != len(rows) or len(which) != len(detectors):
            raise ValueError("explain_rows: one block of rows (and one which) per detector")
        if not detectors:
            return []
        xs = [self._rows_on_device(x, det) for det, x in zip(detectors, rows)]
        res = _hip.explain_rows([self._score_state(det)[0] for det in detectors], xs, top_k, which=which, dense=dense)
        for r, x in zip(res, xs):   # (formed while the launch runs)
            if r["rows"] is None:
                r["rows"] = np.arange(int(x.shape[0]), dtype=np.int64)
        self._rt.sync()

        def host(t):
            return t.cpu().numpy() if t is not None else None

        return [Explanation(rows=r["rows"], idx=host(r["idx"]), resid=host(r["resid"]), sse=host(r["sse"]),
                            resid_full=host(r["resid_full"]), latent_terms=host(r["latent_terms"])) for r in res]

    def monitor_rows(self, detectors, rows, block_rows=None):
        """One ``monitor_rows_kernel`` launch over every detector's rows and
        the ``monitor_fold_kernel`` launch behind it; a knn detector's rows
        leave the first as latents and take ``knn_score_kernel`` after it, the
        clean, compare and bin of those on the host.  An item without rows
        gets no workgroup, and a call without rows launches nothing."""
        from ..deploy.detector import check_block_rows, clean_and_flag, drift_report, score_bins

        if len(detectors) != len(rows):
            raise ValueError("monitor_rows: one block of rows per detector")
        if not detectors:
            return []
        xs = [self._rows_on_device(x, det) for det, x in zip(detectors, rows)]
        rpb = check_block_rows(block_rows if block_rows is not None
                               else _hip.score_rows_per_block(sum(int(x.shape[0]) for x in xs)))

        def initial(det):   # nothing ran: the rule's initial values
            D, base = det.dims.d_in, det.baseline
            stats = (np.zeros(D, np.int64), np.zeros(D, np.int64), np.zeros(D, np.int64), np.zeros(D), np.zeros(D),
                     np.full(D, np.inf, np.float32), np.full(D, -np.inf, np.float32))
            h = np.zeros(base.score_edges.shape[0] + 1, np.int64) if base is not None else None
            return drift_report(det, 0, rpb, *stats, 0, h)

        if not any(x.shape[0] > 0 for x in xs):
            return [initial(det) for det in detectors]
        states = [self._score_state(det) for det in detectors]
        for det, (st, _) in zip(detectors, states):
            # the band and the edges: uploaded when they differ from what the device holds (at most 271 values)
            base = det.baseline
            key = None if base is None else (base.feat_lo.tobytes(), base.feat_hi.tobytes(), base.score_edges.tobytes())
            if key != getattr(st, "baseline_key", None):
                if base is None:
                    st.band = st.edges = None
                    st.nedges = -1
                else:
                    st.set_baseline(base.feat_lo, base.feat_hi, base.score_edges)
                st.baseline_key = key
        total, alarms, hist, lats, rpb, part = _hip.monitor_rows([s for s, _ in states], xs, rows_per_block=rpb)
        knn_scores = self._knn_scores_grouped(detectors, [t for _, t in states], lats,
                                              [i for i, (s, _) in enumerate(states)
                                               if s.kind == 0 and xs[i].shape[0] > 0])
        self._rt.sync()
        tot = total.cpu().numpy().view(_hip.MONITOR_TOTAL_DTYPE)
        counts, hists = alarms.cpu().numpy(), hist.cpu().numpy()
        del part
        out = []
        for i, det in enumerate(detectors):
            n, D, base = int(xs[i].shape[0]), det.dims.d_in, det.baseline
            if n == 0:
                out.append(initial(det))
                continue
            t = tot[i]
            stats = tuple(t[k][:D].copy() for k in ("cnt", "bad", "out", "sum", "sq", "mn", "mx"))
            if i in knn_scores:
                s, _, a = clean_and_flag(knn_scores[i].cpu().numpy(), det.threshold)
                h = score_bins(s, base.score_edges) if base is not None else None
            else:
                a = int(counts[i])
                h = hists[i, :base.score_edges.shape[0] + 1].copy() if base is not None else None
            out.append(drift_report(det, n, rpb, *stats, a, h))
        return out

    def _incident_inputs(self, flags, scores):
        """One ``(flags, scores)`` item as contiguous uint8 / float64 vectors on
        the device (a non-zero flag of any type becomes 1)."""
        def dev(v):
            return v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))

        f, s = dev(flags), dev(scores)
        _hip.check_incident_rows(f.shape, s.shape)
        if f.dtype != torch.uint8:
            f = (f != 0).to(torch.uint8)
        return f.to(self.device).contiguous(), s.to(self.device, torch.float64).contiguous()

    def _incident_results(self, res, sizes, w, m, h):
        """The ``Incidents`` of ``_hip.incidents``' device results (the stream
        is synchronised): the counts first, then that many entries per field."""
        from ..deploy.detector import Incidents, empty_incidents

        out = []
        for o, n in zip(res, sizes):
            if o is None:
                out.append(empty_incidents(0, w, m, h))
                continue
            hot, k, covered, longest = (int(v) for v in o["summary"].cpu().numpy())
            a = o["out"][:, :k].cpu().numpy()
            p = o["peak"][:, :k].cpu().numpy()
            out.append(Incidents(n=n, window=w, min_alarms=m, hold=h, start=a[0].copy(), end=a[1].copy(),
                                 alarms=a[3].copy(), peak_row=p[1].copy(), peak_score=p[0].copy().view(np.float64),
                                 hot_rows=hot, count=k, rows_covered=covered, longest=longest))
        return out

    def incidents(self, flags, scores, window, min_alarms, hold=0):
        """The five launches of fedmx_incident.hip over every item's rows, one
        synchronisation after them; an item without rows gets no workgroup and
        a call without rows launches nothing."""
        w, m, h = _hip.check_incident_params(window, min_alarms, hold)
        if len(flags) != len(scores):
            raise ValueError("incidents: one scores vector per flags vector")
        pairs = [self._incident_inputs(f, s) for f, s in zip(flags, scores)]
        sizes = [int(f.shape[0]) for f, _ in pairs]
        if not any(sizes):
            return self._incident_results([None] * len(pairs), sizes, w, m, h)
        res = _hip.incidents([f for f, _ in pairs], [s for _, s in pairs], w, m, h)
        self._rt.sync()
        return self._incident_results(res, sizes, w, m, h)

    def score_incidents(self, detectors, rows, window, min_alarms, hold=0):
        """``score_rows``' launches, then the incident launches on the scores
        and flags they left on the device: same stream, one synchronisation
        at the end.  A knn detector's scores are cleaned and flagged on the
        host as in ``score_rows`` (one synchronisation more) and uploaded."""
        from ..deploy.detector import clean_and_flag

        w, m, h = _hip.check_incident_params(window, min_alarms, hold)
        if len(detectors) != len(rows):
            raise ValueError("score_rows: one block of rows per detector")
        xs = [self._rows_on_device(x, det) for det, x in zip(detectors, rows)]
        sizes = [int(x.shape[0]) for x in xs]
        live = [i for i, n in enumerate(sizes) if n > 0]
        empty = (np.zeros(0, np.float64), np.zeros(0, np.uint8), 0)
        if not live:
            inc = self._incident_results([None] * len(xs), sizes, w, m, h)
            return [empty + (i,) for i in inc]
        states = [self._score_state(detectors[i]) for i in live]
        res, alarms = _hip.score_rows([s for s, _ in states], [xs[i] for i in live])
        knn = [j for j, (s, _) in enumerate(states) if s.kind == 0]
        knn_scores = self._knn_scores_grouped([detectors[i] for i in live], [t for _, t in states],
                                              [r[2] for r in res], knn)
        host = {}
        sc_dev, fl_dev = [r[0] for r in res], [r[1] for r in res]
        if knn:
            self._rt.sync()
            for j in knn:
                host[j] = clean_and_flag(knn_scores[j].cpu().numpy(), detectors[live[j]].threshold)
                sc_dev[j] = torch.from_numpy(host[j][0]).to(self.device)
                fl_dev[j] = torch.from_numpy(host[j][1]).to(self.device)
        inc_dev = _hip.incidents(fl_dev, sc_dev, w, m, h)
        self._rt.sync()
        counts = alarms.cpu().numpy()
        inc = self._incident_results(inc_dev, [sizes[i] for i in live], w, m, h)
        out = [None] * len(xs)
        for j, i in enumerate(live):
            s, f, a = host[j] if j in host else (sc_dev[j].cpu().numpy(), fl_dev[j].cpu().numpy(), int(counts[j]))
            out[i] = (s, f, a, inc[j])
        for i in set(range(len(xs))) - set(live):
            out[i] = empty + (self._incident_results([None], [0], w, m, h)[0],)
        return out

    def incident_signatures(self, detectors, rows, flags, incidents, top_k=5, which=None, block_rows=None):
        """The list of flagged rows inside the chosen incidents is formed on
        the host from the flags and uploaded; then ``incident_sig_kernel`` over
        every detector's list and ``incident_sig_fold_kernel`` behind it, one
        synchronisation after them.  An item without a list position gets no
        workgroup, and a call without one launches nothing."""
        from ..deploy.detector import (check_block_rows, check_signature_which, check_top_k, signature_list,
                                       signatures_report)

        k = check_top_k(top_k)
        which = list(which) if which is not None else [None] * len(detectors)
        if not (len(rows) == len(flags) == len(incidents) == len(which) == len(detectors)):
            raise ValueError("incident_signatures: one rows / flags / incidents (and which) entry per detector")
        if not detectors:
            return []
        xs = [self._rows_on_device(x, det) for det, x in zip(detectors, rows)]
        lists, segs, counts, picked = [], [], [], []
        for x, f, inc, w in zip(xs, flags, incidents, which):
            f = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
            if int(x.shape[0]) != inc.n:
                raise ValueError(f"rows must be [{inc.n}, D], got {tuple(x.shape)}")
            L, seg, cnt = signature_list(f, inc, w)
            lists.append(L)
            segs.append(seg)
            counts.append(cnt)
            picked.append(check_signature_which(w, inc.count))
        rpb = check_block_rows(block_rows if block_rows is not None
                               else _hip.score_rows_per_block(sum(int(L.shape[0]) for L in lists)))
        if not any(L.shape[0] for L in lists):   # nothing to reduce: the rule's initial values
            return [signatures_report(w, cnt, rpb, np.zeros((len(w), det.dims.d_in)), np.zeros((len(w), det.dims.d_in)),
                                      np.zeros((len(w), det.dims.d_in), np.int64), k)
                    for det, w, cnt in zip(detectors, picked, counts)]
        offsets = [np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt)]) for cnt in counts]
        res = _hip.incident_signatures([self._score_state(det)[0] for det in detectors], xs, lists, segs, offsets, rpb)
        self._rt.sync()
        return [signatures_report(w, cnt, rpb, r["err_sum"].cpu().numpy(), r["resid_sum"].cpu().numpy(),
                                  r["bad"].cpu().numpy(), k) for r, w, cnt in zip(res, picked, counts)]

    def standardize_ddof1(self, x):
        return _hip.standardize_ddof1(x.contiguous(), self.dims.d_in)

    # -- round operations ------------------------------------------------------------
    def standardized_vote_data(self, vote_data):
        """Vote data standardised (ddof 1) into a persistent device buffer (stream-ordered reuse)."""
        if self._vs is None or self._vs.shape[0] < vote_data.shape[0]:
            self._vs = torch.empty(max(vote_data.shape[0], 256), 128, dtype=torch.float32, device=self.device)
        vs = self._vs[:vote_data.shape[0]]
        _hip.standardize_ddof1(vote_data.contiguous(), self.dims.d_in, out=vs)
        return vs

    def vote_scores(self, local_rows, vote_data, dev_set, vote_bs):
        """Host view [k, 2] (vote score, dev MSE) written by the kernels."""
        k = len(local_rows)
        if k == 0:
            return np.zeros((0, 2), dtype=np.float64)
        vs = self.standardized_vote_data(vote_data)
        items = [(c, vs) for c in local_rows]
        if dev_set is not None:
            items += [(c, dev_set) for c in local_rows]
        sse, _ = _hip.forward_rows(self.store.params, items, self.dims, True, False)
        red = _hip.score_reduce(sse, [vote_bs] * k + [0] * (len(sse) - k), self.dims.d_in)
        return _VoteView(red, k, dev_set is not None)

    def verify_stats(self, agg, datasets, hist):
        """(host view of MSEs, host view of drifts) written by the kernels."""
        if datasets:
            sse, _ = _hip.forward_rows(agg.unsqueeze(0), [(0, x) for x in datasets], self.dims, True, False)
            mse = _ColView(_hip.score_reduce(sse, [0] * len(sse), self.dims.d_in), 1)
        else:
            mse = np.zeros(0, dtype=np.float64)
        if hist is not None and hist.shape[0]:
            drift = _hip.param_drift(hist, agg, self._seg, to_host=True)
        else:
            drift = np.zeros(0, dtype=np.float32)
        return mse, drift

    def model_mse(self, local_rows, datasets):
        if not len(local_rows):
            return np.zeros(0)
        sse, _ = _hip.forward_rows(self.store.params, list(zip(local_rows, datasets)), self.dims, True, False)
        red = _hip.score_reduce(sse, [0] * len(sse), self.dims.d_in)
        return self.fetch([_ColView(red, 1)])[0]

    def adopt(self, local_rows, agg, anchor=True):
        st = self.store
        _hip.broadcast_rows(st.params, st.anchor if anchor else None, list(local_rows), agg)

    def _plan(self, model_type: str, params: Optional[torch.Tensor] = None, metric: str = "AUC",
              grid: Optional[tuple] = None) -> dict:
        """Cached evaluation launch plan; ``params`` (default: the live client
        parameters) is the [C, P] buffer the forward reads.  ``metric``: "AUC",
        or one of eval.metrics.DETECT_METRICS (``_detect_plan``)."""
        params = self.store.params if params is None else params
        if metric in DETECT_METRICS:
            return self._detect_plan(model_type, params, metric, grid)
        key = (model_type, params.data_ptr(), *self._scorer_key(model_type))
        p = self._eval_plans.get(key)
        if p is not None:
            return p
        st = self.store
        C = st.num_clients
        labels = [st.label_view(c) for c in range(C)]
        aucs_buf = _hip._hiprt.MappedBuffer(max(8 * C, 64))   # AUCs written straight to host memory
        aucs = aucs_buf.view(0, np.float64, C)
        if model_type == "hybrid":
            items = []
            for c in range(C):
                items += [(c, st.rows("train", c)), (c, st.rows("test", c))]
            fwd = _hip.FwdPlan(params, items, self.dims, want_sse=False, want_latent=True)
            lat = fwd.lat_views()
            scores_all = torch.empty(sum(int(st.test_off[c + 1] - st.test_off[c]) for c in range(C)),
                                     dtype=torch.float64, device=self.device)
            blob, launch, scores = self._scorer_plan(lat[0::2], lat[1::2], scores_all)
            scale = 1.0
            p = dict(fwd=fwd, scorer=blob, score_launch=launch, scores=scores, test_lat=lat[1::2])
        elif model_type == "autoencoder":
            fwd = _hip.FwdPlan(params, [(c, st.rows("test", c)) for c in range(C)], self.dims,
                               want_sse=True, want_latent=False)
            scores = fwd.sse_views()
            scale = 1.0 / self.dims.d_in
            p = dict(fwd=fwd, scorer=None, score_launch=None, scores=scores, test_lat=None)
        else:
            raise ValueError(f"unknown model_type {model_type!r}")
        adesc = _hip.auc_desc(scores, labels, aucs_buf.dev_ptr, scale)
        p["auc"] = torch.from_numpy(adesc.view(np.uint8).copy()).to(self.device)
        # clients beyond auc_kernel's LDS sort: the multi-workgroup path after it, on the
        # same stream, overwrites their -1 in aucs_buf (None: no such client, nothing added)
        p["auc_large"] = self._auc_large_plan(scores, labels, scale, aucs_buf)
        p["auc_scale"] = scale
        p["aucs"] = aucs
        p["aucs_buf"] = aucs_buf
        p["labels"] = labels
        self._eval_plans[key] = p
        return p

    def _detect_plan(self, model_type: str, params: torch.Tensor, metric: str, grid: Optional[tuple]) -> dict:
        """The evaluation plan of a calibrated-threshold metric: the AUC
        plan's forward (plus every client's validation rows for ``detection``),
        for ``hybrid`` the latent scorer's distances (CEN or kNN) of the test rows and, for
        ``detection``, of the validation rows under the same train-latent
        scaler (a second descriptor per client), then one ``detect_kernel``
        descriptor per client.  The [8][C] results land in mapped host memory;
        with ``grid = (N, first)`` in a zeroed [8][N] device tensor at columns
        ``first ..`` instead (the device round's multi-rank all-reduce)."""
        from ..eval.evaluator import detection_ranks

        key = (model_type, params.data_ptr(), metric, float(self.detect_quantile), float(self.target_fpr), grid,
               *self._scorer_key(model_type))
        p = self._eval_plans.get(key)
        if p is not None:
            return p
        if model_type not in ("hybrid", "autoencoder"):
            raise ValueError(f"unknown model_type {model_type!r}")
        st = self.store
        C = st.num_clients
        ids = list(range(C))
        labels = [st.label_view(c) for c in ids]
        with_valid = metric == "detection"
        splits = (["train"] if model_type == "hybrid" else []) + ["test"] + (["valid"] if with_valid else [])
        m = len(splits)
        items = [(c, st.rows(s, c)) for c in ids for s in splits]
        if model_type == "hybrid":
            fwd = _hip.FwdPlan(params, items, self.dims, want_sse=False, want_latent=True)
            lat = fwd.lat_views()
            tr, test_lat = lat[0::m], lat[1::m]
            n_scores = sum(int(l.shape[0]) for l in lat[1::m]) + (sum(int(l.shape[0]) for l in lat[2::m])
                                                                  if with_valid else 0)
            scores_all = torch.empty(n_scores, dtype=torch.float64, device=self.device)
            # test rows first, then (detection) the validation rows: 2 C descriptors, one launch
            blob, launch, views = self._scorer_plan(list(tr) * (2 if with_valid else 1),
                                                    list(test_lat) + (list(lat[2::m]) if with_valid else []),
                                                    scores_all)
            scores = views[:C]
            calib = views[C:] if with_valid else scores
            scale = 1.0
        else:
            fwd = _hip.FwdPlan(params, items, self.dims, want_sse=True, want_latent=False)
            sse = fwd.sse_views()
            scores, test_lat = sse[0::m], None
            calib = sse[1::m] if with_valid else scores
            blob, launch, scale = None, None, 1.0 / self.dims.d_in
        if grid is None:
            det_buf = _hip._hiprt.MappedBuffer(max(8 * 8 * C, 64))   # [8][C], written straight to host memory
            det = det_buf.view(0, np.float64, 8 * C).reshape(8, C)
            det[:] = np.nan
            out_ptr, stride, det_dev = det_buf.dev_ptr, C, None
        else:
            N, first = int(grid[0]), int(grid[1])
            if first < 0 or first + C > N:
                raise ValueError(f"detect plan: columns {first}..{first + C} do not fit {N} clients")
            det_buf, det = None, None
            det_dev = torch.zeros(8 * max(N, 1), dtype=torch.float64, device=self.device)
            out_ptr, stride = det_dev.data_ptr() + 8 * first, N
        ddesc = _hip.detect_desc(calib, scores, labels, detection_ranks(self, ids, metric), out_ptr, max(stride, C),
                                 calib_labels=None if with_valid else labels, f32_scale=scale,
                                 value_is_recall=not with_valid)
        p = dict(fwd=fwd, scorer=blob, score_launch=launch, scores=scores, calib=calib, test_lat=test_lat, labels=labels,
                 detect=torch.from_numpy(ddesc.view(np.uint8).copy()).to(self.device), det=det, det_buf=det_buf,
                 det_dev=det_dev, value_ptr=out_ptr, aucs=None if det is None else det[0])
        self._eval_plans[key] = p
        return p

    def evaluate_launch(self, model_type: str, params: Optional[torch.Tensor] = None, metric: str = "AUC",
                        grid: Optional[tuple] = None) -> np.ndarray:
        """Enqueue the full evaluation of every hosted client; returns the
        host view of the metric (float64 [C], valid after the next sync; None
        for a ``grid`` plan, whose results stay on the device).  ``metric``:
        "AUC" (forward [+ latent scorer] + ``auc_kernel``) or a calibrated-threshold
        metric (``detect_kernel`` in ``auc_kernel``'s place)."""
        p = self._plan(model_type, params, metric, grid)
        p["fwd"].run()
        if p["score_launch"] is not None:
            p["score_launch"]()
        if metric in DETECT_METRICS:
            _hip.launch_detect(p["detect"], self.store.num_clients, self.device)
        else:
            _hip.launch_auc(p["auc"], self.store.num_clients, self.device)
            big = p["auc_large"]
            if big is not None:
                _hip.launch_auc_large(big["desc"], len(big["clients"]), big["max_rows"], big["chunks"], big["slices"],
                                      self.device)
        return p["aucs"]

    def detect_metrics(self, calib, scores, labels, ranks, calib_labels=None, score_scale=1.0, value="f1"):
        if not len(scores):
            return np.zeros((8, 0), dtype=np.float64)
        view = _hip.detect(list(calib), list(scores), list(labels), [int(j) for j in ranks],
                           None if calib_labels is None else list(calib_labels), float(score_scale),
                           detect_value_is_recall(value))
        self._rt.sync()
        return np.array(view, dtype=np.float64)

    def evaluate(self, model_type: str, metric: str = "AUC", keep_latents: bool = False):
        from ..eval.evaluator import EvalResult, detection_result, evaluate_clients

        if metric in DETECT_METRICS:
            self.evaluate_launch(model_type, metric=metric)
            p = self._plan(model_type, metric=metric)
            self._rt.sync()
            return detection_result(np.array(p["det"], dtype=np.float64), self._plan_latents(p, keep_latents))
        if metric != "AUC":
            return evaluate_clients(self, list(range(self.store.num_clients)), model_type, metric, keep_latents)
        aucs = self.evaluate_launch(model_type)
        p = self._plan(model_type)
        vals = self._auc_fixup(self.fetch([aucs])[0], p["scores"], p["labels"], p["auc_scale"])
        return EvalResult(np.asarray(vals, dtype=np.float64), {}, self._plan_latents(p, keep_latents))

    def _plan_latents(self, p: dict, keep_latents: bool):
        if not keep_latents or p["test_lat"] is None:
            return None
        st = self.store
        return [(l.detach().cpu().numpy().astype(np.float32), st.labels(c).astype(np.float32))
                for c, l in enumerate(p["test_lat"])]


class _VoteView:
    """Lazy [k, 2] view over score_reduce output: (vote score of the vote
    segments, dev MSE of the dev segments)."""

    def __init__(self, red: np.ndarray, k: int, has_dev: bool):
        self.red, self.k, self.has_dev = red, k, has_dev

    def copy(self):
        out = np.full((self.k, 2), np.nan)
        out[:, 0] = self.red[:self.k, 0]
        if self.has_dev:
            out[:, 1] = self.red[self.k:2 * self.k, 1]
        return out


class _ColView:
    def __init__(self, a: np.ndarray, col: int):
        self.a, self.col = a, col

    def copy(self):
        return self.a[:, self.col].copy()
