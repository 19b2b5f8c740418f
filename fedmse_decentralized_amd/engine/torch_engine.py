"""Pure-PyTorch engine: the reference-exact execution path.

Runs on CPU (tests, plumbing config 1 of BASELINE.json) or any torch device.
It is the numerical oracle the HIP kernels are tested against, so it follows
the reference math literally: sequential clients, canonical parameter
tensors, autograd, ``torch.optim.Adam``'s single-tensor update formula with
persistent state (`src/Trainer/client_trainer.py:66`, `:360-419`, Q10),
mean-of-batch-mean epoch losses, patience-based early stopping.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from ..models.layout import P_PAD, canonical_to_padded, padded_to_canonical
from ..models.reference import functional_forward, functional_loss, unflatten
from ..ops import _host
from .base import Engine, TrainHandle, TrainHParams, TrainResult


def _adam_update(p, g, m, v, step, hp: TrainHParams):
    """torch.optim.adam._single_tensor_adam (no weight decay, no amsgrad)."""
    m.lerp_(g, 1 - hp.beta1)
    v.mul_(hp.beta2).addcmul_(g, g, value=1 - hp.beta2)
    bc1 = 1 - hp.beta1 ** step
    bc2 = 1 - hp.beta2 ** step
    step_size = hp.lr / bc1
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(hp.eps)
    p.addcdiv_(m, denom, value=-step_size)


class TorchEngine(Engine):
    name = "torch"

    # -- training --------------------------------------------------------------
    def train_launch(self, local_ids: Sequence[int], hp: TrainHParams) -> TrainHandle:
        return TrainHandle(list(local_ids), [], self._train_eager(local_ids, hp))

    def train_collect(self, handle: TrainHandle, host=None) -> TrainResult:
        return handle.result

    def _train_eager(self, local_ids: Sequence[int], hp: TrainHParams) -> TrainResult:
        st = self.store
        D = self.dims.d_in
        k = len(local_ids)
        epochs_run = np.zeros(k, dtype=np.int64)
        best_epoch = np.full(k, -1, dtype=np.int64)
        tracking: List[List[Tuple[float, float]]] = []
        for i, c in enumerate(local_ids):
            flat = padded_to_canonical(st.params[c], self.dims)
            params = [t.clone() for t in unflatten(flat, self.dims)]
            for t in params:
                t.requires_grad_(True)
            m = [t.clone() for t in unflatten(padded_to_canonical(st.adam_m[c], self.dims), self.dims)]
            v = [t.clone() for t in unflatten(padded_to_canonical(st.adam_v[c], self.dims), self.dims)]
            anchor = [t.clone() for t in unflatten(padded_to_canonical(st.anchor[c], self.dims), self.dims)]
            step = int(st.adam_step[c].item())
            xt = st.rows("train", c)[:, :D]
            xv = st.rows("valid", c)[:, :D]
            B = hp.batch_size
            min_valid = float("inf")
            worse = 0
            track = []
            for ep in range(hp.epochs):
                epoch_loss = 0.0
                nb = 0
                for s in range(0, xt.shape[0], B):
                    x = xt[s:s + B]
                    z, y = functional_forward(params, x)
                    loss = functional_loss(x, y, z, hp.shrink_lambda)
                    if hp.fedprox_mu != 0.0:
                        prox = 0.0
                        for p_, a_ in zip(params, anchor):
                            prox = prox + torch.sum(torch.square(p_ - a_))
                        loss = loss + hp.fedprox_mu * prox
                    grads = torch.autograd.grad(loss, params)
                    step += 1
                    with torch.no_grad():
                        for p_, g_, m_, v_ in zip(params, grads, m, v):
                            _adam_update(p_, g_, m_, v_, step, hp)
                    epoch_loss += float(loss.item())
                    nb += 1
                epoch_loss /= max(nb, 1)
                with torch.no_grad():
                    vl = 0.0
                    nvb = 0
                    prox_v = 0.0
                    if hp.fedprox_mu != 0.0:
                        pv = 0.0
                        for p_, a_ in zip(params, anchor):
                            pv = pv + torch.sum(torch.square(p_ - a_))
                        prox_v = hp.fedprox_mu * pv
                    for s in range(0, xv.shape[0], B):
                        x = xv[s:s + B]
                        z, y = functional_forward(params, x)
                        loss = functional_loss(x, y, z, hp.shrink_lambda)
                        if hp.fedprox_mu != 0.0:
                            loss = loss + prox_v
                        vl += float(loss.item())
                        nvb += 1
                    vl = vl / nvb if nvb else float("nan")
                track.append((epoch_loss, vl))
                epochs_run[i] = ep + 1
                if vl < min_valid:
                    min_valid = vl
                    best_epoch[i] = ep
                    with torch.no_grad():
                        st.best[c].copy_(canonical_to_padded(torch.cat([p_.detach().reshape(-1) for p_ in params]), self.dims))
                    worse = 0
                else:
                    worse += 1
                    if worse >= hp.patience:
                        break
            with torch.no_grad():
                st.params[c].copy_(canonical_to_padded(torch.cat([p_.detach().reshape(-1) for p_ in params]), self.dims))
                st.adam_m[c].copy_(canonical_to_padded(torch.cat([t.reshape(-1) for t in m]), self.dims))
                st.adam_v[c].copy_(canonical_to_padded(torch.cat([t.reshape(-1) for t in v]), self.dims))
                st.adam_step[c] = step
            tracking.append(track)
        return TrainResult(list(local_ids), epochs_run, tracking, best_epoch)

    # -- inference primitives ----------------------------------------------------
    def forward_rows(self, params, items, want_sse=True, want_latent=False):
        D = self.dims.d_in
        sse_out, lat_out = [], []
        cache = {}
        with torch.no_grad():
            for row, data in items:
                if row not in cache:
                    cache[row] = unflatten(padded_to_canonical(params[row], self.dims), self.dims)
                x = data[:, :D]
                z, y = functional_forward(cache[row], x)
                if want_sse:
                    sse_out.append(((y - x) ** 2).sum(dim=1))
                if want_latent:
                    lat_out.append(z)
        return sse_out, lat_out

    def weighted_sum(self, stack, weights):
        w = torch.tensor(list(weights), dtype=torch.float32, device=stack.device)
        # sequential accumulation in the given order (deterministic on every rank)
        out = torch.zeros(stack.shape[1], dtype=torch.float32, device=stack.device)
        for k in range(stack.shape[0]):
            out = out + stack[k] * w[k]
        return out

    def robust_aggregate(self, stack, t):
        k, P = stack.shape
        t = int(t)
        if k < 1 or t < 0 or 2 * t >= k:
            raise ValueError(f"robust_aggregate: trim count {t} leaves no model of {k}")
        st = stack.contiguous().to(torch.float32)
        # 32-bit keys (held in int64) whose order is -inf < ... < -0 < +0 < ... < +inf < NaN
        b = st.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        key = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
        key = key.masked_fill((b & 0x7FFFFFFF) > 0x7F800000, 0xFFFFFFFF)
        # rank = position in the stable argsort (ties by row)
        order = torch.argsort(key, dim=0, stable=True)
        rank = torch.empty_like(order)
        rank.scatter_(0, order, torch.arange(k, device=st.device).unsqueeze(1).expand(k, P))
        kept = (rank >= t) & (rank < k - t)
        # the kept values in row order, one fp32 rounding per add, from the first kept value
        acc = torch.zeros(P, dtype=torch.float32, device=st.device)
        started = torch.zeros(P, dtype=torch.bool, device=st.device)
        for j in range(k):
            acc = torch.where(kept[j], torch.where(started, acc + st[j], st[j]), acc)
            started = started | kept[j]
        return acc / torch.tensor(float(k - 2 * t), dtype=torch.float32, device=st.device)

    def krum_aggregate(self, stack, f, m):
        k, P = stack.shape
        f, m = int(f), int(m)
        if k < 1 or f < 0 or not 1 <= m <= k:
            raise ValueError(f"krum_aggregate: f = {f}, m = {m} of {k} models")
        q = max(k - f - 2, 0)
        st = stack.contiguous().to(torch.float32)
        dev = st.device
        # distances: lane l of 256 adds its coordinates l, l + 256, ... in that
        # order in f64 (the rows zero-extended), then eight folds
        C = -(-P // 256)
        pad = torch.zeros(k, C * 256, dtype=torch.float32, device=dev)
        pad[:, :P] = st
        p = torch.zeros(k, k, 256, dtype=torch.float64, device=dev)
        for c in range(C):
            x = pad[:, c * 256:(c + 1) * 256]
            e = (x.unsqueeze(1) - x.unsqueeze(0)).to(torch.float64)   # one fp32 rounding, then exact in f64
            p = p + e * e
        h = 128
        while h >= 1:
            p = p[..., :h] + p[..., h:2 * h]
            h //= 2
        D = p[..., 0]
        D = torch.where(torch.isnan(D), torch.full_like(D, float("inf")), D)
        # scores: the q smallest of each row's k - 1 distances (non-negative
        # doubles order as integers; ties by column), added in column order
        key = D.contiguous().view(torch.int64).clone()
        key.fill_diagonal_(torch.iinfo(torch.int64).max)
        ar = torch.arange(k, device=dev)
        order = torch.argsort(key, dim=1, stable=True)
        rank = torch.empty_like(order)
        rank.scatter_(1, order, ar.unsqueeze(0).expand(k, k).contiguous())
        near = rank < q
        score = torch.zeros(k, dtype=torch.float64, device=dev)
        for j in range(k):
            score = torch.where(near[:, j], score + D[:, j], score)
        # selection: the m lowest scores, ties by position
        sorder = torch.argsort(score.view(torch.int64), stable=True)
        kept = sorted(int(i) for i in sorder[:m].tolist())
        # the kept rows in selection order, one fp32 rounding per add
        acc = st[kept[0]].clone()
        for j in kept[1:]:
            acc = acc + st[j]
        return acc / torch.tensor(float(m), dtype=torch.float32, device=dev), kept

    def geomed_aggregate(self, stack, iters, nu):
        from ..protocol.aggregation import geomed_check

        iters, nu = geomed_check(iters, nu)
        k, P = stack.shape
        if k < 1 or P < 1:
            raise ValueError(f"geomed_aggregate: a stack of {k} models of {P} values")
        f64 = torch.float64
        st = stack.detach().contiguous().to(device="cpu", dtype=torch.float32)
        nb = -(-P // 256)
        pad = torch.zeros(k, nb * 256, dtype=torch.float32)
        pad[:, :P] = st
        st64 = st.to(f64)
        inf = float("inf")

        def fold(p):   # eight folds p_l += p_{l+h}, h = 128 .. 1, over the last axis
            h = 128
            while h >= 1:
                p = p[..., :h] + p[..., h:2 * h]
                h //= 2
            return p[..., 0]

        def dist(z):   # step 1: the block sum of the squared fp32 differences
            e = (pad if z is None else pad - z).to(f64)   # one fp32 rounding, then exact in f64
            s = e * e
            s[:, P:] = 0.0                                # the zero extension
            q = fold(s.view(k, nb, 256))
            d = torch.zeros(k, dtype=f64)
            for b in range(nb):
                d = d + q[:, b]
            return torch.where(torch.isnan(d) | (d == inf), torch.full_like(d, inf), d)

        def lane_sum(x):
            C = -(-k // 256)
            xp = torch.zeros(C * 256, dtype=f64)
            xp[:k] = x
            p = torch.zeros(256, dtype=f64)
            for c in range(C):
                p = p + xp[c * 256:(c + 1) * 256]
            return float(fold(p))

        d = dist(None)
        beta = torch.where(d < inf, torch.ones_like(d), torch.zeros_like(d))
        for t in range(iters + 1):
            B = lane_sum(beta)
            if B == 0.0:   # every row bad: the rule ends
                z = torch.full((P,), 0x7FC00000, dtype=torch.int32).view(torch.float32)
                w = torch.zeros(k, dtype=f64)
                break
            w = beta / torch.full_like(beta, B)   # (a tensor divisor: an IEEE division per element)
            acc = torch.zeros(P, dtype=f64)
            for i in range(k):
                if float(beta[i]) != 0.0:
                    acc = acc + w[i] * st64[i]
            z = acc.to(torch.float32)
            if t == iters:
                break
            zp = torch.zeros(nb * 256, dtype=torch.float32)
            zp[:P] = z
            d = dist(zp)
            with np.errstate(all="ignore"):
                r = torch.from_numpy(np.sqrt(d.numpy()))   # (torch.sqrt's vectorised f64 path is not correctly rounded)
            beta = torch.where(d < inf, torch.ones_like(r) / torch.maximum(r, torch.full_like(r, nu)),
                               torch.zeros_like(d))
        return z.to(stack.device), [float(x) for x in w.tolist()]

    def param_drift(self, hist, new):
        a = padded_to_canonical(hist, self.dims)
        b = padded_to_canonical(new.unsqueeze(0), self.dims)
        from ..models.layout import padded_index
        _, segs = padded_index(self.dims)
        diff = a - b
        tot = torch.zeros(a.shape[0], dtype=torch.float32, device=a.device)
        for s, e in segs:
            tot = tot + torch.linalg.vector_norm(diff[:, s:e], dim=1)
        return tot

    def cen_scores(self, train_lat, test_lat):
        out = []
        for tr, te in zip(train_lat, test_lat):
            trn = tr.detach().cpu().numpy().astype(np.float32)
            ten = te.detach().cpu().numpy().astype(np.float32)
            out.append(torch.from_numpy(cen_score_numpy(trn, ten)))
        return out

    def knn_scores(self, train_lat, query_lat, k):
        out = []
        for tr, qu in zip(train_lat, query_lat):
            trn = tr.detach().cpu().numpy().astype(np.float32)
            qun = qu.detach().cpu().numpy().astype(np.float32)
            out.append(torch.from_numpy(knn_score_numpy(trn, qun, k)))
        return out

    def auc(self, scores, labels):
        res = []
        for s, l in zip(scores, labels):
            sn = np.nan_to_num(s.detach().cpu().numpy().astype(np.float64))
            ln = l.detach().cpu().numpy() if torch.is_tensor(l) else np.asarray(l)
            res.append(_host.roc_auc(sn, ln))
        return np.asarray(res, dtype=np.float64)

    def detect_metrics(self, calib, scores, labels, ranks, calib_labels=None, score_scale=1.0, value="f1"):
        from ..eval.metrics import detect_value_is_recall

        want_recall = detect_value_is_recall(value)
        scale = torch.tensor(float(score_scale), dtype=torch.float32)

        def cleaned(t):
            t = t.detach().cpu()
            if t.dtype != torch.float64:
                t = (t.to(torch.float32) * scale).to(torch.float64)   # one fp32 rounding, then exact
            return torch.nan_to_num(t)   # f64: nan -> 0, +-inf -> +-DBL_MAX

        nan = float("nan")
        out = np.zeros((8, len(scores)), dtype=np.float64)
        for i, (c, s, l, j) in enumerate(zip(calib, scores, labels, ranks)):
            c = cleaned(c)
            if calib_labels is not None:
                c = c[calib_labels[i].detach().cpu() == 0]
            j = int(j)
            tau = nan
            if 0 <= j < c.numel():
                tau = float(torch.sort(c).values[j])
                if tau == 0.0:
                    tau = 0.0   # a selected -0.0 is reported as +0.0
            y = l.detach().cpu() != 0
            flag = cleaned(s) > tau
            tp = int(torch.count_nonzero(flag & y))
            fp = int(torch.count_nonzero(flag & ~y))
            pos = int(torch.count_nonzero(y))
            fn, tn = pos - tp, int(y.numel()) - pos - fp
            if tau != tau or pos == 0 or pos == int(y.numel()):
                precision = recall = f1 = nan
            else:
                precision = tp / (tp + fp) if (tp + fp) else 0.0
                recall = tp / (tp + fn) if (tp + fn) else 0.0
                f1 = 2 * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) else 0.0
            out[:, i] = (recall if want_recall else f1, tau, tp, fp, fn, tn, precision, recall)
        return out

    def score_rows(self, detectors, rows, want_latents=False):
        from ..deploy.detector import score_rows_numpy

        if len(detectors) != len(rows):
            raise ValueError("score_rows: one block of rows per detector")
        out = []
        for det, x in zip(detectors, rows):
            x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
            eng = self if det.dims == self.dims else TorchEngine(det.dims, self.device)
            out.append(score_rows_numpy(det, x, engine=eng, want_latents=want_latents))
        return out

    def explain_rows(self, detectors, rows, top_k=5, which=None, dense=False):
        from ..deploy.detector import check_top_k, explain_rows_numpy

        check_top_k(top_k)
        which = list(which) if which is not None else [None] * len(detectors)
        if len(detectors) != len(rows) or len(which) != len(detectors):
            raise ValueError("explain_rows: one block of rows (and one which) per detector")
        out = []
        for det, x, w in zip(detectors, rows, which):
            x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
            eng = self if det.dims == self.dims else TorchEngine(det.dims, self.device)
            out.append(explain_rows_numpy(det, x, top_k, which=w, dense=dense, engine=eng))
        return out

    def monitor_rows(self, detectors, rows, block_rows=None):
        from ..deploy.detector import check_block_rows, monitor_rows_numpy
        from ..ops._hip import score_rows_per_block

        if len(detectors) != len(rows):
            raise ValueError("monitor_rows: one block of rows per detector")
        xs = [x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in rows]
        for det, x in zip(detectors, xs):
            if x.ndim != 2 or x.shape[1] != det.dims.d_in:
                raise ValueError(f"rows must be [n, {det.dims.d_in}], got {x.shape}")
        rpb = check_block_rows(block_rows if block_rows is not None
                               else score_rows_per_block(sum(int(x.shape[0]) for x in xs)))
        out = []
        for det, x in zip(detectors, xs):
            eng = self if det.dims == self.dims else TorchEngine(det.dims, self.device)
            out.append(monitor_rows_numpy(det, x, rpb, engine=eng))
        return out

    def incidents(self, flags, scores, window, min_alarms, hold=0):
        from ..deploy.detector import check_incident_params, incidents_numpy

        check_incident_params(window, min_alarms, hold)
        if len(flags) != len(scores):
            raise ValueError("incidents: one scores vector per flags vector")

        def host(v):
            return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)

        return [incidents_numpy(host(f), host(s), window, min_alarms, hold) for f, s in zip(flags, scores)]

    def incident_signatures(self, detectors, rows, flags, incidents, top_k=5, which=None, block_rows=None):
        from ..deploy.detector import (check_block_rows, check_top_k, incident_signatures_numpy, signature_list)
        from ..ops._hip import score_rows_per_block

        check_top_k(top_k)
        which = list(which) if which is not None else [None] * len(detectors)
        if not (len(rows) == len(flags) == len(incidents) == len(which) == len(detectors)):
            raise ValueError("incident_signatures: one rows / flags / incidents (and which) entry per detector")

        def host(v):
            return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)

        xs, fs = [host(x) for x in rows], [host(f) for f in flags]
        if block_rows is None:
            block_rows = score_rows_per_block(sum(int(signature_list(f, inc, w)[0].shape[0])
                                                  for f, inc, w in zip(fs, incidents, which)))
        rpb = check_block_rows(block_rows)
        out = []
        for det, x, f, inc, w in zip(detectors, xs, fs, incidents, which):
            eng = self if det.dims == self.dims else TorchEngine(det.dims, self.device)
            out.append(incident_signatures_numpy(det, x, f, inc, top_k, which=w, block_rows=rpb, engine=eng))
        return out

    def standardize_ddof1(self, x):
        D = self.dims.d_in
        xr = x[:, :D]
        mean = xr.mean(dim=0, keepdim=True)
        std = xr.std(dim=0, keepdim=True) + 1e-8
        out = torch.zeros_like(x)
        out[:, :D] = (xr - mean) / std
        return out


def cen_score_numpy(train_lat: np.ndarray, test_lat: np.ndarray) -> np.ndarray:
    """SAE-CEN anomaly score (reference ``CentroidBasedOneClassClassifier``,
    `src/Model/Centroid.py:15-35`): StandardScaler fit on the train latents
    (float64 accumulation, float32 in-place transform, as sklearn does on a
    float32 array), Euclidean distance to the origin in float64 (cdist)."""
    from ..data.scaler import StandardScaler

    sc = StandardScaler().fit(train_lat)
    t = test_lat.astype(np.float32).copy()
    t -= sc.mean_          # numpy in-place: computed in float64, stored as float32
    t /= sc.scale_
    t64 = t.astype(np.float64)
    return np.sqrt(np.sum(t64 * t64, axis=1))


KNN_MAX_K = 16


def knn_score_numpy(train_lat: np.ndarray, query_lat: np.ndarray, k: int, scaler=None) -> np.ndarray:
    """Nearest-neighbour latent score (README "Latent scorers"; the oracle of
    ``knn_score_kernel``): the StandardScaler of ``cen_score_numpy`` fitted on
    the train latents, the same in-place float32 transform applied to the
    train and the query rows, squared distances summed in float64 over the
    columns in order from 0 (NaN counts as +inf), and the square root of the
    ``min(k, n_train)``-th smallest per query row.  ``scaler``: a fitted
    scaler to use instead (tests nudge its mean and scale)."""
    from ..data.scaler import StandardScaler

    train_lat = np.asarray(train_lat, dtype=np.float32)
    query_lat = np.asarray(query_lat, dtype=np.float32)
    if not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError(f"knn: k must lie in 1..{KNN_MAX_K}, got {k!r}")
    n, z = train_lat.shape
    if n == 0:
        raise ValueError("knn: a train set has no rows")
    sc = StandardScaler().fit(train_lat) if scaler is None else scaler

    def scaled(a):
        t = a.astype(np.float32).copy()
        t -= sc.mean_          # numpy in-place: computed in float64, stored as float32
        t /= sc.scale_
        return t.astype(np.float64)

    x, q = scaled(train_lat), scaled(query_lat)
    kth = min(int(k), n) - 1
    out = np.empty(q.shape[0], dtype=np.float64)
    chunk = max(1, (1 << 22) // n)   # <= 32 MiB of float64 distances at a time
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, q.shape[0], chunk):
            qc = q[s:s + chunk]
            d2 = np.zeros((qc.shape[0], n), dtype=np.float64)
            for c in range(z):
                df = qc[:, c:c + 1] - x[None, :, c]
                d2 += df * df
            d2[np.isnan(d2)] = np.inf
            out[s:s + chunk] = np.sqrt(np.partition(d2, kth, axis=1)[:, kth])
    return out
