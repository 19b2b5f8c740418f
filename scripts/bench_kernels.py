"""Per-kernel timing on one GPU (torch CUDA events, median over repeats).

Workload = the flagship round's shapes: 10 N-BaIoT-sized clients, 5 trained
per round for E epochs at batch 12; evaluation of all 10 clients.
Prints one JSON object with microseconds per launch and derived per-step
costs of the fused training kernel.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])

from fedmse_decentralized_amd.data.prepare import prepare_federation  # noqa: E402
from fedmse_decentralized_amd.data.synthetic import SyntheticSpec, generate_federation  # noqa: E402
from fedmse_decentralized_amd.engine.base import TrainHParams  # noqa: E402
from fedmse_decentralized_amd.engine.hip_engine import HipEngine  # noqa: E402
from fedmse_decentralized_amd.eval.evaluator import evaluate_clients  # noqa: E402
from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS  # noqa: E402
from fedmse_decentralized_amd.models.reference import init_client_params  # noqa: E402
from fedmse_decentralized_amd.ops import _hip  # noqa: E402


def timeit(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def aggregation_timings(eng, args) -> dict:
    """``--aggregation``: the distance-based rules' launches over k models of
    the benchmark's clients (rows repeated past 10), event-timed over
    preallocated workspaces: ``krum`` / ``multi_krum`` (three launches) and
    ``geomed`` at T = 0, 3 and 8 (T + 2 launches) beside the plain weighted sum
    over the same rows."""
    from fedmse_decentralized_amd.protocol.aggregation import krum_counts

    dev = eng.device
    out = {}
    agg_out = torch.empty(eng.store.params.shape[1], dtype=torch.float32, device=dev)
    for kk in (5, 40, 256):
        st = eng.store.params[torch.arange(kk, device=dev) % args.clients].contiguous()
        # (distinct rows: identical ones would sit at distance 0 of their median)
        st = st * (1.0 + 0.01 * torch.arange(kk, device=dev, dtype=torch.float32).unsqueeze(1))
        out[f"weighted_sum_k{kk}_us"] = timeit(lambda: _hip.weighted_sum(st, [1.0 / kk] * kk, out=agg_out),
                                               reps=args.reps)[0]
        ws = torch.empty(_hip.krum_workspace_size(kk), dtype=torch.float64, device=dev)
        for ut in ("krum", "multi_krum"):
            kf, _, km = krum_counts(ut, kk, 0.2)
            out[f"{ut}_k{kk}_us"] = timeit(lambda: _hip.krum_aggregate_stack(st, kf, km, out=agg_out, workspace=ws),
                                           reps=args.reps)[0]
        gws = torch.empty(_hip.geomed_workspace_size(kk, st.shape[1]), dtype=torch.float64, device=dev)
        for T in (0, 3, 8):
            key = f"geomed_k{kk}_us" if T == 3 else f"geomed_T{T}_k{kk}_us"
            out[key] = timeit(lambda: _hip.geomed_aggregate_stack(st, T, 1e-6, out=agg_out, workspace=gws),
                              reps=args.reps)[0]
    return out


def detect_timings(eng, clients, args) -> dict:
    """``--detect``: detect_kernel (fedmx_detect.hip) beside auc_kernel on the
    same scores (the benchmark's 10 clients: CEN distances of each test set,
    calibrated on the ~170 validation rows), one large client where auc_kernel
    answers -1 (host fallback), and ms / round of the device-resident round
    under ``--metric detection`` against ``--metric classification``."""
    from fedmse_decentralized_amd.eval.metrics import calibration_rank

    dev = eng.device
    out = {}
    allc = list(range(args.clients))
    items = []
    for c in allc:
        items += [(c, eng.store.rows(s, c)) for s in ("train", "test", "valid")]
    _, lat = eng.forward_rows(eng.store.params, items, False, True)
    sc = eng.cen_scores(lat[0::3], lat[1::3])
    vc = eng.cen_scores(lat[0::3], lat[2::3])
    labs = [eng.store.label_view(c) for c in allc]
    ranks = [calibration_rank(int(v.shape[0]), 0.95) for v in vc]
    out["detect_valid_rows"] = [int(v.shape[0]) for v in vc]
    out["detect_us"] = timeit(lambda: _hip.detect(vc, sc, labs, ranks), reps=args.reps)[0]
    out["auc_us"] = timeit(lambda: _hip.auc(sc, labs), reps=args.reps)[0]
    n0 = [int((lb == 0).sum()) for lb in labs]
    out["detect_tpr_at_fpr_us"] = timeit(lambda: _hip.detect(sc, sc, labs, [calibration_rank(n, 0.99) for n in n0],
                                                             calib_labels=labs, value_is_recall=True),
                                         reps=args.reps)[0]
    g = torch.Generator(device="cpu").manual_seed(5)
    big_c = [torch.rand(10_000, dtype=torch.float64, generator=g).to(dev)]
    big_s = [torch.rand(100_000, dtype=torch.float64, generator=g).to(dev)]
    big_y = [(torch.rand(100_000, generator=g) < 0.5).to(torch.int32).to(dev)]
    out["detect_large_us"] = timeit(lambda: _hip.detect(big_c, big_s, big_y, [9499]), reps=args.reps)[0]
    view = _hip.auc(big_s, big_y)
    out["auc_large_us"] = timeit(lambda: _hip.auc(big_s, big_y), reps=args.reps)[0]
    _hip.runtime(dev).sync()
    out["auc_large_result"] = float(view[0])   # -1: the class is too large for the LDS sort
    if args.detect_rounds > 0:
        import tempfile

        from fedmse_decentralized_amd.config import ExperimentConfig
        from fedmse_decentralized_amd.federation import Federation

        for metric in ("detection", "classification", "AUC"):
            cfg = ExperimentConfig(num_participants=0.5, epoch=args.epochs, num_rounds=10 ** 9,
                                   network_size=args.clients, synthetic="nbaiot", compat="fixed", backend="hip",
                                   global_early_stop=False, save_checkpoints=False, log_level="WARNING",
                                   output_root=tempfile.mkdtemp(), metric=metric)
            fed = Federation(cfg, "hybrid", "mse_avg", 0, write_reports=False).setup()
            assert fed._fast is not None
            for _ in range(20):
                fed.run_round()
            fed.finish()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.detect_rounds):
                fed.run_round()
            fed.finish()
            torch.cuda.synchronize()
            out[f"round_ms_{metric}"] = (time.perf_counter() - t0) / args.detect_rounds * 1e3
    return out


def scorer_timings(eng, clients, args) -> dict:
    """``--latent-scorer``: knn_score_kernel (fedmx_knn.hip) beside
    cen_score_kernel in one process.  The benchmark's 10 clients (each test set
    against its train latents, then test + validation sets as ``--metric
    detection`` launches them) at k = 1, 5 and 16; one large client (50,000
    train x 100,000 query rows, k = 5); the whole evaluation chain (forward +
    scorer + AUC) of the cached plan for both scorers; and ms / round of the
    device-resident round under either scorer."""
    dev = eng.device
    out = {}
    allc = list(range(args.clients))
    items = []
    for c in allc:
        items += [(c, eng.store.rows(s, c)) for s in ("train", "test", "valid")]
    _, lat = eng.forward_rows(eng.store.params, items, False, True)
    tr, te, va = lat[0::3], lat[1::3], lat[2::3]
    out["train_rows"] = [int(t.shape[0]) for t in tr]
    out["test_rows"] = [int(t.shape[0]) for t in te]
    out["valid_rows"] = [int(t.shape[0]) for t in va]
    Z = eng.dims.latent

    def launcher(scorer, trs, qus, k=5):
        """A cached-descriptor launch, as an evaluation plan issues it."""
        res = torch.empty(sum(int(q.shape[0]) for q in qus), dtype=torch.float64, device=dev)
        eng.latent_scorer, eng.knn_k = scorer, k
        blob, launch, _ = eng._scorer_plan(list(trs), list(qus), res)
        return lambda keep=(blob, res): launch()

    reps = max(args.reps, 50)
    out["cen_test_us"] = timeit(launcher("cen", tr, te), reps=reps)[0]
    out["cen_test_valid_us"] = timeit(launcher("cen", list(tr) * 2, list(te) + list(va)), reps=reps)[0]
    for k in (1, 5, 16):
        out[f"knn_k{k}_test_us"] = timeit(launcher("knn", tr, te, k), reps=reps)[0]
        out[f"knn_k{k}_test_valid_us"] = timeit(launcher("knn", list(tr) * 2, list(te) + list(va), k), reps=reps)[0]
    g = torch.Generator(device="cpu").manual_seed(6)
    big_tr = [torch.randn(50_000, Z, generator=g).to(dev)]
    big_q = [(1.5 * torch.randn(100_000, Z, generator=g)).to(dev)]
    out["cen_large_us"] = timeit(launcher("cen", big_tr, big_q), reps=args.reps)[0]
    out["knn_k5_large_us"] = timeit(launcher("knn", big_tr, big_q, 5), reps=max(args.reps // 4, 5), warm=1)[0]
    out["knn_large_grid_y"] = _hip.knn_grid_y(big_q)
    # pairs x padded columns x (subtract + FMA): the float64 VALU work of the scan
    cols = 4 * ((Z + 3) // 4)
    out["knn_k5_large_f64_gops"] = 50_000 * 100_000 * cols * 2 / out["knn_k5_large_us"] / 1e3
    # the evaluation chain of the cached plan: forward + scorer + AUC / detect
    for metric in ("AUC", "detection"):
        for scorer, k in (("cen", 5), ("knn", 1), ("knn", 5), ("knn", 16)):
            eng.latent_scorer, eng.knn_k = scorer, k
            name = f"eval_chain_{metric}_{scorer}" + (f"_k{k}" if scorer == "knn" else "") + "_us"
            out[name] = timeit(lambda: eng.evaluate_launch("hybrid", metric=metric), reps=reps)[0]
    eng.latent_scorer, eng.knn_k = "cen", 5
    if args.scorer_rounds > 0:
        import tempfile

        from fedmse_decentralized_amd.config import ExperimentConfig
        from fedmse_decentralized_amd.federation import Federation

        feds = {}
        for scorer in ("cen", "knn"):
            cfg = ExperimentConfig(num_participants=0.5, epoch=args.epochs, num_rounds=10 ** 9,
                                   network_size=args.clients, synthetic="nbaiot", compat="fixed", backend="hip",
                                   global_early_stop=False, save_checkpoints=False, log_level="WARNING",
                                   output_root=tempfile.mkdtemp(), latent_scorer=scorer, knn_k=5)
            fed = Federation(cfg, "hybrid", "mse_avg", 0, write_reports=False).setup()
            assert fed._fast is not None
            for _ in range(20):
                fed.run_round()
            fed.finish()
            feds[scorer] = fed
        # alternating blocks of rounds, so both scorers see the same machine state
        tot = {"cen": 0.0, "knn": 0.0}
        blocks, per = 4, max(args.scorer_rounds // 4, 1)
        for _ in range(blocks):
            for scorer, fed in feds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per):
                    fed.run_round()
                fed.finish()
                torch.cuda.synchronize()
                tot[scorer] += time.perf_counter() - t0
        for scorer in feds:
            out[f"round_ms_{scorer}"] = tot[scorer] / (blocks * per) * 1e3
    return out


def score_rows_timings(args) -> dict:
    """``--score-rows``: score_rows_kernel (fedmx_score.hip) over ``--score-n``
    synthetic N-BaIoT-shaped raw float64 rows for one detector, AE and CEN,
    beside the same result composed from the ops that existed before it: host
    ``transform`` + ``pad_features`` + host-to-device copy + ``forward_rows``
    (+ ``cen_scores``, which refits the latent scaler per launch).  The fused
    launch is event-timed with the raw rows already on the device; both paths
    are also wall-clocked from host rows to host scores (alternating, so they
    see the same machine state).  Phase split of the fused kernel: the same
    launch with nothing but standardise + forward (latents only), and the
    forward alone on prepared fp32 rows."""
    from fedmse_decentralized_amd.data.scaler import StandardScaler
    from fedmse_decentralized_amd.deploy.detector import Detector
    from fedmse_decentralized_amd.engine.base import pad_features

    dev = torch.device("cuda", 0)
    dims = DEFAULT_DIMS
    n = args.score_n
    raws = generate_federation(SyntheticSpec(kind="nbaiot", n_clients=1, seed=1))
    clients, _ = prepare_federation(raws, 1234)
    sc = dict(clients[0].meta["scaler"])
    kind = sc.pop("kind")
    pool = np.concatenate([raws[0].normal, raws[0].abnormal, raws[0].test_normal], 0)
    rows = pool[np.random.default_rng(3).integers(0, pool.shape[0], size=n)].copy()
    init, _ = init_client_params(1, 0)
    eng = HipEngine(dims, dev)
    ae = Detector(dims=dims, model_type="autoencoder", params=init[0].numpy(), scaler_kind=kind, scaler=sc,
                  threshold=0.5)
    params = ae.padded_params().unsqueeze(0).to(dev)
    train = torch.from_numpy(pad_features(clients[0].train)).to(dev)
    _, tl = eng.forward_rows(params, [(0, train)], False, True)
    zs = StandardScaler().fit(eng.fetch([tl[0]])[0])
    cen = Detector(dims=dims, model_type="hybrid", params=ae.params, scaler_kind=kind, scaler=sc, threshold=1.0,
                   latent_scorer="cen", latent_mean=zs.mean_, latent_scale=zs.scale_)
    rows_dev = torch.from_numpy(rows).to(dev)
    rpb = _hip.score_rows_per_block(n)
    out = {"score_rows_n": n, "score_rows_per_block": rpb, "score_rows_workgroups": -(-n // rpb),
           "score_rows_threads": 256, "score_rows_input": "float64"}
    proc = ae.processor()
    reps = max(args.reps // 2, 5)

    def composed(det):
        x = torch.from_numpy(pad_features(proc.transform(rows)[0])).to(dev)
        if det.model_type == "autoencoder":
            sse, _ = eng.forward_rows(params, [(0, x)], True, False)
            return eng.fetch([sse[0]])[0]
        _, lat = eng.forward_rows(params, [(0, train), (0, x)], False, True)
        return eng.fetch([eng.cen_scores([lat[0]], [lat[1]])[0]])[0]

    for name, det in (("ae", ae), ("cen", cen)):
        state, _ = eng._score_state(det)
        us = timeit(lambda: _hip.score_rows([state], [rows_dev]), reps=args.reps)[0]
        out[f"score_rows_{name}_us"] = us
        out[f"score_rows_{name}_rows_per_s"] = n / us * 1e6
        wall = {"fused": [], "composed": []}
        for i in range(reps + 1):
            for path, fn in (("fused", lambda: eng.score_rows([det], [rows])), ("composed", lambda: composed(det))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i:   # (the first pass warms both paths up)
                    wall[path].append(time.perf_counter() - t0)
        for path, ts in wall.items():
            out[f"{path}_{name}_host_to_host_ms"] = float(np.median(ts)) * 1e3
            out[f"{path}_{name}_host_to_host_rows_per_s"] = n / float(np.median(ts))
    # the composed chain's device part alone (rows already standardised, padded and copied)
    x = torch.from_numpy(pad_features(proc.transform(rows)[0])).to(dev)
    t0 = time.perf_counter()
    for _ in range(3):
        pad_features(proc.transform(rows)[0])
    out["composed_host_transform_pad_ms"] = (time.perf_counter() - t0) / 3 * 1e3
    out["composed_fwd_sse_us"] = timeit(lambda: eng.forward_rows(params, [(0, x)], True, False), reps=args.reps)[0]
    out["composed_fwd_lat_us"] = timeit(lambda: eng.forward_rows(params, [(0, x)], False, True), reps=args.reps)[0]
    _, lat = eng.forward_rows(params, [(0, train), (0, x)], False, True)
    out["composed_cen_us"] = timeit(lambda: eng.cen_scores([lat[0]], [lat[1]]), reps=args.reps)[0]
    # phase split of the fused kernel: standardise + forward to latents, no score
    lat_only = _hip.ScoreState(params[0].contiguous(), dims, sc["mean_"], sc["scale_"], kind == "minmax", 0, 0.0)
    out["score_rows_latents_only_us"] = timeit(lambda: _hip.score_rows([lat_only], [rows_dev]), reps=args.reps)[0]
    return out


def explain_rows_timings(args) -> dict:
    """``--explain-rows``: explain_rows_kernel (fedmx_explain.hip) over the
    ``--score-n`` raw float64 rows of ``--score-rows`` (same generator, same
    detectors), event-timed with the rows on the device, beside
    score_rows_kernel on those rows in the same process: every row at K = 5,
    5 % of the rows through ``which`` (ascending and shuffled), dense mode, and
    K = 1 / 16 to split the selection from the rest."""
    from fedmse_decentralized_amd.data.scaler import StandardScaler
    from fedmse_decentralized_amd.deploy.detector import Detector
    from fedmse_decentralized_amd.engine.base import pad_features

    dev = torch.device("cuda", 0)
    dims = DEFAULT_DIMS
    n = args.score_n
    raws = generate_federation(SyntheticSpec(kind="nbaiot", n_clients=1, seed=1))
    clients, _ = prepare_federation(raws, 1234)
    sc = dict(clients[0].meta["scaler"])
    kind = sc.pop("kind")
    pool = np.concatenate([raws[0].normal, raws[0].abnormal, raws[0].test_normal], 0)
    rows = pool[np.random.default_rng(3).integers(0, pool.shape[0], size=n)].copy()
    init, _ = init_client_params(1, 0)
    eng = HipEngine(dims, dev)
    ae = Detector(dims=dims, model_type="autoencoder", params=init[0].numpy(), scaler_kind=kind, scaler=sc,
                  threshold=0.5)
    params = ae.padded_params().unsqueeze(0).to(dev)
    train = torch.from_numpy(pad_features(clients[0].train)).to(dev)
    _, tl = eng.forward_rows(params, [(0, train)], False, True)
    zs = StandardScaler().fit(eng.fetch([tl[0]])[0])
    cen = Detector(dims=dims, model_type="hybrid", params=ae.params, scaler_kind=kind, scaler=sc, threshold=1.0,
                   latent_scorer="cen", latent_mean=zs.mean_, latent_scale=zs.scale_)
    rows_dev = torch.from_numpy(rows).to(dev)
    m5 = max(n // 20, 1)
    rng = np.random.default_rng(4)
    sub_sorted = np.sort(rng.choice(n, size=m5, replace=False))
    sub_shuffled = rng.permutation(sub_sorted)
    out = {"explain_rows_n": n, "explain_rows_subset": m5, "explain_rows_per_block": _hip.score_rows_per_block(n),
           "explain_rows_subset_per_block": _hip.score_rows_per_block(m5), "explain_rows_input": "float64"}
    for name, det in (("ae", ae), ("cen", cen)):
        state, _ = eng._score_state(det)
        score_us = timeit(lambda: _hip.score_rows([state], [rows_dev]), reps=args.reps)[0]
        out[f"score_rows_{name}_us"] = score_us
        cases = {"all_k5": dict(top_k=5), "all_k1": dict(top_k=1), "all_k16": dict(top_k=16),
                 "all_k5_dense": dict(top_k=5, dense=True),
                 "subset_sorted_k5": dict(top_k=5, which=[sub_sorted]),
                 "subset_shuffled_k5": dict(top_k=5, which=[sub_shuffled])}
        for case, kw in cases.items():
            us = timeit(lambda: _hip.explain_rows([state], [rows_dev], **kw), reps=args.reps)[0]
            out[f"explain_rows_{name}_{case}_us"] = us
            out[f"explain_rows_{name}_{case}_vs_score_rows"] = us / score_us
    return out


def monitor_rows_timings(args) -> dict:
    """``--monitor-rows``: monitor_rows_kernel + monitor_fold_kernel
    (fedmx_monitor.hip) over the ``--score-n`` raw float64 rows of
    ``--score-rows`` (same generator, same detectors, each with a baseline of
    its own train rows and 10 score bins), event-timed with the rows on the
    device, beside score_rows_kernel on those rows in the same process; then
    host to host: ``HipEngine.monitor_rows`` on host rows (upload, both
    launches, read-back, report) beside host numpy computing the same report
    (``TorchEngine.monitor_rows``, the oracle, with the same block size; CEN).
    The two kernels are also timed apart.  ``--monitor-kernels-only`` stops
    after the event-timed figures (A/B of builds through ``FEDMX_HIP_LIB``)."""
    import time

    from fedmse_decentralized_amd.data.scaler import StandardScaler
    from fedmse_decentralized_amd.deploy.detector import Detector, make_baseline, score_rows_numpy
    from fedmse_decentralized_amd.engine.base import pad_features

    dev = torch.device("cuda", 0)
    dims = DEFAULT_DIMS
    n = args.score_n
    raws = generate_federation(SyntheticSpec(kind="nbaiot", n_clients=1, seed=1))
    clients, _ = prepare_federation(raws, 1234)
    sc = dict(clients[0].meta["scaler"])
    kind = sc.pop("kind")
    pool = np.concatenate([raws[0].normal, raws[0].abnormal, raws[0].test_normal], 0)
    rows = pool[np.random.default_rng(3).integers(0, pool.shape[0], size=n)].copy()
    init, _ = init_client_params(1, 0)
    eng = HipEngine(dims, dev)
    ae = Detector(dims=dims, model_type="autoencoder", params=init[0].numpy(), scaler_kind=kind, scaler=sc,
                  threshold=0.5, detect_quantile=0.95)
    params = ae.padded_params().unsqueeze(0).to(dev)
    train = torch.from_numpy(pad_features(clients[0].train)).to(dev)
    _, tl = eng.forward_rows(params, [(0, train)], False, True)
    zs = StandardScaler().fit(eng.fetch([tl[0]])[0])
    cen = Detector(dims=dims, model_type="hybrid", params=ae.params, scaler_kind=kind, scaler=sc, threshold=1.0,
                   detect_quantile=0.95, latent_scorer="cen", latent_mean=zs.mean_, latent_scale=zs.scale_)
    rows_dev = torch.from_numpy(rows).to(dev)
    rpb = _hip.score_rows_per_block(n)
    out = {"monitor_rows_n": n, "monitor_rows_per_block": rpb, "monitor_rows_workgroups": -(-n // rpb),
           "monitor_rows_input": "float64", "monitor_rows_bins": 10}
    for name, det in (("ae", ae), ("cen", cen)):
        valid_scores = np.sort(eng.score_rows([det], [raws[0].normal[:2000]])[0][0])
        det.baseline = make_baseline(clients[0].train[:, :dims.d_in], valid_scores, 10)
        det.validate()
        state, _ = eng._score_state(det)
        state.set_baseline(det.baseline.feat_lo, det.baseline.feat_hi, det.baseline.score_edges)
        score_us = timeit(lambda: _hip.score_rows([state], [rows_dev]), reps=args.reps)[0]
        us = timeit(lambda: _hip.monitor_rows([state], [rows_dev]), reps=args.reps)[0]
        out[f"score_rows_{name}_us"] = score_us
        out[f"monitor_rows_{name}_us"] = us
        out[f"monitor_rows_{name}_vs_score_rows"] = us / score_us
        # the two launches apart, on one descriptor set (no allocation, no zeroing in the timed span)
        total, alarms, hist, lats, _, part = _hip.monitor_rows([state], [rows_dev])
        desc, fold = _hip.monitor_desc([state], [rows_dev], lats, alarms, hist, part, total, rpb)
        rt = _hip.runtime(dev)
        dptr, fptr = rt.desc.put(desc, fold)
        L = _hip.lib()
        out[f"monitor_rows_kernel_{name}_us"] = timeit(
            lambda: _hip._check(L.fedmx_monitor_rows(dptr, len(desc), fptr, 0, rt.stream), "fedmx_monitor_rows"),
            reps=args.reps)[0]
        out[f"monitor_fold_kernel_{name}_us"] = timeit(
            lambda: _hip._check(L.fedmx_monitor_fold(fptr, len(fold), rt.stream), "fedmx_monitor_fold"),
            reps=args.reps)[0]
        out[f"monitor_rows_kernel_{name}_vs_score_rows"] = out[f"monitor_rows_kernel_{name}_us"] / score_us
        if args.monitor_kernels_only:
            continue
        eng.monitor_rows([det], [rows[:4096]])
        t0 = time.perf_counter()
        rep = eng.monitor_rows([det], [rows])[0]
        out[f"monitor_rows_{name}_host_to_host_ms"] = (time.perf_counter() - t0) * 1e3
        out[f"monitor_rows_{name}_alarm_rate"] = rep.alarm_rate
        out[f"monitor_rows_{name}_psi"] = rep.psi
        out[f"monitor_rows_{name}_max_out_share"] = float(rep.out_share.max())
    if args.monitor_kernels_only:
        return out
    # host numpy computing the same report: the oracle, on the same rows with the same block size
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine

    host = TorchEngine(dims, torch.device("cpu"))
    t0 = time.perf_counter()
    want = host.monitor_rows([cen], [rows], block_rows=rep.block_rows)[0]
    out["monitor_rows_cen_host_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    cen.standardise(rows)
    out["monitor_rows_host_transform_ms"] = (time.perf_counter() - t0) * 1e3
    out["monitor_rows_cen_sums_equal_host"] = bool(want.sum.tobytes() == rep.sum.tobytes()
                                                   and want.sq.tobytes() == rep.sq.tobytes()
                                                   and np.array_equal(want.cnt, rep.cnt)
                                                   and np.array_equal(want.out, rep.out))
    return out


def incidents_timings(args) -> dict:
    """``--incidents``: the incident launches (fedmx_incident.hip) over the
    ``--score-n`` raw float64 rows of ``--score-rows`` (same generator, the AE
    detector), at window 64, hold 64 and the ``auto`` minimum for a 0.05 flag
    rate, with the threshold at the score quantile that flags 5 % and 50 % of
    the rows.  Event-timed with flags and scores on the device: the whole call
    (two allocations, five launches) and the passes as cumulative prefixes of
    the launch sequence, beside score_rows_kernel on the same rows; wall clock
    from host rows to host results: ``HipEngine.score_incidents`` beside
    ``HipEngine.score_rows`` followed by ``incidents_numpy`` on the host."""
    from fedmse_decentralized_amd.deploy.detector import Detector, incident_min_alarms, incidents_numpy

    dev = torch.device("cuda", 0)
    dims = DEFAULT_DIMS
    n = args.score_n
    raws = generate_federation(SyntheticSpec(kind="nbaiot", n_clients=1, seed=1))
    clients, _ = prepare_federation(raws, 1234)
    sc = dict(clients[0].meta["scaler"])
    kind = sc.pop("kind")
    pool = np.concatenate([raws[0].normal, raws[0].abnormal, raws[0].test_normal], 0)
    rows = pool[np.random.default_rng(3).integers(0, pool.shape[0], size=n)].copy()
    init, _ = init_client_params(1, 0)
    eng = HipEngine(dims, dev)
    det = Detector(dims=dims, model_type="autoencoder", params=init[0].numpy(), scaler_kind=kind, scaler=sc,
                   threshold=0.5, detect_quantile=0.95)
    rows_dev = torch.from_numpy(rows).to(dev)
    w, h = 64, 64
    m = incident_min_alarms(w, 0.05, 1e-6)
    S = _hip.incident_span_rows()
    out = {"incidents_n": n, "incidents_window": w, "incidents_min_alarms": m, "incidents_hold": h,
           "incidents_span_rows": S, "incidents_workgroups": -(-n // S), "incidents_threads": 1024}
    scores0 = eng.score_rows([det], [rows])[0][0]
    state, _ = eng._score_state(det)
    out["score_rows_us"] = score_us = timeit(lambda: _hip.score_rows([state], [rows_dev]), reps=args.reps)[0]
    rt = _hip.runtime(dev)
    L = _hip.lib()
    reps = max(args.reps // 2, 5)
    for name, density in (("d05", 0.05), ("d50", 0.5)):
        det.threshold = float(np.quantile(scores0, 1.0 - density))
        state, _ = eng._score_state(det)
        (sc_dev, fl_dev, _), = _hip.score_rows([state], [rows_dev])[0]
        rt.sync()
        out[f"incidents_{name}_flag_share"] = float(fl_dev.sum().item()) / n
        us = timeit(lambda: _hip.incidents([fl_dev], [sc_dev], w, m, h), reps=args.reps)[0]
        out[f"incidents_{name}_call_us"] = us
        out[f"incidents_{name}_call_vs_score_rows"] = us / score_us
        # the passes: prefixes of the launch sequence over one descriptor set (the zeroing inside the timed span)
        o, = _hip.incidents([fl_dev], [sc_dev], w, m, h)
        items, spans = _hip.incident_desc([fl_dev], [sc_dev], w, m, h, [o])
        iptr, sptr = rt.desc.put(items, spans)
        kmax = int(items["kmax"].max())

        def run(phases):
            o["peak"].zero_()
            o["summary"].zero_()
            _hip._check(L.fedmx_incidents(iptr, 1, sptr, len(spans), kmax, phases, rt.stream), "fedmx_incidents")

        prev = 0.0
        for pname, mask in (("mark", 1), ("scan", 3), ("emit", 7), ("peak", 15), ("finish", 31)):
            t = timeit(lambda: run(mask), reps=args.reps)[0]
            out[f"incidents_{name}_{pname}_us"] = t - prev
            prev = t
        out[f"incidents_{name}_launches_us"] = prev
        out[f"incidents_{name}_launches_vs_score_rows"] = prev / score_us
        wall = {"device": [], "host": []}
        res = {}
        for i in range(reps + 1):
            for path, fn in (("device", lambda: eng.score_incidents([det], [rows], w, m, h)[0]),
                             ("host", lambda: (lambda r: r + (incidents_numpy(r[1], r[0], w, m, h),))(
                                 eng.score_rows([det], [rows])[0]))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[path] = fn()
                torch.cuda.synchronize()
                if i:
                    wall[path].append(time.perf_counter() - t0)
        a, b = res["device"][3], res["host"][3]
        out[f"incidents_{name}_count"] = a.count
        out[f"incidents_{name}_rows_covered"] = a.rows_covered
        out[f"incidents_{name}_equal_host"] = bool(all(
            getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("start", "end", "alarms", "peak_row", "peak_score"))
            and (a.hot_rows, a.count, a.rows_covered, a.longest) == (b.hot_rows, b.count, b.rows_covered, b.longest))
        out[f"score_incidents_{name}_host_to_host_ms"] = float(np.median(wall["device"])) * 1e3
        out[f"score_rows_plus_numpy_{name}_host_to_host_ms"] = float(np.median(wall["host"])) * 1e3
        t0 = time.perf_counter()
        incidents_numpy(res["host"][1], res["host"][0], w, m, h)
        out[f"incidents_numpy_{name}_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    eng.score_rows([det], [rows])
    torch.cuda.synchronize()
    out["score_rows_host_to_host_ms"] = (time.perf_counter() - t0) * 1e3
    return out


def signatures_timings(args) -> dict:
    """``--signatures``: incident signatures (fedmx_signature.hip) over the
    rows, detector and incident parameters of ``--incidents``, with the
    threshold at the score quantile that flags 5 % and 50 % of the rows (and,
    at 5 %, also with window 16, min 3, hold 0: many short incidents); the
    incidents summarised are all of them, or the 4096 with the most alarms.
    Event-timed with the list on the device: the two launches (the zeroing of
    the partial slots inside the timed span).  Wall clock from host flags and
    incidents to host results, with the raw rows on the host and already on the
    device: ``HipEngine.incident_signatures`` beside the only other way to the
    same numbers, ``HipEngine.explain_rows(dense=True, which=L)`` followed by
    ``signature_sums`` and ``signatures_report`` on the host; both must give
    equal bits."""
    from fedmse_decentralized_amd.deploy.detector import (SIGNATURE_MAX_INCIDENTS, Detector, incident_min_alarms,
                                                          signature_list, signature_sums, signatures_report)

    dev = torch.device("cuda", 0)
    dims = DEFAULT_DIMS
    n = args.score_n
    raws = generate_federation(SyntheticSpec(kind="nbaiot", n_clients=1, seed=1))
    clients, _ = prepare_federation(raws, 1234)
    sc = dict(clients[0].meta["scaler"])
    kind = sc.pop("kind")
    pool = np.concatenate([raws[0].normal, raws[0].abnormal, raws[0].test_normal], 0)
    rows = pool[np.random.default_rng(3).integers(0, pool.shape[0], size=n)].copy()
    init, _ = init_client_params(1, 0)
    eng = HipEngine(dims, dev)
    det = Detector(dims=dims, model_type="autoencoder", params=init[0].numpy(), scaler_kind=kind, scaler=sc,
                   threshold=0.5, detect_quantile=0.95)
    rows_dev = torch.from_numpy(rows).to(dev)
    w, h = 64, 64
    m = incident_min_alarms(w, 0.05, 1e-6)
    out = {"signatures_n": n, "signatures_window": w, "signatures_min_alarms": m, "signatures_hold": h}
    scores0 = eng.score_rows([det], [rows_dev])[0][0]
    rt = _hip.runtime(dev)
    reps = max(args.reps // 4, 3)
    # (at a flag share of 0.05 the auto minimum finds no incident in these rows: window 16, min 3, hold 0 beside it)
    for name, density, (cw, cm, ch) in (("d05", 0.05, (w, m, h)), ("d05_w16_m3_h0", 0.05, (16, 3, 0)),
                                        ("d50", 0.5, (w, m, h))):
        det.threshold = float(np.quantile(scores0, 1.0 - density))
        _, flags, _, inc = eng.score_incidents([det], [rows_dev], cw, cm, ch)[0]
        out[f"signatures_{name}_incidents_found"] = inc.count
        which = np.sort(np.argsort(-inc.alarms, kind="stable")[:SIGNATURE_MAX_INCIDENTS]).astype(np.int64)
        L, seg, cnt = signature_list(flags, inc, which)
        s, R = int(which.shape[0]), _hip.score_rows_per_block(L.shape[0])
        out.update({f"signatures_{name}_flag_share": float(flags.sum()) / n, f"signatures_{name}_incidents": s,
                    f"signatures_{name}_list_rows": int(L.shape[0]), f"signatures_{name}_block_rows": R,
                    f"signatures_{name}_workgroups": -(-int(L.shape[0]) // R)})
        if not L.shape[0]:
            continue
        # the two launches alone: one descriptor set, the list and the results on the device
        state, _ = eng._score_state(det)
        offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt)])
        o, = _hip.incident_signatures([state], [rows_dev], [L], [seg], [offsets], R)
        wdev, sdev, part = o["keep"]
        desc, fold = _hip.signature_desc([state], [rows_dev], [wdev], [sdev], [offsets], part, [o], R)
        dptr, fptr = rt.desc.put(desc, fold)

        def launches():
            part.zero_()
            _hip._check(_hip.lib().fedmx_incident_signatures(dptr, len(desc), fptr, len(fold), rt.stream),
                        "fedmx_incident_signatures")

        out[f"signatures_{name}_launches_us"] = timeit(launches, reps=args.reps)[0]
        out[f"signatures_{name}_partial_mb"] = part.numel() / 1e6
        out[f"signatures_{name}_dense_residual_mb"] = 4.0 * L.shape[0] * dims.d_in / 1e6

        def fused(x):
            return eng.incident_signatures([det], [x], [flags], [inc], which=[which], block_rows=R)[0]

        def composed(x):
            l, sg, c = signature_list(flags, inc, which)
            r = eng.explain_rows([det], [x], top_k=5, which=[l], dense=True)[0].resid_full
            return signatures_report(which, c, R, *signature_sums(r, sg, s, R), 5)

        for where, x in (("host_rows", rows), ("device_rows", rows_dev)):
            wall = {"fused": [], "composed": []}
            res = {}
            for i in range(reps + 1):
                for path, fn in (("fused", fused), ("composed", composed)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res[path] = fn(x)
                    torch.cuda.synchronize()
                    if i:
                        wall[path].append(time.perf_counter() - t0)
            a, b = res["fused"], res["composed"]
            out[f"signatures_{name}_{where}_equal_bits"] = bool(
                all(getattr(a, k).tobytes() == getattr(b, k).tobytes()
                    for k in ("rows", "err_sum", "resid_sum", "bad", "idx", "share", "mean_resid")))
            fm, cm = float(np.median(wall["fused"])) * 1e3, float(np.median(wall["composed"])) * 1e3
            out[f"signatures_{name}_{where}_fused_ms"] = fm
            out[f"signatures_{name}_{where}_explain_plus_host_sums_ms"] = cm
            out[f"signatures_{name}_{where}_composed_over_fused"] = cm / fm
        t0 = time.perf_counter()
        r = eng.explain_rows([det], [rows_dev], top_k=5, which=[L], dense=True)[0].resid_full
        out[f"signatures_{name}_explain_dense_device_rows_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        signature_sums(r, seg, s, R)
        out[f"signatures_{name}_host_sums_ms"] = (time.perf_counter() - t0) * 1e3
    return out


def auc_large_timings(args) -> dict:
    """``--auc-large``: the multi-workgroup AUC path (fedmx_auc_large.hip)
    beside the host fallback it replaces, on the same tensors.  Per shape:
    ``*_launch_us`` the cached-plan launch sequence (events), ``*_call_us``
    ``_hip.auc_large`` with its workspace from torch's pool (events),
    ``*_engine_ms`` ``engine.auc`` as a round pays it (wall clock: auc_kernel's
    -1, a fetch, the large path, a second fetch) and ``*_host_ms`` the fallback
    it replaces (wall clock: auc_kernel's -1, a fetch, the D2H copy of the
    scores and ``_host.roc_auc``)."""
    from fedmse_decentralized_amd.ops import _host

    dev = torch.device("cuda", 0)
    eng = HipEngine(DEFAULT_DIMS, dev)
    g = torch.Generator(device="cpu").manual_seed(5)
    shapes = {"10k_in_100k": [(10_000, 90_000)], "100k_100k": [(100_000, 100_000)],
              "1m_1m": [(1_000_000, 1_000_000)], "10x_9k_10k": [(9_000, 10_000)] * 10}
    out = {}

    def wall(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def host_fallback(scores, labels):
        vals = eng.fetch([_hip.auc(scores, labels)])[0]
        for i in np.flatnonzero(vals == -1.0):
            s = scores[i].detach().double().cpu().numpy()
            vals[i] = _host.roc_auc(np.nan_to_num(s), labels[i].cpu().numpy())
        return vals

    for name, pairs in shapes.items():
        scores, labels = [], []
        for P, N in pairs:
            y = torch.cat([torch.ones(P, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)])
            y = y[torch.randperm(P + N, generator=g)]
            s = torch.rand(P + N, dtype=torch.float64, generator=g) + 0.2 * y
            scores.append(s.to(dev))
            labels.append(y.to(dev))
        rows = [P + N for P, N in pairs]
        ws = torch.empty(sum(rows), dtype=torch.float64, device=dev)
        ctr = torch.zeros(_hip.AUC_LARGE_CTR_WORDS * len(pairs), dtype=torch.int64, device=dev)
        res = torch.zeros(len(pairs), dtype=torch.float64, device=dev)
        desc = _hip.auc_large_desc(scores, labels, res.data_ptr(), ws.data_ptr(), ctr.data_ptr())
        blob = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        chunks, slices = _hip.auc_large_grid([min(p) for p in pairs], [max(p) for p in pairs])
        out[f"{name}_grid"] = [chunks, slices]
        out[f"{name}_launch_us"] = timeit(lambda: _hip.launch_auc_large(blob, len(pairs), max(rows), chunks, slices,
                                                                        dev), reps=args.reps)[0]
        out[f"{name}_call_us"] = timeit(lambda: _hip.auc_large(scores, labels), reps=args.reps)[0]
        out[f"{name}_engine_ms"] = wall(lambda: eng.auc(scores, labels), args.reps)
        out[f"{name}_host_ms"] = wall(lambda: host_fallback(scores, labels), max(3, args.reps // 4))
        new, old = eng.auc(scores, labels), host_fallback(scores, labels)
        out[f"{name}_equal_bits"] = bool(np.array_equal(new, old)) and bool(np.array_equal(res.cpu().numpy(), old))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--auc-large", action="store_true", help="only the large-class AUC timings (the multi-workgroup "
                   "path beside the host fallback it replaces)")
    p.add_argument("--score-rows", action="store_true", help="only the deployed-detector scoring timings "
                   "(score_rows_kernel over --score-n raw rows, AE and CEN, beside the chain composed from "
                   "transform + pad + copy + forward_rows + cen_scores)")
    p.add_argument("--explain-rows", action="store_true", help="only the alarm-explanation timings "
                   "(explain_rows_kernel over --score-n raw rows: all rows at K = 5, 5 %% through which, dense "
                   "mode, beside score_rows_kernel on the same rows)")
    p.add_argument("--monitor-rows", action="store_true", help="only the drift-monitoring timings "
                   "(monitor_rows_kernel + monitor_fold_kernel over --score-n raw rows, AE and CEN, beside "
                   "score_rows_kernel on the same rows and host numpy computing the feature statistics)")
    p.add_argument("--incidents", action="store_true", help="only the incident-grouping timings (the launches of "
                   "fedmx_incident.hip over --score-n rows at flag densities 0.05 and 0.5, beside score_rows_kernel "
                   "on the same rows and score_rows + incidents_numpy on the host)")
    p.add_argument("--signatures", action="store_true", help="only the incident-signature timings (the two launches "
                   "of fedmx_signature.hip over the flagged rows of --score-n rows at flag densities 0.05 and 0.5, and "
                   "the whole call beside explain_rows(dense) + signature_sums on the host)")
    p.add_argument("--monitor-kernels-only", action="store_true", help="with --monitor-rows: only the event-timed "
                   "launches (to compare builds of the kernel library)")
    p.add_argument("--score-n", type=int, default=1_000_000)
    p.add_argument("--latent-scorer", action="store_true", help="only the latent-scorer timings (knn_score_kernel "
                   "beside cen_score_kernel, the evaluation chain and ms / round under either scorer)")
    p.add_argument("--scorer-rounds", type=int, default=200)
    p.add_argument("--detect", action="store_true", help="only the detection-metric timings (detect_kernel beside "
                   "auc_kernel, and ms / round under --metric detection vs classification)")
    p.add_argument("--detect-rounds", type=int, default=200)
    p.add_argument("--aggregation", action="store_true", help="only the distance-based aggregation rules' timings "
                   "(krum / multi_krum and geomed at k = 5, 40 and 256 beside the weighted sum over the same rows)")
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--clients", type=int, default=10)
    p.add_argument("--train-clients", type=int, default=5)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--train-only", action="store_true", help="only the training-kernel timings (A/B of builds)")
    args = p.parse_args()
    if args.score_rows or args.auc_large or args.explain_rows or args.monitor_rows or args.incidents \
            or args.signatures:
        out = (score_rows_timings if args.score_rows else explain_rows_timings if args.explain_rows
               else monitor_rows_timings if args.monitor_rows else incidents_timings if args.incidents
               else signatures_timings if args.signatures else auc_large_timings)(args)
        print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}))
        return
    dev = torch.device("cuda", 0)
    raws = generate_federation(SyntheticSpec(kind="nbaiot", n_clients=args.clients, seed=1))
    clients, dev_set = prepare_federation(raws, 1234)
    init, _ = init_client_params(args.clients, 0)
    eng = HipEngine(DEFAULT_DIMS, dev)
    eng.setup([c.train for c in clients], [c.valid for c in clients], [c.test for c in clients],
              [c.test_label for c in clients], init)
    if args.aggregation:
        out = aggregation_timings(eng, args)
        print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}))
        return
    if args.detect or args.latent_scorer:
        out = (detect_timings if args.detect else scorer_timings)(eng, clients, args)
        print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}))
        return
    out = {}
    sel = list(range(args.train_clients))
    # fixed-epoch training (patience large so every epoch runs)
    hp = TrainHParams(epochs=args.epochs, batch_size=12, lr=1e-3, shrink_lambda=5.0, patience=10 ** 6)
    n_train = [c.train.shape[0] for c in clients[:args.train_clients]]
    n_valid = [c.valid.shape[0] for c in clients[:args.train_clients]]
    steps = max((n + 11) // 12 for n in n_train) * args.epochs
    vsteps = max((n + 11) // 12 for n in n_valid) * args.epochs
    med, mn = timeit(lambda: eng.train_async(sel, hp), reps=args.reps)
    out["train_launch_us"] = med
    out["train_launch_us_min"] = mn
    out["train_steps_per_client"] = steps
    out["valid_batches_per_client"] = vsteps
    out["us_per_train_step_upper"] = med / steps
    hp1 = TrainHParams(epochs=args.epochs, batch_size=12, lr=1e-3, shrink_lambda=5.0, patience=10 ** 6)
    med1, _ = timeit(lambda: eng.train_async([0], hp1), reps=args.reps)
    out["train_launch_1client_us"] = med1
    hpp = TrainHParams(epochs=args.epochs, batch_size=12, lr=1e-3, shrink_lambda=5.0, fedprox_mu=0.001,
                       patience=10 ** 6)
    out["train_launch_fedprox_us"] = timeit(lambda: eng.train_async(sel, hpp), reps=args.reps)[0]
    _hip.TRAIN_COMPACT = False   # identity internal order (no padded k-steps skipped)
    out["train_launch_identity_order_us"] = timeit(lambda: eng.train_async(sel, hp), reps=args.reps)[0]
    _hip.TRAIN_COMPACT = True
    # batch 64 (the thesis's GPU runs): helper-wave kernel (16-row chunks) vs the 4-wave kernel
    hp64 = TrainHParams(epochs=args.epochs, batch_size=64, lr=1e-3, shrink_lambda=5.0, patience=10 ** 6)
    out["train_launch_b64_us"] = timeit(lambda: eng.train_async(sel, hp64), reps=args.reps)[0]
    hp64p = TrainHParams(epochs=args.epochs, batch_size=64, lr=1e-3, shrink_lambda=5.0, fedprox_mu=0.001,
                         patience=10 ** 6)
    out["train_launch_b64_fedprox_us"] = timeit(lambda: eng.train_async(sel, hp64p), reps=args.reps)[0]
    prev, _hip.TRAIN_HELPER = _hip.TRAIN_HELPER, False
    out["train_launch_b64_4wave_us"] = timeit(lambda: eng.train_async(sel, hp64), reps=args.reps)[0]
    _hip.TRAIN_HELPER = prev
    if args.train_only:
        print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}))
        return
    allc = list(range(args.clients))
    items = [(c, eng.store.rows("test", c)) for c in allc]
    out["fwd_sse_all_test_us"] = timeit(lambda: eng.forward_rows(eng.store.params, items, True, False))[0]
    items2 = []
    for c in allc:
        items2 += [(c, eng.store.rows("train", c)), (c, eng.store.rows("test", c))]
    out["fwd_latent_train_test_us"] = timeit(lambda: eng.forward_rows(eng.store.params, items2, False, True))[0]
    _, lat = eng.forward_rows(eng.store.params, items2, False, True)
    out["cen_us"] = timeit(lambda: eng.cen_scores(lat[0::2], lat[1::2]))[0]
    sc = eng.cen_scores(lat[0::2], lat[1::2])
    labs = [eng.store.test_label[int(eng.store.test_off[c]):int(eng.store.test_off[c + 1])] for c in allc]
    out["auc_us"] = timeit(lambda: _hip.auc(sc, labs))[0]
    V = eng.to_device(clients[0].valid)
    out["standardize_us"] = timeit(lambda: eng.standardize_ddof1(V))[0]
    stack = eng.store.params[:5].contiguous()
    out["weighted_sum_us"] = timeit(lambda: eng.weighted_sum(stack, [0.2] * 5))[0]
    out["param_drift_us"] = timeit(lambda: eng.param_drift(stack[:2], stack[3]))[0]
    # robust aggregation (trimmed_mean at the default ratio; fedmx_robust.hip), the
    # extra launch a trimmed_mean / median round pays behind elect_wsum, next to
    # the plain weighted sum over the same rows: k = 5 (the flagship round) and
    # k = 40 (the 8-rank job's selection)
    from fedmse_decentralized_amd.protocol.aggregation import trim_count  # noqa: E402

    agg_out = torch.empty(stack.shape[1], dtype=torch.float32, device=dev)
    for kk in (5, 40):
        st = eng.store.params[torch.arange(kk, device=dev) % args.clients].contiguous()
        t = trim_count("trimmed_mean", kk, 0.2)
        out[f"weighted_sum_k{kk}_us"] = timeit(lambda: _hip.weighted_sum(st, [1.0 / kk] * kk, out=agg_out))[0]
        out[f"robust_agg_k{kk}_us"] = timeit(lambda: _hip.robust_aggregate_stack(st, t, out=agg_out))[0]
        out[f"robust_median_k{kk}_us"] = timeit(lambda: _hip.robust_aggregate_stack(st, (kk - 1) // 2, out=agg_out))[0]
        # krum / multi_krum (fedmx_krum.hip): the three launches a round of
        # these rules pays behind elect_wsum, over one preallocated workspace
        from fedmse_decentralized_amd.protocol.aggregation import krum_counts  # noqa: E402

        ws = torch.empty(_hip.krum_workspace_size(kk), dtype=torch.float64, device=dev)
        for ut in ("krum", "multi_krum"):
            kf, _, km = krum_counts(ut, kk, 0.2)
            out[f"{ut}_k{kk}_us"] = timeit(lambda: _hip.krum_aggregate_stack(st, kf, km, out=agg_out,
                                                                             workspace=ws))[0]
        # geomed (fedmx_geomed.hip): the T + 2 = 5 launches a round of this rule
        # pays behind elect_wsum at the default T = 3
        gws = torch.empty(_hip.geomed_workspace_size(kk, st.shape[1]), dtype=torch.float64, device=dev)
        out[f"geomed_k{kk}_us"] = timeit(lambda: _hip.geomed_aggregate_stack(st, 3, 1e-6, out=agg_out,
                                                                             workspace=gws))[0]
    t0 = time.perf_counter()
    for _ in range(20):
        evaluate_clients(eng, allc, "hybrid", "AUC")
    out["evaluate_hybrid_host_us"] = (time.perf_counter() - t0) / 20 * 1e6
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
