"""Robust aggregation (update types ``trimmed_mean`` / ``median``) on the CPU:
the torch engine against a literal numpy oracle of the rule, the trim counts,
the median against numpy, the guaranteed robustness bound, the host round
under a poisoning client, two in-process ranks, and the command line.

The rule (protocol/aggregation.py): per coordinate the k values get a 32-bit
key whose unsigned order is -inf < ... < -0 < +0 < ... < +inf < NaN, model j's
rank is #{l : key_l < key_j or (key_l == key_j and l < j)}, the models with
t <= rank < k - t are kept, their values are added in selection order in fp32
(one rounding per add, starting from the first kept value) and divided by
(float)(k - 2t).

Bit comparisons treat every NaN as the same value: IEEE 754 leaves the payload
and sign of a NaN result open (the kernel returns the canonical quiet NaN,
numpy and torch propagate an operand's payload).
"""
import threading

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.config import ExperimentConfig

SMALL = dict(normal_rows=(90, 100), abnormal_rows=(120, 130), test_normal_rows=20)


# ----------------------------------------------------------------------------
# oracle (shared with tests/test_robust_aggregation_gpu.py)
# ----------------------------------------------------------------------------

def oracle_keys(stack: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(stack, dtype=np.float32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return key


def oracle_literal(stack: np.ndarray, t: int) -> np.ndarray:
    """The rule, coordinate by coordinate and pair by pair."""
    k, P = stack.shape
    key = oracle_keys(stack)
    out = np.empty(P, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(P):
            acc = None
            for j in range(k):
                rank = sum(1 for l in range(k) if key[l, i] < key[j, i] or (key[l, i] == key[j, i] and l < j))
                if t <= rank < k - t:
                    acc = stack[j, i] if acc is None else np.float32(acc + stack[j, i])
            out[i] = np.float32(acc) / np.float32(k - 2 * t)
    return out


def oracle_rank(stack: np.ndarray) -> np.ndarray:
    """rank[j, i] as the position of model j in a stable argsort of the keys."""
    k, P = stack.shape
    order = np.argsort(oracle_keys(stack), axis=0, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(k)[:, None], (k, P)), axis=0)
    return rank


def oracle_fast(stack: np.ndarray, t: int, rank: np.ndarray = None) -> np.ndarray:
    """The same rule with the stable-argsort rank (``oracle_rank``; may be
    passed in when several t share a stack) and the in-order sum vectorised
    over the coordinates (large k x P; checked against ``oracle_literal``
    below)."""
    k, P = stack.shape
    if rank is None:
        rank = oracle_rank(stack)
    kept = (rank >= t) & (rank < k - t)
    acc = np.zeros(P, dtype=np.float32)
    started = np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(k):
            acc = np.where(kept[j], np.where(started, acc + stack[j], stack[j]), acc).astype(np.float32)
            started |= kept[j]
        return acc / np.float32(k - 2 * t)


LEVELS = np.array([-1.5, -0.25, 0.0, 0.125, 0.7, 1.0, 3.0], dtype=np.float32)
# +-0, +-inf, +-NaN, denormals (the smallest, a negative one, the largest)
SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
                         0x00000001, 0x80012345, 0x007FFFFF], dtype=np.uint32)


def make_stack(rng, rows: int, P: int, special: float = 0.08) -> np.ndarray:
    """Values quantised to seven levels (frequent ties) with +-0, +-inf, NaN
    and denormals sprinkled in."""
    x = LEVELS[rng.integers(0, len(LEVELS), size=(rows, P))]
    m = rng.random((rows, P)) < special
    x.view(np.uint32)[m] = SPECIAL_BITS[rng.integers(0, len(SPECIAL_BITS), size=int(m.sum()))]
    return x


def assert_same_bits(got: np.ndarray, want: np.ndarray):
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    np.testing.assert_array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])


def trims(k: int):
    return sorted({t for t in (0, 1, (k - 1) // 2) if 2 * t < k})


def _engine():
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
    from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS

    return TorchEngine(DEFAULT_DIMS, torch.device("cpu"))


# ----------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 5, 6, 9])
def test_torch_engine_matches_literal_oracle(k):
    rng = np.random.default_rng(100 + k)
    stack = make_stack(rng, k, 257)
    assert np.isnan(stack).any() or k == 1
    eng = _engine()
    for t in trims(k):
        want = oracle_literal(stack, t)
        assert_same_bits(eng.robust_aggregate(torch.from_numpy(stack), t).numpy(), want)
        assert_same_bits(oracle_fast(stack, t), want)
    with pytest.raises(ValueError):
        eng.robust_aggregate(torch.from_numpy(stack), (k + 1) // 2)


def test_single_model_and_signed_zero_pass_through():
    x = np.array([[-0.0, 0.0, 1.0, -np.inf]], dtype=np.float32)
    assert_same_bits(_engine().robust_aggregate(torch.from_numpy(x), 0).numpy(), x[0])
    # -0 ranks below +0: the median of (-0, +0, +0) is +0, of (-0, -0, +0) is -0
    y = np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, -0.0]], dtype=np.float32)
    assert_same_bits(_engine().robust_aggregate(torch.from_numpy(y), 1).numpy(), np.array([0.0, -0.0], np.float32))


def test_trim_count():
    from fedmse_decentralized_amd.protocol.aggregation import ROBUST_TYPES, UPDATE_TYPES, make_plan, trim_count

    assert [trim_count("trimmed_mean", k, 0.2) for k in range(1, 13)] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2]
    for k in range(1, 40):
        assert trim_count("trimmed_mean", k, 0.49) == min(int(0.49 * k), (k - 1) // 2) <= (k - 1) // 2
        assert k - 2 * trim_count("trimmed_mean", k, 0.49) >= 1
    assert [trim_count("trimmed_mean", k, 0.49) for k in (1, 2, 3, 4)] == [0, 0, 1, 1]   # clamped: 0.49 * 4 = 1.96
    assert [trim_count("median", k) for k in (1, 2, 5, 6)] == [0, 0, 2, 2]
    assert ROBUST_TYPES == ("trimmed_mean", "median") and set(ROBUST_TYPES) < set(UPDATE_TYPES)
    for ut in ROBUST_TYPES:   # not (source, weight) plans: callers branch before make_plan
        with pytest.raises(ValueError):
            make_plan(ut, [0, 1, 2], 0)
    with pytest.raises(ValueError):
        trim_count("avg", 5, 0.2)


@pytest.mark.parametrize("k", [1, 2, 5, 6, 9, 40])
def test_median_matches_numpy(k):
    from fedmse_decentralized_amd.protocol.aggregation import trim_count

    rng = np.random.default_rng(7 + k)
    stack = rng.normal(size=(k, 257)).astype(np.float32)
    got = _engine().robust_aggregate(torch.from_numpy(stack), trim_count("median", k)).numpy()
    s = np.sort(stack, axis=0)
    if k % 2:
        want = s[k // 2]
        np.testing.assert_array_equal(got, np.median(stack, axis=0).astype(np.float32))
    else:
        want = (s[k // 2 - 1] + s[k // 2]) / np.float32(2)
    assert want.dtype == np.float32
    np.testing.assert_array_equal(got, want)


def test_trimmed_mean_stays_within_the_honest_range():
    """One of six models poisoned (x 50), one model trimmed per side: every
    kept value lies between two honest values, so the output lies in the
    honest rows' [min, max] up to the rounding of three adds and a division
    (<= 4 eps32 max|honest|).  The plain mean leaves that range."""
    from fedmse_decentralized_amd.protocol.aggregation import make_plan

    rng = np.random.default_rng(11)
    stack = rng.normal(size=(6, 257)).astype(np.float32)
    stack[2] *= 50.0
    honest = np.delete(stack, 2, axis=0)
    lo, hi = honest.min(0).astype(np.float64), honest.max(0).astype(np.float64)
    slack = 4 * float(np.finfo(np.float32).eps) * float(np.abs(honest).max())
    eng = _engine()
    out = eng.robust_aggregate(torch.from_numpy(stack), 1).numpy().astype(np.float64)
    assert np.all(out >= lo - slack) and np.all(out <= hi + slack)
    plan = make_plan("avg", list(range(6)), 0)
    mean = eng.weighted_sum(torch.from_numpy(stack), [w for _, w in plan]).numpy().astype(np.float64)
    assert np.any((mean < lo - slack) | (mean > hi + slack))


# ----------------------------------------------------------------------------
# the host round
# ----------------------------------------------------------------------------

@pytest.fixture()
def small_synthetic(monkeypatch):
    # shrink the synthetic clients so CPU tests stay fast
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    orig = synthetic.SyntheticSpec.resolved

    def resolved(self):
        s = orig(self)
        s.normal_rows, s.abnormal_rows, s.test_normal_rows = SMALL["normal_rows"], SMALL["abnormal_rows"], \
            SMALL["test_normal_rows"]
        return s
    monkeypatch.setattr(synthetic.SyntheticSpec, "resolved", resolved)
    federation._PREP_CACHE.clear()
    yield
    federation._PREP_CACHE.clear()


def _cfg(tmp_path, **kw):
    base = dict(synthetic="nbaiot", network_size=6, num_rounds=3, epoch=2, batch_size=12,
                output_root=str(tmp_path), backend="torch", device="cpu", log_level="WARNING",
                model_types=["hybrid"], update_types=["trimmed_mean"], num_participants=1.0,
                global_early_stop=False, save_checkpoints=False)
    base.update(kw)
    return ExperimentConfig(**base)


HONEST = [0, 1, 3, 4, 5]
# |final-round mean AUC over the honest clients, attacked - attack-free|
# three times the largest gap measured on the CPU over runs (seeds) 0-2 (the
# docstring of test_host_round_under_poisoning), below the 0.05 cap
AUC_MARGIN = 3 * 0.006456


def _final_auc(tmp_path, update_type, run, **kw):
    import json
    import os

    from fedmse_decentralized_amd.federation import Federation

    cfg = _cfg(tmp_path, update_types=[update_type], **kw)
    fed = Federation(cfg, "hybrid", update_type, run).setup()
    assert fed._fast is None
    rs = [fed.run_round() for _ in range(3)]
    fed.writer.flush()
    assert all(r.aggregator is not None for r in rs)
    params = fed.engine.store.params
    rep_dir = os.path.join(cfg.checkpoint_dir, f"Run_{run}", "AUC")
    (rep,) = [f for f in os.listdir(rep_dir) if f.endswith(f"_hybrid_{update_type}_results.json")]
    lines = [json.loads(l) for l in open(os.path.join(rep_dir, rep))]
    return float(np.mean(rs[-1].metrics[HONEST])), params, lines


@pytest.mark.parametrize("update_type", ["trimmed_mean", "median"])
def test_host_round_under_poisoning(tmp_path, small_synthetic, update_type):
    """Six clients, all selected, client 2 multiplies its update by 50 in every
    round.  The robust rules run, keep every honest client's parameters finite,
    write their reports under the new name, and the honest clients' final-round
    mean AUC stays within AUC_MARGIN of the attack-free run of the same rule.

    Observed |attacked - attack-free| gaps on the CPU, runs 0 / 1 / 2:
      trimmed_mean  0.000548  0.002955  0.006456
      median        0.000805  0.001662  0.001712
    (the attacked arm scored 0.974 - 0.987, the attack-free arm 0.967 - 0.986)
    margin = min(3 x the largest gap, 0.05) = 3 x 0.006456 = 0.019368.
    """
    from fedmse_decentralized_amd import federation

    for run in (0, 1, 2):
        federation._PREP_CACHE.clear()
        attacked, params, lines = _final_auc(tmp_path / f"a{run}", update_type, run, malicious_clients=[2],
                                             malicious_scale=50.0)
        clean, _, _ = _final_auc(tmp_path / f"c{run}", update_type, run)
        assert torch.isfinite(params[HONEST]).all()
        assert [l["round"] for l in lines] == [1, 2, 3] and all(l["update_type"] == update_type for l in lines)
        print(f"{update_type} run {run}: attacked {attacked:.6f} attack-free {clean:.6f} "
              f"gap {abs(attacked - clean):.6f}")
        assert abs(attacked - clean) <= AUC_MARGIN


def _run_threads(world, cfg, update_type, rounds):
    from fedmse_decentralized_amd.federation import Federation
    from fedmse_decentralized_amd.parallel.comm import ThreadComm

    comms = ThreadComm.group(world)
    out = [None] * world
    errs = []

    def worker(r):
        try:
            f = Federation(cfg, "hybrid", update_type, 0, comm=comms[r], device=torch.device("cpu")).setup()
            out[r] = [f.run_round() for _ in range(rounds)] + [f.engine.store.params.clone(), f.local]
        except Exception:  # pragma: no cover
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


def test_two_ranks_match_single_rank(tmp_path, small_synthetic):
    # six selected models, one trimmed per side; three clients per rank
    cfg = _cfg(tmp_path, malicious_clients=[2], malicious_scale=25.0)
    single = _run_threads(1, cfg, "trimmed_mean", 3)[0]
    outs = _run_threads(2, cfg, "trimmed_mean", 3)
    for r in range(3):
        for o in outs:
            assert o[r].aggregator == single[r].aggregator and o[r].aggregator is not None
            assert o[r].selected == single[r].selected
            np.testing.assert_array_equal(o[r].metrics, single[r].metrics)
    for o in outs:
        params, local = o[3], o[4]
        assert torch.equal(params, single[3][local[0]:local[-1] + 1])


def test_peer_api_aggregates_with_the_robust_rule(tmp_path, small_synthetic):
    from fedmse_decentralized_amd.federation import Federation

    fed = Federation(_cfg(tmp_path, update_types=["median"]), "hybrid", "median", 0).setup()
    peers = fed.peers()
    stack = fed.engine.store.params[:5].clone()
    stack[1] *= 40.0
    fed.engine.store.params[:5].copy_(stack)
    agg = peers[0].aggregate_models(peers[:5])
    assert_same_bits(agg.numpy(), oracle_fast(stack.numpy(), 2))


# ----------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------

def test_cli_accepts_the_robust_rules(capsys):
    import argparse

    from fedmse_decentralized_amd.config import add_arguments, from_args

    p = add_arguments(argparse.ArgumentParser())
    cfg = from_args(p.parse_args(["--update-types", "trimmed_mean", "median", "--robust-trim-ratio", "0.3"]))
    assert cfg.update_types == ["trimmed_mean", "median"] and cfg.robust_trim_ratio == 0.3
    assert ExperimentConfig().robust_trim_ratio == 0.2
    with pytest.raises(SystemExit):
        p.parse_args(["--help"])
    text = capsys.readouterr().out
    assert "trimmed_mean" in text and "median" in text and "--robust-trim-ratio" in text
