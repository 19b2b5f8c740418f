"""Krum / Multi-Krum aggregation (update types ``krum`` / ``multi_krum``) on
the CPU: numpy oracles of the rule, the counts, the torch engine against the
oracle bit for bit, the host round under a poisoning client, the command line.

The rule (protocol/aggregation.py), k models of P fp32 values, f assumed
poisoned, q = max(k - f - 2, 0), m = 1 (krum) or k - f (multi_krum):

1. d(i, j): e_c = fp32(a_c - b_c); s_c = (double)e_c * (double)e_c; s
   zero-extended to a multiple of 256; p_l = s_l + s_{l+256} + ... in that
   order in f64, l < 256; eight folds p_l += p_{l+h}, h = 128 .. 1; d = p_0;
   NaN -> +inf.
2. score_i: the k - 1 distances d(i, j) ranked ascending, ties by the smaller
   j; the q lowest added in order of j in f64 (q = 0: 0.0).
3. rank_i = #{l : score_l < score_i or (score_l == score_i and l < i)}; model
   i is kept iff rank_i < m.
4. per coordinate the kept values added in selection order in fp32, divided by
   (float)m.

Aggregates are compared bit for bit with every NaN taken as the same value
(``assert_same_bits`` of tests/test_robust_aggregation.py).
"""
import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.config import ExperimentConfig
from test_robust_aggregation import assert_same_bits

SMALL = dict(normal_rows=(90, 100), abnormal_rows=(120, 130), test_normal_rows=20)
RULES = ("krum", "multi_krum")
RATIOS = (0.0, 0.2)


# ----------------------------------------------------------------------------
# oracles (shared with tests/test_krum_aggregation_gpu.py)
# ----------------------------------------------------------------------------

def counts(rule: str, k: int, ratio: float):
    """(f, q, m) straight from the rule's text."""
    f = min(int(np.floor(ratio * k)), max((k - 3) // 2, 0))
    return f, max(k - f - 2, 0), 1 if rule == "krum" else k - f


def oracle_dist(stack: np.ndarray) -> np.ndarray:
    """Step 1 in the chunked order: D[k, k] float64, the diagonal 0."""
    stack = np.ascontiguousarray(stack, dtype=np.float32)
    k, P = stack.shape
    C = -(-P // 256)
    pad = np.zeros((k, C * 256), dtype=np.float32)
    pad[:, :P] = stack
    D = np.zeros((k, k), dtype=np.float64)
    blk = max(1, (1 << 16) // (k * 256))   # row blocks whose temporaries stay in the cache
    with np.errstate(all="ignore"):
        for i0 in range(0, k, blk):
            a = pad[i0:i0 + blk]
            p = np.zeros((a.shape[0], k, 256), dtype=np.float64)
            e32 = np.empty(p.shape, dtype=np.float32)
            e = np.empty_like(p)
            for c in range(C):
                np.subtract(a[:, None, c * 256:(c + 1) * 256], pad[None, :, c * 256:(c + 1) * 256], out=e32)
                e[...] = e32                 # one fp32 rounding, then exact in f64
                np.multiply(e, e, out=e)
                p += e
            h = 128
            while h >= 1:
                p = p[..., :h] + p[..., h:2 * h]
                h //= 2
            D[i0:i0 + blk] = p[..., 0]
    D[np.isnan(D)] = np.inf
    D[np.arange(k), np.arange(k)] = 0.0
    return D


def oracle_literal(stack: np.ndarray, D: np.ndarray, q: int, m: int):
    """Steps 2 to 4 pair by pair: (aggregate, kept mask, scores)."""
    k, P = stack.shape
    score = np.zeros(k, dtype=np.float64)
    for i in range(k):
        acc = None
        for j in range(k):
            if j == i:
                continue
            rank = sum(1 for l in range(k) if l != i and (D[i, l] < D[i, j] or (D[i, l] == D[i, j] and l < j)))
            if rank < q:
                acc = D[i, j] if acc is None else np.float64(acc + D[i, j])
        score[i] = 0.0 if acc is None else acc
    kept = np.zeros(k, dtype=np.int32)
    for i in range(k):
        rank = sum(1 for l in range(k) if score[l] < score[i] or (score[l] == score[i] and l < i))
        kept[i] = 1 if rank < m else 0
    return oracle_mean(stack, kept, m), kept, score


def oracle_mean(stack: np.ndarray, kept: np.ndarray, m: int) -> np.ndarray:
    pos = np.flatnonzero(kept)
    assert len(pos) == m
    with np.errstate(all="ignore"):
        acc = stack[pos[0]].astype(np.float32)
        for j in pos[1:]:
            acc = (acc + stack[j]).astype(np.float32)
        return acc / np.float32(m)


def oracle_fast(stack: np.ndarray, D: np.ndarray, q: int, m: int):
    """Steps 2 to 4 with stable argsorts (large k; checked against
    ``oracle_literal`` below)."""
    k = stack.shape[0]
    key = np.ascontiguousarray(D).view(np.uint64).copy()
    key[np.arange(k), np.arange(k)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    order = np.argsort(key, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(k)[None, :], (k, k)), axis=1)
    near = rank < q
    score = np.zeros(k, dtype=np.float64)
    for j in range(k):
        score = np.where(near[:, j], score + D[:, j], score)
    kept = np.zeros(k, dtype=np.int32)
    kept[np.argsort(score.view(np.uint64), kind="stable")[:m]] = 1
    return oracle_mean(stack, kept, m), kept, score


STACKS = ("random", "tie", "identical", "scaled", "inf", "nan", "subnormal")


def make_stack(kind: str, rng, k: int, P: int) -> np.ndarray:
    x = rng.normal(size=(k, P)).astype(np.float32)
    a, b = (k // 2, k - 1) if k >= 2 else (0, 0)
    if kind == "tie":            # two identical rows: exact ties, resolved by position
        x[b] = x[a]
    elif kind == "identical":
        x[:] = x[0]
    elif kind == "scaled":
        x[a] *= np.float32(25.0)
    elif kind == "inf":
        x[a, [0, P // 2, P - 1]] = np.inf
    elif kind == "nan":
        x[a, [1, P // 3, P - 2]] = np.nan
    elif kind == "subnormal":    # rows a and b differ by 2^-149 in one coordinate
        x[b] = x[a]
        c = P - 3
        x[a, c] = np.float32(2.0 ** -126)
        x[b, c] = np.float32(2.0 ** -126) + np.float32(2.0 ** -149)
    return x


def same_f64_bits(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float64).view(np.uint64),
                                  np.ascontiguousarray(want, dtype=np.float64).view(np.uint64))


def _engine():
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
    from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS

    return TorchEngine(DEFAULT_DIMS, torch.device("cpu"))


# ----------------------------------------------------------------------------
# the oracles themselves
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("k,P", [(2, 100), (5, 256), (9, 1000), (6, 9216)])
def test_oracle_dist_agrees_with_plain_float64(k, P):
    """A sanity bound on the oracle, not on the code under test."""
    x = np.random.default_rng(k * P).normal(size=(k, P)).astype(np.float32)
    D = oracle_dist(x)
    for i in range(k):
        for j in range(k):
            if i != j:
                e = (x[i] - x[j]).astype(np.float64)
                plain = (e ** 2).sum()
                assert abs(D[i, j] - plain) <= 1e-12 * plain
    same_f64_bits(D, D.T)


def test_oracle_dist_special_values():
    x = make_stack("subnormal", np.random.default_rng(3), 5, 300)
    D = oracle_dist(x)
    assert D[2, 4] == 2.0 ** -298 and D[4, 2] == 2.0 ** -298
    x = make_stack("inf", np.random.default_rng(3), 5, 300)
    D = oracle_dist(x)
    assert np.all(np.isinf(D[2, [0, 1, 3, 4]])) and np.isfinite(D[0, 1])
    x = make_stack("nan", np.random.default_rng(3), 5, 300)
    D = oracle_dist(x)
    assert np.all(D[[0, 1, 3, 4], 2] == np.inf) and not np.isnan(D).any()


@pytest.mark.parametrize("kind", STACKS)
@pytest.mark.parametrize("k", [1, 2, 3, 5, 9])
def test_oracle_fast_matches_literal(k, kind):
    x = make_stack(kind, np.random.default_rng(10 * k), k, 100)
    D = oracle_dist(x)
    for rule in RULES:
        for ratio in (0.0, 0.2, 0.49):
            _, q, m = counts(rule, k, ratio)
            a, ka, sa = oracle_literal(x, D, q, m)
            b, kb, sb = oracle_fast(x, D, q, m)
            assert_same_bits(a, b)
            np.testing.assert_array_equal(ka, kb)
            same_f64_bits(sa, sb)


# ----------------------------------------------------------------------------
# the counts
# ----------------------------------------------------------------------------

def test_krum_counts():
    from fedmse_decentralized_amd.protocol.aggregation import (KRUM_TYPES, ROBUST_TYPES, UPDATE_TYPES, krum_counts,
                                                               make_plan, trim_count)

    assert KRUM_TYPES == ("krum", "multi_krum") and set(KRUM_TYPES) < set(UPDATE_TYPES)
    assert ROBUST_TYPES == ("trimmed_mean", "median")
    # (f, q) per k; m = 1 / k - f
    table = {
        0.0: {k: (0, max(k - 2, 0)) for k in (*range(1, 10), 40, 1024)},
        0.2: {1: (0, 0), 2: (0, 0), 3: (0, 1), 4: (0, 2), 5: (1, 2), 6: (1, 3), 7: (1, 4), 8: (1, 5), 9: (1, 6),
              40: (8, 30), 1024: (204, 818)},
        0.49: {1: (0, 0), 2: (0, 0), 3: (0, 1), 4: (0, 2), 5: (1, 2), 6: (1, 3), 7: (2, 3), 8: (2, 4), 9: (3, 4),
               40: (18, 20), 1024: (501, 521)},
    }
    for ratio, rows in table.items():
        for k, (f, q) in rows.items():
            assert krum_counts("krum", k, ratio) == (f, q, 1), (ratio, k)
            assert krum_counts("multi_krum", k, ratio) == (f, q, k - f), (ratio, k)
            assert counts("multi_krum", k, ratio) == (f, q, k - f)
    for bad in (-0.1, 0.5, 1.0):
        with pytest.raises(ValueError):
            krum_counts("krum", 5, bad)
    with pytest.raises(ValueError):
        krum_counts("krum", 0, 0.2)
    with pytest.raises(ValueError):
        krum_counts("median", 5, 0.2)
    with pytest.raises(ValueError):
        trim_count("krum", 5, 0.2)
    for ut in KRUM_TYPES:   # not (source, weight) plans: callers branch before make_plan
        with pytest.raises(ValueError):
            make_plan(ut, [0, 1, 2], 0)


# ----------------------------------------------------------------------------
# the torch engine
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("P", [100, 9216])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 9, 40])
def test_torch_engine_matches_oracle(k, P):
    eng = _engine()
    for n, kind in enumerate(STACKS):
        x = make_stack(kind, np.random.default_rng(1000 * k + P + n), k, P)
        D = oracle_dist(x)
        for rule in RULES:
            for ratio in RATIOS:
                f, q, m = counts(rule, k, ratio)
                want, kept, _ = oracle_fast(x, D, q, m)
                got, pos = eng.krum_aggregate(torch.from_numpy(x), f, m)
                assert pos == np.flatnonzero(kept).tolist(), (kind, rule, ratio)
                assert_same_bits(got.numpy(), want)
                bad = k // 2
                if kind in ("inf", "nan") and f >= 1:
                    assert bad not in pos
                if kind == "scaled" and k >= 5:
                    assert bad not in pos or f == 0 and rule == "multi_krum"
                if rule == "krum":   # one model's row unchanged
                    assert_same_bits(got.numpy(), x[pos[0]])
                if kind == "identical" and f == 0 and rule == "multi_krum":
                    with np.errstate(all="ignore"):
                        assert_same_bits(got.numpy(), _times(x[0], m) / np.float32(m))
                    assert pos == list(range(k))
                if kind == "identical" and rule == "krum":
                    assert pos == [0]    # every score ties: the first position wins


def _times(row, m):
    acc = row.copy()
    for _ in range(m - 1):
        acc = (acc + row).astype(np.float32)
    return acc


def test_torch_engine_literal_oracle_and_errors():
    eng = _engine()
    x = make_stack("tie", np.random.default_rng(7), 6, 300)
    D = oracle_dist(x)
    for rule in RULES:
        f, q, m = counts(rule, 6, 0.2)
        want, kept, _ = oracle_literal(x, D, q, m)
        got, pos = eng.krum_aggregate(torch.from_numpy(x), f, m)
        assert_same_bits(got.numpy(), want)
        assert pos == np.flatnonzero(kept).tolist()
    for f, m in [(0, 0), (0, 7), (-1, 1)]:
        with pytest.raises(ValueError):
            eng.krum_aggregate(torch.from_numpy(x), f, m)


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
                model_types=["hybrid"], update_types=["multi_krum"], num_participants=1.0,
                global_early_stop=False, save_checkpoints=False, malicious_clients=[2], malicious_scale=25.0)
    base.update(kw)
    return ExperimentConfig(**base)


def _host_rounds(tmp_path, update_type, rounds=3):
    """The rounds' results and the first aggregating round's aggregate."""
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.federation import Federation

    federation._PREP_CACHE.clear()
    fed = Federation(_cfg(tmp_path, update_types=[update_type]), "hybrid", update_type, 0).setup()
    assert fed._fast is None
    aggs = []
    eng = fed.engine
    krum, wsum = eng.krum_aggregate, eng.weighted_sum

    def krum_rec(stack, f, m):
        out = krum(stack, f, m)
        aggs.append(out[0].clone())
        return out

    def wsum_rec(stack, weights):
        out = wsum(stack, weights)
        aggs.append(out.clone())
        return out
    eng.krum_aggregate, eng.weighted_sum = krum_rec, wsum_rec
    rs = [fed.run_round() for _ in range(rounds)]
    fed.writer.flush()
    return rs, aggs


def test_host_round_under_poisoning(tmp_path, small_synthetic, caplog):
    """Six clients, all selected (k = 6, f = 1, q = 3, m = 5), client 2
    multiplies its update by 25 in every round: multi_krum keeps the five
    others, krum keeps one of them, and the plain mean's first aggregate is
    more than 3 times as long as multi_krum's (the poisoned row contributes
    about 25 / 6 of an honest norm to the mean)."""
    import logging

    with caplog.at_level(logging.INFO, logger="fedmx"):
        rs, aggs = _host_rounds(tmp_path / "mk", "multi_krum")
    assert any(r.aggregator is not None for r in rs)
    n_agg = 0
    for r in rs:
        if r.aggregator is None:
            assert r.agg_kept is None
            continue
        n_agg += 1
        assert len(r.agg_kept) == 5 and 2 not in r.agg_kept
        assert r.agg_kept == [c for c in r.selected if c in r.agg_kept]   # selection order
    assert sum("Aggregate keeps clients" in rec.getMessage() for rec in caplog.records) == n_agg
    rs1, _ = _host_rounds(tmp_path / "k", "krum")
    assert any(r.aggregator is not None for r in rs1)
    for r in rs1:
        if r.aggregator is not None:
            assert len(r.agg_kept) == 1 and 2 not in r.agg_kept
    rs0, aggs0 = _host_rounds(tmp_path / "avg", "avg")
    assert all(r.agg_kept is None for r in rs0)
    first = next(i for i, r in enumerate(rs) if r.aggregator is not None)
    assert first == next(i for i, r in enumerate(rs0) if r.aggregator is not None) == 0
    assert rs0[0].selected == rs[0].selected
    n_avg, n_mk = float(aggs0[0].double().norm()), float(aggs[0].double().norm())
    print(f"first aggregate: |avg| = {n_avg:.4f}, |multi_krum| = {n_mk:.4f}, ratio {n_avg / n_mk:.3f}")
    assert n_avg > 3.0 * n_mk


def test_peer_api_aggregates_with_krum(tmp_path, small_synthetic):
    from fedmse_decentralized_amd.federation import Federation

    fed = Federation(_cfg(tmp_path, malicious_clients=[]), "hybrid", "multi_krum", 0).setup()
    peers = fed.peers()
    stack = fed.engine.store.params[:5].clone()
    stack[1] *= 40.0
    fed.engine.store.params[:5].copy_(stack)
    agg = peers[0].aggregate_models(peers[:5])
    f, q, m = counts("multi_krum", 5, 0.2)
    want, kept, _ = oracle_fast(stack.numpy(), oracle_dist(stack.numpy()), q, m)
    assert kept.tolist() == [1, 0, 1, 1, 1]
    assert_same_bits(agg.numpy(), want)


# ----------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------

def test_cli_lists_the_krum_rules(capsys):
    import argparse

    import main as driver
    from fedmse_decentralized_amd.config import add_arguments, from_args

    p = add_arguments(argparse.ArgumentParser())
    cfg = from_args(p.parse_args(["--update-types", "krum", "multi_krum", "--robust-trim-ratio", "0.3"]))
    assert cfg.update_types == ["krum", "multi_krum"] and cfg.robust_trim_ratio == 0.3
    with pytest.raises(SystemExit):
        driver.main(["--help"])
    text = capsys.readouterr().out
    import re

    assert re.search(r"(?<![\w])krum\b", text) and "multi_krum" in text and "--robust-trim-ratio" in text


def test_unknown_rule_still_raises(tmp_path, small_synthetic):
    from fedmse_decentralized_amd.federation import Federation
    from fedmse_decentralized_amd.protocol.aggregation import make_plan

    with pytest.raises(ValueError):
        make_plan("bulyan", [0, 1, 2], 0)
    fed = Federation(_cfg(tmp_path, update_types=["bulyan"], malicious_clients=[]), "hybrid", "bulyan", 0).setup()
    with pytest.raises(ValueError):
        for _ in range(3):
            fed.run_round()
