"""Geometric-median aggregation (update type ``geomed``; RFA) on the CPU: two
numpy oracles of the rule against each other, the torch engine against them
bit for bit, the rule's properties, the configuration and command line, the
host round under a poisoning client and the Peer API.

The rule (protocol/aggregation.py), k models of P fp32 values in selection
order, T iterations, smoothing nu:

* block sum of a length-P f64 vector: zero-extended to nb = ceil(P / 256)
  blocks of 256; in a block eight folds p_l += p_{l+h}, h = 128 .. 1, give q_b
  = p_0; the sum is ((+0.0 + q_0) + q_1) + ... in block order.
* lane sum of a length-k f64 vector: zero-extended to a multiple of 256; lane
  l adds x_l + x_{l+256} + ... from +0.0; then the same eight folds.

1. d_i(z): e_c = fp32(theta_i[c] - z[c]); s_c = (double)e_c * (double)e_c; d_i
   the block sum of s; NaN or +inf -> +inf (the row is bad for that step).
2. step -1: d_i = d_i(z = 0); beta_i = 1.0 for a finite d_i, else 0.0.
3. steps t = 0 .. T: B = lane sum of beta; B == 0: w = 0, the aggregate is the
   NaN 0x7FC00000 everywhere, end.  Else w_i = beta_i / B; acc = +0.0, then acc
   = acc + (w_i * (double)theta_i[c]) for i in order with beta_i != 0; z_t =
   (float)acc.  t == T: stop; else d_i = d_i(z_t), beta_i = 1 / max(sqrt(d_i),
   nu) for a finite d_i, else 0.0.
4. the aggregate z_T, the weights w that formed it and the squared distances d
   those weights came from.

Everything is compared bit for bit; an aggregate's NaNs count as one value
(only the all-rows-bad aggregate's bits are fixed by the rule, and checked).
"""
import math

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.config import ExperimentConfig
from test_robust_aggregation import assert_same_bits

SMALL = dict(normal_rows=(90, 100), abnormal_rows=(120, 130), test_normal_rows=20)
NAN_BITS = 0x7FC00000
INF = float("inf")


# ----------------------------------------------------------------------------
# oracles (shared with tests/test_geomed_aggregation_gpu.py)
# ----------------------------------------------------------------------------

def _fold_literal(p):
    """Eight folds of 256 Python floats; p_0."""
    p = list(p)
    h = 128
    while h >= 1:
        for l in range(h):
            p[l] = p[l] + p[l + h]
        h //= 2
    return p[0]


def _dist_literal(row: np.ndarray, z) -> float:
    P = row.shape[0]
    with np.errstate(all="ignore"):
        e = row if z is None else (row - z).astype(np.float32)
    s = [float(x) * float(x) for x in e]
    nb = -(-P // 256)
    s += [0.0] * (nb * 256 - P)
    d = 0.0
    for b in range(nb):
        d = d + _fold_literal(s[256 * b:256 * b + 256])
    return INF if (d != d or d == INF) else d


def oracle_literal(stack: np.ndarray, iters: int, nu: float):
    """The rule row by row in Python floats: (aggregate f32[P], weights f64[k],
    squared distances f64[k])."""
    stack = np.ascontiguousarray(stack, dtype=np.float32)
    k, P = stack.shape
    nu = float(nu)
    d = [_dist_literal(stack[i], None) for i in range(k)]
    beta = [1.0 if x < INF else 0.0 for x in d]
    for t in range(iters + 1):
        lanes = [0.0] * 256
        for i in range(k):               # lane i % 256, in order of i
            lanes[i % 256] = lanes[i % 256] + beta[i]
        B = _fold_literal(lanes)
        if B == 0.0:
            z = np.full(P, NAN_BITS, dtype=np.uint32).view(np.float32)
            w = [0.0] * k
            break
        w = [x / B for x in beta]
        acc = np.zeros(P, dtype=np.float64)
        with np.errstate(all="ignore"):
            for i in range(k):
                if beta[i] != 0.0:
                    acc = acc + np.float64(w[i]) * stack[i].astype(np.float64)
            z = acc.astype(np.float32)
        if t == iters:
            break
        d = [_dist_literal(stack[i], z) for i in range(k)]
        beta = [1.0 / max(math.sqrt(x), nu) if x < INF else 0.0 for x in d]
    return z, np.asarray(w, dtype=np.float64), np.asarray(d, dtype=np.float64)


def _fold(p: np.ndarray) -> np.ndarray:
    h = 128
    while h >= 1:
        p = p[..., :h] + p[..., h:2 * h]
        h //= 2
    return p[..., 0]


def oracle_fast(stack: np.ndarray, iters: int, nu: float):
    """The rule vectorised over rows and coordinates (large k and P; checked
    against ``oracle_literal`` below)."""
    stack = np.ascontiguousarray(stack, dtype=np.float32)
    k, P = stack.shape
    nb, C = -(-P // 256), -(-k // 256)
    pad = np.zeros((k, nb * 256), dtype=np.float32)
    pad[:, :P] = stack

    def dist(z):
        with np.errstate(all="ignore"):
            if z is None:
                e = pad.astype(np.float64)
            else:
                zp = np.zeros(nb * 256, dtype=np.float32)
                zp[:P] = z
                e = (pad - zp).astype(np.float64)
            s = e * e
            s[:, P:] = 0.0
            q = _fold(s.reshape(k, nb, 256))
            d = np.zeros(k, dtype=np.float64)
            for b in range(nb):
                d = d + q[:, b]
        d[~(d < INF)] = INF
        return d

    def lane_sum(x):
        xp = np.zeros(C * 256, dtype=np.float64)
        xp[:k] = x
        p = np.zeros(256, dtype=np.float64)
        with np.errstate(all="ignore"):
            for c in range(C):
                p = p + xp[256 * c:256 * c + 256]
            return float(_fold(p))

    d = dist(None)
    beta = np.where(d < INF, 1.0, 0.0)
    for t in range(iters + 1):
        B = lane_sum(beta)
        if B == 0.0:
            return np.full(P, NAN_BITS, dtype=np.uint32).view(np.float32), np.zeros(k), d
        with np.errstate(all="ignore"):
            w = beta / B
            acc = np.zeros(P, dtype=np.float64)
            for i in np.flatnonzero(beta != 0.0):
                acc = acc + w[i] * stack[i].astype(np.float64)
            z = acc.astype(np.float32)
        if t == iters:
            break
        d = dist(z)
        with np.errstate(all="ignore"):
            beta = np.where(d < INF, 1.0 / np.maximum(np.sqrt(d), nu), 0.0)
    return z, w, d


STACKS = ("random", "crowd", "identical", "nan", "inf", "ninf", "huge", "subnormal", "allbad")


def make_stack(kind: str, rng, k: int, P: int) -> np.ndarray:
    x = rng.normal(size=(k, P)).astype(np.float32)
    a = k // 2
    if kind == "crowd":          # honest rows around one base, one pushed away
        x = (rng.normal(size=(1, P)) + 0.01 * rng.normal(size=(k, P))).astype(np.float32)
        x[a] = x[a] * np.float32(25.0) + np.float32(3.0)
    elif kind == "identical":
        x[:] = x[0]
    elif kind == "nan":
        x[a, int(rng.integers(P))] = np.nan
    elif kind == "inf":
        x[a, int(rng.integers(P))] = np.inf
    elif kind == "ninf":
        x[a, int(rng.integers(P))] = -np.inf
    elif kind == "huge":         # finite rows of +-3e38: squared distances near 1e81, tiny weights
        x[a] = np.float32(3e38)
        if k >= 3:
            x[0] = np.float32(-3e38)
    elif kind == "subnormal":
        x *= np.float32(1e-42)
    elif kind == "allbad":
        x[np.arange(k), rng.integers(P, size=k)] = np.nan
    return x


def same_f64_bits(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float64).view(np.uint64),
                                  np.ascontiguousarray(want, dtype=np.float64).view(np.uint64))


def assert_same_result(got, want):
    """(aggregate, weights, dist) bit for bit."""
    assert_same_bits(got[0], want[0])
    same_f64_bits(got[1], want[1])
    if len(got) > 2 and got[2] is not None:
        same_f64_bits(got[2], want[2])


def _engine():
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
    from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS

    return TorchEngine(DEFAULT_DIMS, torch.device("cpu"))


def _eng_run(eng, x, iters, nu):
    agg, w = eng.geomed_aggregate(torch.from_numpy(x), iters, nu)
    assert isinstance(w, list) and len(w) == x.shape[0] and all(isinstance(v, float) for v in w)
    return agg.numpy(), np.asarray(w, dtype=np.float64)


# ----------------------------------------------------------------------------
# the oracles themselves
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_oracle_fast_matches_literal(seed):
    """6 x 45 random small cases: every stack kind, k <= 9, P <= 600 (one to
    three blocks, block edges included), T in 0..3 and a few smoothings."""
    rng = np.random.default_rng(100 + seed)
    edges = (1, 255, 256, 257, 511, 512, 513, 600)
    for n in range(45):
        kind = STACKS[n % len(STACKS)]
        k = int(rng.integers(1, 10))
        P = int(edges[rng.integers(len(edges))]) if n % 3 == 0 else int(rng.integers(1, 601))
        T = int(rng.integers(0, 4))
        nu = float((1e-6, 1e-12, 0.5, 1e3)[int(rng.integers(4))])
        x = make_stack(kind, rng, k, P)
        assert_same_result(oracle_fast(x, T, nu), oracle_literal(x, T, nu))


def test_oracle_agrees_with_plain_float64():
    """A sanity bound on the oracle, not on the code under test: plain numpy
    Weiszfeld steps in f64 give the same point to fp32 accuracy."""
    rng = np.random.default_rng(5)
    x = make_stack("crowd", rng, 6, 9216)
    z, w, d = oracle_fast(x, 3, 1e-6)
    x64 = x.astype(np.float64)
    zz = x64.mean(0)
    for _ in range(3):
        r = np.sqrt(((x64 - zz) ** 2).sum(1))
        ww = (1.0 / np.maximum(r, 1e-6))
        ww /= ww.sum()
        zz = (ww[:, None] * x64).sum(0)
    assert np.max(np.abs(z - zz)) <= 1e-5 * np.max(np.abs(zz))
    np.testing.assert_allclose(w, ww, rtol=1e-4)
    assert abs(w.sum() - 1.0) < 1e-12 and np.argmin(w) == 3
    # far closer to the honest rows' mean than the plain mean is
    honest = np.delete(x64, 3, axis=0).mean(0)
    near, far = np.linalg.norm(z - honest), np.linalg.norm(x64.mean(0) - honest)
    print(f"k = 6, T = 3: |geomed - honest| = {near:.3f}, |mean - honest| = {far:.3f}, ratio {far / near:.1f}")
    assert far > 10.0 * near


# ----------------------------------------------------------------------------
# the torch engine
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("P", [100, 257, 9216])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 9, 40, 257])
def test_torch_engine_matches_oracle(k, P):
    if k == 257 and P == 9216:
        P = 513   # (the lane sum's second pass needs no large P)
    eng = _engine()
    for n, kind in enumerate(STACKS):
        x = make_stack(kind, np.random.default_rng(1000 * k + P + n), k, P)
        for T, nu in ((0, 1e-6), (1, 1e-6), (3, 1e-6), (2, 1e3)):
            want = oracle_fast(x, T, nu)
            got = _eng_run(eng, x, T, nu)
            assert_same_result(got, want[:2])
            if kind in ("nan", "inf", "ninf"):
                assert got[1][k // 2] == 0.0
            if kind == "allbad":
                assert np.all(got[0].view(np.uint32) == NAN_BITS) and np.all(got[1] == 0.0)


def test_torch_engine_literal_oracle_and_errors():
    eng = _engine()
    x = make_stack("crowd", np.random.default_rng(7), 6, 300)
    for T in (0, 1, 3):
        assert_same_result(_eng_run(eng, x, T, 1e-6), oracle_literal(x, T, 1e-6)[:2])
    for T, nu in [(-1, 1e-6), (65, 1e-6), (1.5, 1e-6), (True, 1e-6), (3, 0.0), (3, -1.0), (3, INF), (3, float("nan")),
                  (3, "x")]:
        with pytest.raises(ValueError):
            eng.geomed_aggregate(torch.from_numpy(x), T, nu)


# ----------------------------------------------------------------------------
# properties of the rule
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 5, 6, 9])
def test_identical_rows_return_the_row(k):
    eng = _engine()
    row = np.random.default_rng(k).normal(size=700).astype(np.float32)
    x = np.tile(row, (k, 1))
    for T in (0, 1, 3, 8):
        for run in (lambda: _eng_run(eng, x, T, 1e-6), lambda: oracle_fast(x, T, 1e-6)[:2]):
            z, w = run()
            assert_same_bits(z, row)
            if k & (k - 1) == 0:   # 1 / k exact in f64: k equal weights add up without rounding
                same_f64_bits(w, np.full(k, 1.0 / k))
            else:   # (at most 16 roundings of 2^-53 each between 1 / nu and w)
                same_f64_bits(w, np.full(k, w[0]))
                assert abs(w[0] - 1.0 / k) <= 16 * 2.0 ** -53 / k


def test_identical_rows_weights_are_one_over_k():
    """T = 0 (beta = 1.0 each, B = k exactly): 1 / k to the bit for every k."""
    for k in (3, 5, 6, 7, 40, 257):
        x = np.tile(np.random.default_rng(k).normal(size=50).astype(np.float32), (k, 1))
        z, w, d = oracle_fast(x, 0, 1e-6)
        same_f64_bits(w, np.full(k, 1.0 / k))
        # (the mean of k equal values in f64, rounded to fp32, is the value)
        assert_same_bits(z, x[0])


def test_single_row_is_returned():
    eng = _engine()
    x = np.random.default_rng(1).normal(size=(1, 513)).astype(np.float32)
    for T in (0, 3):
        z, w = _eng_run(eng, x, T, 1e-6)
        assert_same_bits(z, x[0])
        assert w.tolist() == [1.0]
        d = oracle_fast(x, T, 1e-6)[2]
        assert d[0] == (0.0 if T else oracle_fast(x, 0, 1e-6)[2][0])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_bad_row_has_weight_zero_and_changes_no_bit(bad):
    """A row with one NaN / +inf / -inf at any coordinate has weight exactly 0
    and dist +inf.  Bit for bit the result is the one computed without the
    row: for every row position at T = 0 (beta = 1.0 each: B is exact), and
    for the last row position at every T (its lane adds 0.0 to the lane sum
    and the other rows keep their lanes; in another position the rows after
    it would change lanes, and B its rounding)."""
    eng = _engine()
    rng = np.random.default_rng(11)
    k, P = 6, 600
    clean = make_stack("crowd", rng, k - 1, P)
    for col in (0, 255, 256, 300, P - 1):
        for pos in range(k):
            row = rng.normal(size=P).astype(np.float32)
            row[col] = bad
            x = np.insert(clean, pos, row, axis=0)
            others = [i for i in range(k) if i != pos]
            for T in (0, 1, 3):
                z, w = _eng_run(eng, x, T, 1e-6)
                zo, wo, do = oracle_fast(x, T, 1e-6)
                assert_same_result((z, w), (zo, wo))
                assert w[pos] == 0.0 and do[pos] == INF and np.all(w[others] > 0) and np.all(np.isfinite(do[others]))
                assert not np.isnan(z).any()
                if T == 0 or pos == k - 1:
                    zc, wc, dc = oracle_fast(clean, T, 1e-6)
                    assert_same_bits(z, zc)
                    same_f64_bits(w[others], wc)
                    same_f64_bits(do[others], dc)
                if T == 0:
                    same_f64_bits(w[others], np.full(k - 1, 1.0 / (k - 1)))


def test_all_rows_bad_gives_the_nan_aggregate():
    eng = _engine()
    rng = np.random.default_rng(12)
    for k in (1, 3, 6):
        x = make_stack("allbad", rng, k, 300)
        x[0, 5] = np.inf
        for T in (0, 3):
            z, w = _eng_run(eng, x, T, 1e-6)
            assert np.all(z.view(np.uint32) == NAN_BITS) and np.all(w == 0.0)
            for orc in (oracle_fast, oracle_literal):
                zo, wo, do = orc(x, T, 1e-6)
                assert np.all(zo.view(np.uint32) == NAN_BITS) and np.all(wo == 0.0) and np.all(do == INF)


def test_large_nu_gives_equal_weights():
    eng = _engine()
    x = make_stack("crowd", np.random.default_rng(13), 6, 600)
    z, w = _eng_run(eng, x, 3, 1e6)
    d = oracle_fast(x, 3, 1e6)[2]
    assert np.sqrt(d.max()) < 1e6
    same_f64_bits(w, np.full(6, w[0]))
    assert abs(w[0] - 1.0 / 6) <= 16 * 2.0 ** -53 / 6
    # equal weights: every step is the T = 0 mean up to the weights' rounding
    np.testing.assert_allclose(z, _eng_run(eng, x, 0, 1e-6)[0], rtol=0, atol=1e-6 * np.abs(x).max())


def test_poisoned_row_is_down_weighted():
    for k, floor in ((6, 10.0), (5, 10.0)):
        x = make_stack("crowd", np.random.default_rng(k), k, 9216).astype(np.float64)
        honest = np.delete(x, k // 2, axis=0).mean(0)
        z3, w3, _ = oracle_fast(x.astype(np.float32), 3, 1e-6)
        z8, w8, _ = oracle_fast(x.astype(np.float32), 8, 1e-6)
        far = np.linalg.norm(x.mean(0) - honest)
        assert far > floor * np.linalg.norm(z3 - honest) and np.argmin(w3) == k // 2 == np.argmin(w8)
        assert np.linalg.norm(z8 - honest) <= np.linalg.norm(z3 - honest)


# ----------------------------------------------------------------------------
# configuration, plans, command line
# ----------------------------------------------------------------------------

def test_geomed_check_and_types():
    from fedmse_decentralized_amd.protocol.aggregation import (GEOMED_TYPES, KRUM_TYPES, ROBUST_TYPES, UPDATE_TYPES,
                                                               geomed_check, krum_counts, make_plan, trim_count)

    assert GEOMED_TYPES == ("geomed",) and "geomed" in UPDATE_TYPES
    assert "geomed" not in ROBUST_TYPES and "geomed" not in KRUM_TYPES
    assert geomed_check(3, 1e-6) == (3, 1e-6) and geomed_check(0, 5) == (0, 5.0) and geomed_check(64, 1e3) == (64, 1e3)
    assert geomed_check(np.int64(2), np.float32(0.5)) == (2, 0.5)
    for T, nu in [(-1, 1e-6), (65, 1e-6), (1.0, 1e-6), ("3", 1e-6), (None, 1e-6), (True, 1e-6), (3, 0), (3, -1e-6),
                  (3, INF), (3, float("nan")), (3, None), (3, "tiny"), (3, True)]:
        with pytest.raises(ValueError):
            geomed_check(T, nu)
    with pytest.raises(ValueError):   # not a (source, weight) plan: callers branch before make_plan
        make_plan("geomed", [0, 1, 2], 0)
    with pytest.raises(ValueError):
        trim_count("geomed", 5, 0.2)
    with pytest.raises(ValueError):
        krum_counts("geomed", 5, 0.2)


def test_config_and_cli(capsys):
    import argparse

    import main as driver
    from fedmse_decentralized_amd.config import add_arguments, from_args

    cfg = ExperimentConfig()
    assert cfg.geomed_iters == 3 and cfg.geomed_nu == 1e-6
    p = add_arguments(argparse.ArgumentParser())
    cfg = from_args(p.parse_args(["--update-types", "geomed", "--geomed-iters", "8", "--geomed-nu", "1e-3"]))
    assert cfg.update_types == ["geomed"] and cfg.geomed_iters == 8 and cfg.geomed_nu == 1e-3
    assert from_args(p.parse_args(["--geomed-iters", "0"])).geomed_iters == 0
    for bad in (["--geomed-iters", "65"], ["--geomed-iters", "-1"], ["--geomed-nu", "0"], ["--geomed-nu", "-1"],
                ["--geomed-nu", "inf"], ["--geomed-nu", "nan"]):
        with pytest.raises(ValueError):
            from_args(p.parse_args(bad))
    for bad in (["--geomed-iters", "2.5"], ["--geomed-nu", "small"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    capsys.readouterr()
    for kw in (dict(geomed_iters=65), dict(geomed_iters=1.5), dict(geomed_nu=0.0), dict(geomed_nu=INF)):
        with pytest.raises(ValueError):
            ExperimentConfig(**kw)
    with pytest.raises(SystemExit):
        driver.main(["--help"])
    text = capsys.readouterr().out
    assert "geomed" in text and "--geomed-iters" in text and "--geomed-nu" in text


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
                model_types=["hybrid"], update_types=["geomed"], num_participants=1.0,
                global_early_stop=False, save_checkpoints=False, malicious_clients=[2], malicious_scale=25.0)
    base.update(kw)
    return ExperimentConfig(**base)


def _host_rounds(tmp_path, update_type, rounds=3):
    """The rounds' results and, per aggregating round, (stack, aggregate)."""
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.federation import Federation

    federation._PREP_CACHE.clear()
    fed = Federation(_cfg(tmp_path, update_types=[update_type]), "hybrid", update_type, 0).setup()
    assert fed._fast is None
    aggs = []
    eng = fed.engine
    geomed, wsum = eng.geomed_aggregate, eng.weighted_sum

    def geomed_rec(stack, iters, nu):
        out = geomed(stack, iters, nu)
        aggs.append((stack.clone(), out[0].clone()))
        return out

    def wsum_rec(stack, weights):
        out = wsum(stack, weights)
        aggs.append((stack.clone(), out.clone()))
        return out
    eng.geomed_aggregate, eng.weighted_sum = geomed_rec, wsum_rec
    rs = [fed.run_round() for _ in range(rounds)]
    fed.writer.flush()
    return rs, aggs


def test_host_round_under_poisoning(tmp_path, small_synthetic, caplog):
    """Six clients, all selected, client 2 multiplies its update by 25 in every
    round: the first geomed aggregate lies at least 10 times closer to the mean
    of the five honest models than the plain mean does (the oracle gives about
    70 times at T = 3 on the prototype's geometry), and the poisoned client's
    weight is the smallest in every aggregating round."""
    import logging

    with caplog.at_level(logging.INFO, logger="fedmx"):
        rs, aggs = _host_rounds(tmp_path / "gm", "geomed")
    assert any(r.aggregator is not None for r in rs)
    n_agg = 0
    for r in rs:
        if r.aggregator is None:
            assert r.agg_weights is None
            continue
        n_agg += 1
        w = r.agg_weights
        assert isinstance(w, list) and len(w) == len(r.selected) == 6 and r.agg_kept is None
        assert abs(sum(w) - 1.0) < 1e-12 and all(x > 0 for x in w)
        assert r.selected[int(np.argmin(w))] == 2
    assert sum("Aggregate weights of clients" in rec.getMessage() for rec in caplog.records) == n_agg == len(aggs)
    rs0, aggs0 = _host_rounds(tmp_path / "avg", "avg")
    assert all(r.agg_weights is None for r in rs0)
    assert rs[0].aggregator is not None and rs0[0].aggregator is not None and rs0[0].selected == rs[0].selected
    stack, agg = aggs[0]
    stack0, mean0 = aggs0[0]
    assert torch.equal(stack, stack0)
    # the recorded aggregate is the rule's
    want = oracle_fast(stack.numpy(), 3, 1e-6)
    assert_same_bits(agg.numpy(), want[0])
    same_f64_bits(np.asarray(rs[0].agg_weights), want[1])
    s64 = stack.double().numpy()
    pos = rs[0].selected.index(2)
    honest = np.delete(s64, pos, axis=0).mean(0)
    near = float(np.linalg.norm(agg.double().numpy() - honest))
    far = float(np.linalg.norm(mean0.double().numpy() - honest))
    print(f"first aggregate: |geomed - honest mean| = {near:.4f}, |mean - honest mean| = {far:.4f}, "
          f"ratio {far / near:.1f}")
    assert far >= 10.0 * near


def test_peer_api_aggregates_with_geomed(tmp_path, small_synthetic):
    from fedmse_decentralized_amd.federation import Federation

    fed = Federation(_cfg(tmp_path, malicious_clients=[], geomed_iters=2, geomed_nu=1e-3), "hybrid", "geomed",
                     0).setup()
    peers = fed.peers()
    stack = fed.engine.store.params[:5].clone()
    stack[1] *= 40.0
    fed.engine.store.params[:5].copy_(stack)
    agg = peers[0].aggregate_models(peers[:5])
    want, w, _ = oracle_fast(stack.numpy(), 2, 1e-3)
    assert int(np.argmin(w)) == 1
    assert_same_bits(agg.numpy(), want)
