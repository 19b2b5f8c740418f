"""The round-protocol kernel tests' CPU half: the case grid of
``tests/protocol_oracle.py`` is decisive (every verification decision of the
float64 oracle equals the one an fp32 ``TorchEngine`` forward gives, with the
margin rule stated there and no case left out), the host election follows the
NaN rule the kernels implement, and the ctypes argument blocks have the sizes
the kernels assert.  The GPU half is ``test_protocol_kernels_gpu.py``.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import protocol_oracle as po  # noqa: E402
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine  # noqa: E402
from fedmse_decentralized_amd.ops import _hip  # noqa: E402

SPEC_IDS = [s.name for s in po.VERIFY_SPECS]


def test_argument_block_sizes():
    """The kernels' static_asserts (fedmx_protocol.hip)."""
    got = [ctypes.sizeof(t) for t in (_hip.ElectArgs, _hip.WsumArgs, _hip.DecideArgs, _hip.VerifyArgs,
                                      _hip.VerifySplitArgs)]
    assert got == [120, 48, 152, 200, 48]


def test_grid_covers_the_issue_list():
    specs = po.VERIFY_SPECS
    assert {s.dims for s in specs} == set(po.CP_SHAPES + po.GENERAL_SHAPES) | {(115, 28, 8)}
    assert {n for s in specs for n in s.rows} == set(po.ROW_COUNTS)
    assert max(n for s in specs for n in s.rows) == po.VERIFY_MAX_ROWS == _hip.VERIFY_MAX_ROWS
    assert {len(s.kinds) for s in specs} == {1, 3, 5}
    assert {s.start for s in specs} == {0, 7}
    for mode in (0, 1, 3):
        assert {s.hosted for s in specs if s.mode == mode and s.elected} == {True, False}, mode
        assert {s.dims in po.CP_SHAPES for s in specs if s.mode == mode} == {True, False}, mode
    assert {s.dims in po.CP_SHAPES for s in specs if s.mode == 2} == {True, False}
    kinds = {k for s in specs for k in s.kinds}
    assert kinds == set(po.EXPECTED_OK)
    # every receiver state of mode 0 in one launch where n_local allows: the two five-client launches hold them all
    m0 = {k for s in specs if s.mode == 0 and len(s.kinds) == 5 for k in s.kinds}
    assert {"first", "accept", "rej_drift", "rej_perf", "rej2", "n0_hist", "n0_first", "agg"} <= m0
    for s in specs:
        assert len(s.kinds) == len(s.rows)
        assert ("agg" in s.kinds) == (s.hosted and s.elected and s.mode != 1 or s.mode == 1 and s.hosted), s.name


@pytest.mark.parametrize("spec", po.VERIFY_SPECS, ids=SPEC_IDS)
def test_receivers_decide_as_they_were_built(spec):
    case, out, oks = po.launches_of(spec)[0]
    want = [po.EXPECTED_OK[k] if po.verifying(case, i) else None for i, k in enumerate(spec.kinds)]
    assert oks == want
    # the aggregation-cap count rises by exactly one, at the aggregator
    delta = (out["agg_counts"] - case.agg_counts).tolist()
    assert delta == [1 if c == case.a else 0 for c in range(case.N)]


def _fp32_inputs(case):
    """MSE / drift / history norm as an fp32 TorchEngine computes them."""
    eng = TorchEngine(case.dims, torch.device("cpu"))
    nl = len(case.spec.kinds)
    d = case.dims.d_in

    def mse_of(p, x):
        if x.shape[0] == 0:
            return float("nan"), None
        (sse,), _ = eng.forward_rows(p.unsqueeze(0), [(0, x)])
        return float(sse.double().sum()) / (float(x.shape[0]) * d), sse

    new = [mse_of(case.agg, x) for x in case.vrows]
    old = [mse_of(case.params[i], case.vrows[i])[0] if case.spec.mode == 2 else 0.0 for i in range(nl)]
    drift = eng.param_drift(case.hist, case.agg).tolist()
    hn = eng.param_drift(case.hist, torch.zeros_like(case.agg)).tolist()
    return [m for m, _ in new], old, drift, hn, [s for _, s in new]


@pytest.mark.parametrize("spec", po.VERIFY_SPECS, ids=SPEC_IDS)
def test_tier2_decisions_equal_fp32_engine_and_margins_hold(spec):
    """The margin rule (protocol_oracle docstring), with zero cases left out:
    every compared pair of every launch of the grid is at least ten times the
    forward tolerance's (and fp32 drift rounding's) reach apart, so the fp64
    decision is THE decision, and an fp32 engine takes it too."""
    for case, out, oks in po.launches_of(spec):
        mse, old, drift, hn, sses = _fp32_inputs(case)
        out32, oks32 = po.decide_all(case, mse, old, drift, hn)
        assert oks32 == oks
        for k in po.STATE_F32 + ("has_hist", "rejected", "agg_counts"):
            assert torch.equal(out32[k], out[k]), k
        use = po.margin_use(case)
        print(f"{spec.name}: margin use {use:.3e} over {len(po.margins(case))} compared pairs")
        assert use <= 1.0, po.margins(case)
        for s in sses:
            assert s is None or po.sse_spread_ok(s)
    # a second launch with another aggregate (the split kernel's back-to-back test) keeps the rule
    if spec.mode != 2 and spec.elected:
        case, out, _ = po.launches_of(spec)[0]
        nxt = po.advance(case, out, po.second_aggregate(case))
        assert po.margin_use(nxt) <= 1.0, po.margins(nxt)
        assert po.decide_all(nxt, *_fp32_inputs(nxt)[:4])[1] == po.tier2(nxt)[1]


def test_exact_boundary_receivers_are_exact_in_fp32():
    """The receivers the margin rule excepts: their drift is the same number
    in fp32 and fp64 (no rounding to argue about), on the stated side of 3.0."""
    f32 = np.float32
    seen = set()
    for spec in po.VERIFY_SPECS:
        case = po.build_case(spec)
        _, _, drift64, _ = po.tier2_inputs(case)
        for i, kind in enumerate(spec.kinds):
            if kind == "t_equal":
                assert torch.equal(case.params[i], case.agg) and spec.thr == 0.0
                seen.add(kind)
            if not kind.startswith("exact"):
                continue
            seen.add(kind)
            assert spec.mode == 0 and spec.thr == 3.0
            diff = (case.hist[i] - case.agg).numpy()
            nz = np.flatnonzero(diff)
            segs = case.seg.numpy()[nz]
            assert len(set(segs.tolist())) == len(nz) and (segs >= 0).all()      # one element per tensor
            # the kernels' arithmetic on these elements, op by op in fp32
            d32 = f32(0.0)
            for v in diff[nz]:
                d32 = f32(d32 + f32(np.sqrt(f32(f32(v) * f32(v)))))
            assert float(d32) == float(f32(drift64[i]))
            assert (float(d32) <= 3.0) == (drift64[i] <= 3.0) == po.EXPECTED_OK[kind]
            if kind == "exact3_next":
                assert float(d32) == float(np.nextafter(f32(3.0), f32(4.0)))
            else:
                assert float(d32) == 3.0 == drift64[i]
    assert seen == set(po.EXPECTED_OK) & set(po.EXACT_KINDS)


# -- election -----------------------------------------------------------------

def _scan_election(S, e):
    """The kernels' election, transcribed: per voter a first-minimum scan in
    selection order under ``score_before`` (NaN after every number)."""
    k, sel = S.k, S.sel.tolist()

    def before(s, best):
        return s < best or (best != best and s == s)

    agg, voter = -1, -1
    votes = [0] * k
    for vi in range(k):
        if agg >= 0 and not e.mode & 1:
            break
        best, best_s = -1, 0.0
        for ci in range(k):
            if ci == vi:
                continue
            sc = float(e.scores[ci]) * (1.0 + (float(e.noise[vi * (k - 1) + ci - (ci > vi)]) - 0.5) * 0.0002)
            if e.counts[sel[ci]] < e.cap and (not e.mode & 2 or sc <= e.vote_cap) and (best < 0 or before(sc, best_s)):
                best, best_s = ci, sc
        if best >= 0:
            agg, voter = sel[best], sel[vi]
            votes[best] += 1
    if e.mode & 1:
        top = max(range(k), key=lambda ci: (votes[ci], -ci))
        agg, voter = (sel[top] if votes[top] > 0 else -1), -1
    if agg < 0 and e.mode & 4:
        elig = [c for c in sel if e.counts[c] < e.cap]
        if elig:
            agg, voter = elig[min(int(e.fallback_u * len(elig)), len(elig) - 1)], -1
    return agg, voter


def test_nan_scores_order_after_every_number():
    """The rule of protocol/election.py: NaN after every number, ties in
    selection order.  The issue's example elected client 1 under a plain
    float sort; the rule elects client 3."""
    S = po.ElectSetup(4, 4, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int64), 4)
    assert po.election_truth(S, po.issue_nan_example()) == (3, 0)
    nan = float("nan")
    flat = [0.5] * 12
    el = lambda scores, counts=(0, 0, 0, 0), mode=0, cap=0.0: po.host_election(
        [0, 1, 2, 3], dict(enumerate(scores)), list(counts), 3, mode, flat, cap)
    assert el([1.0, nan, 2.0, 3.0]) == (2, 0)            # NaN first candidate
    assert el([1.0, 2.0, 3.0, nan]) == (1, 0)            # NaN last
    assert el([1.0, nan, nan, nan]) == (1, 0)            # only NaN: the earliest in selection order
    assert el([nan, nan, nan, nan]) == (1, 0)
    assert el([1.0, nan, 2.0, 3.0], counts=(0, 0, 3, 3)) == (1, 0)     # the numbers are capped: NaN is voted for
    assert el([1.0, nan, nan, nan], mode=2, cap=5.0) == (0, 1)         # never under a vote cap; voter 1 finds 0
    assert el([nan, nan, nan, nan], mode=2, cap=5.0) == (-1, -1)
    assert el([1.0, nan, 0.5, 0.5]) == (2, 0)            # exact tie: selection order
    assert el([9.0, 1.0, nan, 0.5], mode=1) == (3, -1)   # majority: every ballot under the same rule


@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 65])
def test_host_election_equals_first_minimum_scan(k):
    """The host functions and the scan the kernels run agree on every election
    case of the grid (what the GPU file then checks on the device)."""
    S = po.elect_setup(k)
    for e in po.election_scenarios(k):
        if e.quadratic and k > 9:
            continue
        assert po.election_truth(S, e) == _scan_election(S, e), e.name


def test_election_scenarios_reach_every_outcome():
    S = po.elect_setup(9)
    res = {e.name: po.election_truth(S, e) for e in po.election_scenarios(9)}
    assert res["second-voter"] == (int(S.sel[0]), int(S.sel[1]))
    assert res["all-capped"] == res["all-capped-fallback"] == res["votecap-none"] == (-1, -1)
    assert res["votecap-equal"] == (int(S.sel[8]), int(S.sel[0]))
    assert res["votecap-just-below"] == (-1, -1)
    assert res["tie-exact"] == (int(S.sel[1]), int(S.sel[0]))
    assert res["tie-exact-partial"][0] == int(S.sel[4])       # voter 0 is a tied one itself: the next tied in order
    e = po.election_scenarios(9)
    elig = [int(c) for c in S.sel if next(x for x in e if x.name == "votecap-none").counts[c] < 3]
    some = [int(c) for c in S.sel if next(x for x in e if x.name.startswith("fallback-u0.0")).counts[c] < 3]
    assert len(elig) == 9 and 1 < len(some) < 9
    assert res["fallback-u0.0"] == (some[0], -1) and res["fallback-u1.0"] == (some[-1], -1)
    assert res[f"fallback-u{float(np.nextafter(1.0, 0.0))!r}"] == (some[-1], -1)
    assert res["fallback-u0.5"] == (some[len(some) // 2], -1)
    assert len({v for n, v in res.items() if n.startswith("nan-")}) > 2


def test_weight_oracle_rules():
    assert po.weight_oracle(0, 3).tolist() == [float(np.float32(1.0 / 3.0))] * 3
    w = po.weight_oracle(1, 3, mses=[1e-4, 1.0, 1e2])
    inv = np.array([1e4, 1.0, 1e-2])
    np.testing.assert_array_equal(w, (inv / ((inv[0] + inv[1]) + inv[2])).astype(np.float32))
    base = torch.arange(12, dtype=torch.float32).reshape(3, 4) + 0.1
    ref = (base[2] * w[0] + base[0] * w[1]) + base[2] * w[2]
    assert torch.equal(po.aggregate_oracle(base, [2, 0, 2], w), ref)
    assert math.isclose(float(w.sum()), 1.0, rel_tol=1e-6)
