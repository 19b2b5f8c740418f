"""The four decision kernels of ``fedmx_protocol.hip`` (``elect_wsum_kernel``,
``decide_adopt_kernel``, ``verify_decide_kernel``, ``verify_split_kernel``)
launched directly from hand-built argument blocks and compared with the host
protocol functions (``tests/protocol_oracle.py``; the grid's CPU half is
``test_protocol_kernels.py``).

* Election and aggregate: selection sizes 1 .. 1024 (float4 / wide aggregate,
  wave / serial election, the wide loop's 64-row chunks, the LDS tables'
  limit), every mode, caps, vote cap, fallback draw, ties, NaN scores, record
  table and failure words against ``elect_aggregator`` / ``elect_majority``;
  weights and aggregate bitwise against the weight and aggregate oracles.
* Verification: the forward plan + ``decide_adopt`` + ``copy2_f64``,
  ``verify_decide`` and ``verify_split`` from deep copies of one hosted
  state; every buffer bitwise equal across the three, bitwise equal to the
  tier-1 oracle (composed from ``forward_rows``, ``score_reduce`` and
  ``param_drift``) and equal to the float64 tier-2 oracle in every decision.

Measured on an MI355X (gfx950), every case passing, each test under 3.5 s:

* Elections: 44 cases at each k in 2 .. 130 (36 at k = 1), 21 at k = 1024
  plus its nine no-vote cases one per test (majority elections stay at
  k <= 130: k^2 work on one lane); 18 distinct (aggregator, voter) outcomes
  at k = 64 .. 130.  The slowest case is k = 1024 (1.0 s for its 21 launches).
* Verification: 17 hosted states (20 launches) on the three paths, 15 of
  them at every split count in {1, 2, 3, 8, 64, production}, three
  back-to-back pairs on one scratch.  Worst tier-2 margin use (ten times
  the tolerance's reach over the gap, <= 1 required): 2.5e-2, a receiver that
  is sent the same aggregate twice (dperf = 0 against pthr = 0.002); 2.0e-4
  over the first launches.
* Bugs found: the NaN election order only (host sort against the kernels'
  scan; one rule now, protocol/election.py).  The three verification paths
  and the tier-1 oracle agreed bitwise at every shape, row count and split
  count from the first run.  Clamping ``row0`` to ``n`` in the split kernel
  is redundant (an unclamped ``row0`` gives ``nr <= 0``, the same idle
  workgroup), so no test can tell it from its absence.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import protocol_oracle as po  # noqa: E402
from fedmse_decentralized_amd.models.layout import P_PAD  # noqa: E402
from fedmse_decentralized_amd.ops import _hip, _hiprt  # noqa: E402

DEV = torch.device("cuda", 0)
W_SENTINEL, OUT_SENTINEL, STATE_SENTINEL, REPORT_SENTINEL = 777.0, -555.0, -9, -2


def _sync():
    _hip.runtime(DEV).sync()
    torch.cuda.synchronize()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---------------------------------------------------------------------------
# election and aggregate

_BASES = {}


def _base(S):
    """[n_base, ELECT_P] source rows of one selection size (host copy, device copy)."""
    if S.k not in _BASES:
        g = torch.Generator().manual_seed(300 + S.k)
        b = torch.randn(S.n_base, po.ELECT_P, generator=g)
        _BASES[S.k] = (b, b.to(DEV))
    return _BASES[S.k]


def _elect(S, e, rule=0, mses=None, hw=None, rec=None, table_rows=None, err=None, err_n=0, err_stride=0,
           expect_error=None):
    """One elect_wsum launch from device-resident inputs; every output starts as a sentinel."""
    _hip.runtime(DEV)
    k, P = S.k, po.ELECT_P
    R = table_rows or S.N
    vec = np.full((R, 4), -1.0)
    for j in range(k):
        ri = int(rec[j]) if rec is not None else int(S.sel[j])
        vec[ri, 0] = e.scores[j]
        vec[ri, 3] = 1.0 if mses is None else mses[j]
    _, base = _base(S)
    keep = dict(sel=_dev(S.sel), vec=_dev(vec), noise=_dev(e.noise if e.noise.size else np.zeros(1)),
                counts=_dev(e.counts), rows=_dev(S.rows),
                weights=torch.full((k + 8,), W_SENTINEL, dtype=torch.float32, device=DEV),
                state=torch.full((4,), STATE_SENTINEL, dtype=torch.int32, device=DEV),
                out=torch.full((P + 64,), OUT_SENTINEL, dtype=torch.float32, device=DEV),
                rec=None if rec is None else _dev(np.asarray(rec, dtype=np.int32)),
                hw=None if hw is None else _dev(np.asarray(hw, dtype=np.float32)),
                err=None if err is None else _dev(np.asarray(err, dtype=np.int32)))
    report = _hiprt.MappedBuffer(64)
    rep = report.view(0, np.int32, 2)
    rep[:] = REPORT_SENTINEL

    def ptr(name):
        return 0 if keep[name] is None else keep[name].data_ptr()

    E = _hip.ElectArgs(sel=ptr("sel"), vec=ptr("vec"), noise=ptr("noise"), agg_counts=ptr("counts"),
                       weights=ptr("weights"), state=ptr("state"), report=report.dev_ptr, k=k, cap=e.cap, rule=rule,
                       mode=e.mode, rec=ptr("rec"), hw=ptr("hw"), vote_cap=float(e.vote_cap),
                       fallback_u=float(e.fallback_u), err=ptr("err"), err_n=err_n, err_stride=err_stride)
    W = _hip.WsumArgs(base=base.data_ptr(), rows=ptr("rows"), weights=ptr("weights"), state=ptr("state"),
                      out=ptr("out"), k=k, P=P)
    torch.cuda.synchronize()
    if expect_error is not None:
        with pytest.raises(RuntimeError, match=expect_error):
            _hip.elect_wsum(E, W, DEV)
    else:
        _hip.elect_wsum(E, W, DEV)
    _sync()
    res = dict(weights=keep["weights"].cpu().numpy(), state=keep["state"].cpu().tolist(), out=keep["out"].cpu(),
               report=rep.tolist(), counts=keep["counts"].cpu().numpy())
    del keep, report
    return res


def _assert_untouched(res, name):
    assert (res["weights"] == np.float32(W_SENTINEL)).all(), name
    assert bool((res["out"] == OUT_SENTINEL).all()), name


def _assert_elected(S, e, res, truth, weights, agg_ref):
    agg, voter = truth
    name = f"k={S.k} {e.name}"
    assert res["state"] == [agg, voter, STATE_SENTINEL, STATE_SENTINEL], name
    assert res["report"] == [agg, voter], name
    assert np.array_equal(res["counts"], e.counts), name      # the cap count is bumped by the verification kernel
    if agg < 0:
        _assert_untouched(res, name)
        return
    assert np.array_equal(res["weights"][:S.k].view(np.int32), weights.view(np.int32)), name
    assert (res["weights"][S.k:] == np.float32(W_SENTINEL)).all(), name
    assert torch.equal(res["out"][:po.ELECT_P], agg_ref), name
    assert bool((res["out"][po.ELECT_P:] == OUT_SENTINEL).all()), name


@pytest.mark.parametrize("k", po.ELECT_KS)
def test_election_and_mean_aggregate_match_host(k):
    S = po.elect_setup(k)
    w = po.weight_oracle(0, k)
    ref = po.aggregate_oracle(_base(S)[0], S.rows, w)
    ran, outcomes = 0, set()
    for e in po.election_scenarios(k):
        if e.quadratic and k > po.QUADRATIC_MAX_K:
            continue
        truth = po.election_truth(S, e)
        _assert_elected(S, e, _elect(S, e), truth, w, ref)
        outcomes.add(truth)
        ran += 1
    print(f"k={k}: {ran} elections, {len(outcomes)} distinct outcomes")
    assert ran >= 20 and (k == 1 or len(outcomes) > 3)


# At the tables' limit an election in which no voter finds a candidate is k^2
# work on one lane (about a second): one case each.  Majority elections stay
# at k <= QUADRATIC_MAX_K.
NO_VOTE_1024 = [e.name for e in po.election_scenarios(1024) if e.quadratic and not e.mode & 1]


@pytest.mark.parametrize("name", NO_VOTE_1024)
def test_election_without_a_vote_at_the_table_limit(name):
    S = po.elect_setup(1024)
    e = next(x for x in po.election_scenarios(1024) if x.name == name)
    w = po.weight_oracle(0, 1024)
    _assert_elected(S, e, _elect(S, e), po.election_truth(S, e), w, po.aggregate_oracle(_base(S)[0], S.rows, w))


def test_issue_nan_example_elects_the_lowest_number():
    S = po.ElectSetup(4, 4, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int64), 4)
    e = po.issue_nan_example()
    assert po.election_truth(S, e) == (3, 0)
    res = _elect(S, e)
    assert res["state"][:2] == [3, 0] and res["report"] == [3, 0]


@pytest.mark.parametrize("k", po.ELECT_KS)
def test_weight_rules_and_aggregate_bitwise(k):
    S = po.elect_setup(k)
    rng = np.random.default_rng(400 + k)
    e = po.election_scenarios(k)[0]._replace(mode=4, fallback_u=0.6)     # k = 1 elects through the fallback
    truth = po.election_truth(S, e)
    assert truth[0] >= 0
    mses = 10.0 ** rng.uniform(-4.0, 2.0, size=k)
    mses[k - 1] = 1e2
    mses[0] = 1e-4
    hw = rng.uniform(0.1, 1.0, size=k).astype(np.float32)
    hw /= hw.sum()
    for rule in (1, 2):
        w = po.weight_oracle(rule, k, mses=mses, hw=hw)
        ref = po.aggregate_oracle(_base(S)[0], S.rows, w)
        _assert_elected(S, e, _elect(S, e, rule=rule, mses=mses, hw=hw), truth, w, ref)


@pytest.mark.parametrize("k", [3, 9, 64, 65])
def test_record_table_equals_records_by_client_id(k):
    S = po.elect_setup(k)
    rng = np.random.default_rng(500 + k)
    R = 2 * S.N + 3
    rec = rng.permutation(R)[:k].astype(np.int32)
    mses = 10.0 ** rng.uniform(-4.0, 2.0, size=k)
    w = po.weight_oracle(1, k, mses=mses)
    ref = po.aggregate_oracle(_base(S)[0], S.rows, w)
    for e in po.election_scenarios(k):
        if e.name not in ("open-m0", "open-m3", "open-m7", "votecap-min-out", "fallback-u0.5", "nan-middle",
                          "tie-noise"):
            continue
        truth = po.election_truth(S, e)
        by_id = _elect(S, e, rule=1, mses=mses)
        by_rec = _elect(S, e, rule=1, mses=mses, rec=rec, table_rows=R)
        _assert_elected(S, e, by_rec, truth, w, ref)
        assert by_id["state"] == by_rec["state"] and by_id["report"] == by_rec["report"]
        assert np.array_equal(by_id["weights"], by_rec["weights"]) and torch.equal(by_id["out"], by_rec["out"])


@pytest.mark.parametrize("k", [3, 65])
@pytest.mark.parametrize("err_n,err_stride", [(1, 0), (3, 1), (3, 7)])
def test_training_failure_word_stops_the_round(k, err_n, err_stride):
    S = po.elect_setup(k)
    e = po.election_scenarios(k)[0]
    truth = po.election_truth(S, e)
    w = po.weight_oracle(0, k)
    ref = po.aggregate_oracle(_base(S)[0], S.rows, w)
    size = (err_n - 1) * err_stride + 1
    clean = np.zeros(size, dtype=np.int32)
    _assert_elected(S, e, _elect(S, e, err=clean, err_n=err_n, err_stride=err_stride), truth, w, ref)
    for r in sorted({0, err_n // 2, err_n - 1}):
        err = clean.copy()
        err[r * err_stride] = 1 << r
        res = _elect(S, e, err=err, err_n=err_n, err_stride=err_stride)
        assert res["state"][0] == -1 and res["state"][2:] == [STATE_SENTINEL] * 2
        assert res["report"][0] == _hip.ELECT_TRAIN_FAILED == -3
        _assert_untouched(res, f"k={k} word {r}")


def test_selection_beyond_the_tables_is_refused():
    S = po.elect_setup(1025)
    e = po.election_scenarios(1025)[0]
    res = _elect(S, e, expect_error=r"code -1")
    assert res["state"] == [STATE_SENTINEL] * 4 and res["report"] == [REPORT_SENTINEL] * 2
    _assert_untouched(res, "k=1025")


# ---------------------------------------------------------------------------
# verification: three kernels, one truth

class Hosted:
    """A deep copy of a case's hosted state on the device."""

    def __init__(self, case):
        _hip.runtime(DEV)
        self.case = case
        sp = case.spec
        for name in ("params", "anchor", "hist", "best", "has_hist", "hist_perf", "rejected", "rej_out", "agg_counts",
                     "agg", "seg"):
            setattr(self, name, getattr(case, name).clone().to(DEV))
        self.vrows = [x.to(DEV) if x.shape[0] else torch.zeros(1, 128, device=DEV) for x in case.vrows]
        self.vx = torch.tensor([x.data_ptr() for x in self.vrows], dtype=torch.int64, device=DEV)
        self.vn = torch.tensor(list(sp.rows), dtype=torch.int32, device=DEV)
        self.eval_params = torch.full_like(self.params, OUT_SENTINEL)
        self.best_stage = torch.full_like(self.params, OUT_SENTINEL)
        self.state = torch.tensor([case.a, -1, STATE_SENTINEL, STATE_SENTINEL], dtype=torch.int32, device=DEV)
        self.nl = len(sp.kinds)
        torch.cuda.synchronize()

    def decide_args(self, sse=0, sse_off=0, sse_n=0):
        sp = self.case.spec
        return _hip.DecideArgs(params=self.params.data_ptr(), anchor=self.anchor.data_ptr(), hist=self.hist.data_ptr(),
                               agg=self.agg.data_ptr(), state=self.state.data_ptr(), sse=sse, sse_off=sse_off,
                               sse_n=sse_n, seg=self.seg.data_ptr(), agg_counts=self.agg_counts.data_ptr(),
                               has_hist=self.has_hist.data_ptr(), hist_perf=self.hist_perf.data_ptr(),
                               rejected=self.rejected.data_ptr(), rej_out=self.rej_out.data_ptr(), thr=float(sp.thr),
                               pthr=float(sp.pthr), start=sp.start, n_local=self.nl, P=P_PAD,
                               d_in=self.case.dims.d_in, mode=sp.mode, pad=0)

    def verify_args(self):
        return _hip.VerifyArgs(D=self.decide_args(), vx=self.vx.data_ptr(), vn=self.vn.data_ptr(),
                               eval_params=self.eval_params.data_ptr(), best_stage=self.best_stage.data_ptr(),
                               best=self.best.data_ptr(), latent=self.case.dims.latent, hidden=self.case.dims.hidden)

    def read(self):
        _sync()
        return {k: getattr(self, k).cpu() for k in po.STATE_KEYS}

    # -- the three paths ------------------------------------------------------
    def run_separate(self):
        """The forward plan, decide_adopt and the snapshot copy (the unfused round)."""
        rows = self.case.spec.rows
        live = [i for i, n in enumerate(rows) if n > 0]
        off = np.zeros(self.nl, dtype=np.int32)
        sse_ptr = self.vx.data_ptr()     # never read when no receiver has rows
        if live:
            plan = _hip.FwdPlan(self.agg.unsqueeze(0), [(0, self.vrows[i]) for i in live], self.case.dims,
                                want_sse=True, want_latent=False)
            plan.run()
            off[live] = plan.offs
            sse_ptr = plan.sse.data_ptr()
        off_t, n_t = _dev(off), self.vn
        torch.cuda.synchronize()
        _hip.decide_adopt(self.decide_args(sse_ptr, off_t.data_ptr(), n_t.data_ptr()), DEV)
        nd = self.params.numel() // 2
        _hip.copy2_f64(self.eval_params.data_ptr(), self.params.data_ptr(), nd, self.best_stage.data_ptr(),
                       self.best.data_ptr(), nd, DEV)
        _sync()

    def run_fused(self):
        _hip.verify_decide(self.verify_args(), DEV)
        _sync()

    def split_scratch(self):
        """SSE rows and drift granules as NaN bit patterns: nothing stale may be read."""
        if not hasattr(self, "scratch"):
            self.scratch = (torch.full((self.nl, _hip.VERIFY_MAX_ROWS), float("nan"), device=DEV),
                            torch.full((self.nl,), 0x7FC000007FC00000, dtype=torch.int64, device=DEV),
                            torch.zeros(self.nl, dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
        return self.scratch

    def run_split(self, splits, done=None, seq=0):
        sse, drift, count = self.split_scratch()
        s = _hip.VerifySplitArgs(sse=sse.data_ptr(), drift=drift.data_ptr(), count=count.data_ptr(), splits=splits,
                                 pad=0, done=0 if done is None else done.data_ptr(), seq=seq, pad2=0)
        _hip.verify_split(self.verify_args(), s, DEV)
        _sync()
        assert count.cpu().tolist() == [0] * self.nl


def _same(got, exp, what, keys=po.STATE_KEYS):
    for k in keys:
        g, x = got[k], exp[k]
        if g.dtype == torch.float64:
            assert np.array_equal(g.numpy(), x.numpy(), equal_nan=True), (what, k, g, x)
        else:
            assert torch.equal(g, x), (what, k)


def _tier1_inputs(case):
    """MSE, drift and history norm from the kernels that have tests of their
    own, on a fresh upload of the case."""
    h = Hosted(case)
    dims, nl = case.dims, h.nl
    live = [i for i, n in enumerate(case.spec.rows) if n > 0]
    nan = float("nan")
    mse, old = [nan] * nl, [nan if case.spec.mode == 2 else 0.0] * nl
    views = []
    if live:
        ns = [case.spec.rows[i] for i in live]
        sse, _ = _hip.forward_rows(h.agg.unsqueeze(0), [(0, h.vrows[i]) for i in live], dims, True, False)
        views.append((mse, _hip.score_reduce(sse, ns, dims.d_in)))
        if case.spec.mode == 2:
            sse_o, _ = _hip.forward_rows(h.params, [(i, h.vrows[i]) for i in live], dims, True, False)
            views.append((old, _hip.score_reduce(sse_o, ns, dims.d_in)))
    drift = _hip.param_drift(h.hist, h.agg, h.seg)
    hn = _hip.param_drift(h.hist, torch.zeros_like(h.agg), h.seg)
    _sync()
    for dst, view in views:
        for j, i in enumerate(live):
            dst[i] = float(view[j, 1])
    return mse, old, [float(v) for v in drift.cpu()], [float(v) for v in hn.cpu()]


def _tier1(case):
    return po.decide_all(case, *_tier1_inputs(case))


SPEC_IDS = [s.name for s in po.VERIFY_SPECS]


@pytest.mark.parametrize("spec", po.VERIFY_SPECS, ids=SPEC_IDS)
def test_three_verification_kernels_one_truth(spec):
    chain1 = po.launches_of(spec, tier=_tier1)
    chain2 = po.launches_of(spec)
    first = chain1[0][0]
    production = po.production_splits(spec)
    if spec.mode == 2:
        paths = {"fused": Hosted(first)}
        refused = Hosted(first)
        before = refused.read()
        with pytest.raises(RuntimeError, match=r"code -5"):
            refused.run_split(production)
        _same(refused.read(), before, "mode 2 refused by verify_split")
    else:
        paths = {"separate": Hosted(first), "fused": Hosted(first), "split": Hosted(first)}
    for li, ((case, exp1, oks1), (case2, exp2, oks2)) in enumerate(zip(chain1, chain2)):
        assert oks1 == oks2, (spec.name, li)                     # tier 1 and tier 2 decide alike
        _same(exp1, exp2, "tier 1 vs tier 2", keys=po.STATE_F32 + ("has_hist", "rejected", "rej_out", "agg_counts"))
        use = po.margin_use(case2)
        print(f"{spec.name} launch {li}: decisions {oks1}, tier-2 margin use {use:.3e}")
        got = {}
        for name, h in paths.items():
            {"separate": h.run_separate, "fused": h.run_fused, "split": lambda: h.run_split(production)}[name]()
            got[name] = h.read()
            _same(got[name], exp1, f"{spec.name} launch {li} {name} vs tier 1")
        for name in got:
            _same(got[name], got["fused"], f"{spec.name} launch {li} {name} vs fused")
        delta = (got["fused"]["agg_counts"] - case.agg_counts).tolist()
        assert delta == [1 if c == case.a else 0 for c in range(case.N)]


SPLIT_SPECS = [s for s in po.VERIFY_SPECS if s.mode != 2]


@pytest.mark.parametrize("spec", SPLIT_SPECS, ids=[s.name for s in SPLIT_SPECS])
def test_split_verification_at_every_split_count(spec):
    """1 .. 64 forward workgroups per receiver (more splits than tiles: idle
    workgroups) and the production value, on NaN-filled scratch."""
    case = po.build_case(spec)
    exp, _ = _tier1(case)
    for splits in po.split_values(spec):
        h = Hosted(case)
        h.run_split(splits)
        _same(h.read(), exp, f"{spec.name} splits={splits}")


@pytest.mark.parametrize("name,with_done", [("m0-default-hosted", True), ("m3-default-away", True),
                                            ("m0-general-away", False)])
def test_split_verification_back_to_back_on_one_scratch(name, with_done):
    case = po.build_case(po.spec_by_name(name))
    h = Hosted(case)
    done = torch.zeros(2, dtype=torch.int32, device=DEV) if with_done else None
    agg2 = po.second_aggregate(case)
    for seq, agg in ((1, None), (0xFFFFFFFF, agg2)):
        if agg is not None:
            case = po.advance(case, exp, agg)
            h.agg.copy_(agg.to(DEV))
            h.case = case
            torch.cuda.synchronize()
        exp, _ = _tier1(case)
        h.run_split(3, done=done, seq=seq)       # (run_split checks the arrival counters are back at zero)
        _same(h.read(), exp, f"{name} seq={seq:#x}")
        if done is not None:
            assert done.cpu().numpy().view(np.uint32).tolist() == [0, seq]
