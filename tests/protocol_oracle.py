"""Host oracles and the case grid of the round-protocol kernel tests
(``test_protocol_kernels.py`` on the CPU, ``test_protocol_kernels_gpu.py`` on
the GPU; kernels in ``ops/csrc/hip/fedmx_protocol.hip``).

* Election: the host protocol functions themselves (``elect_aggregator`` /
  ``elect_majority``) on a noise source replaying the ``[k][k-1]`` voter-major
  table the kernel reads, and a ``OneDraw`` for the fallback.
* Weights and aggregate: the three weight rules and the separately rounded
  fp32 order of ``weighted_sum_kernel``.
* Verification, two tiers.  Both feed ``decide_all``, which runs
  ``Verifier.decide`` / ``ThesisVerifier.decide_losses`` and ``Verifier.apply``
  and builds every buffer the kernels write.  Tier 1 (GPU test file) takes
  its MSE, drift and history norm from kernels that have tests of their own,
  so it is bitwise.  Tier 2 (here) takes them from float64 arithmetic and is
  compared in the decisions.  (Tier 1 uses ``score_reduce``, whose summation
  order differs from the verification kernels'; both sum fp32 SSE rows in
  double, which is exact in any order while the rows of one receiver lie
  within 2^18 of each other -- ``sse_spread_ok`` checks that for the grid.)

The margin rule of tier 2 (``margins``): a decision of the grid may not depend
on rounding.  The project's forward tolerance (``test_forward_rows_matches_torch``)
is rtol 2e-5, atol 1e-5 on a row's SSE, so an MSE can move by
``atol / d_in + rtol * mse`` and ``perf = 1 / (1 + mse)`` by that times
``perf^2``.  The drift is a sum of eight fp32 norms; the kernels round at
most 9 + 6 + 16 times per tensor sum, so 64 fp32 epsilons (``DRIFT_RTOL``)
bound its relative error, and the relative limit's (mode 3) as well.  Every
compared pair -- drift against its limit, ``dperf`` against ``-pthr``, the
thesis rule's new loss against ``old * (1 + thr)`` -- must be at least
``MARGIN_FACTOR`` = 10 times that movement apart.  Excepted by construction,
and checked for exactness instead (``EXACT_KINDS``): the boundary receivers,
whose drift arithmetic is exact in fp32, and the thesis receiver whose own
model is the aggregate (one computation, twice).  A NaN MSE (no rows) and an
SSE beyond the fp32 range (inf in the kernels' number format) decide the
same way at any precision.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from fedmse_decentralized_amd.federation import _TableNoise
from fedmse_decentralized_amd.models.layout import (P_PAD, ModelDims, canonical_to_padded, padded_index,
                                                     padded_to_canonical, segment_ids_padded)
from fedmse_decentralized_amd.models.reference import init_client_params, rowwise_sse
from fedmse_decentralized_amd.protocol.election import OneDraw, elect_aggregator, elect_majority
from fedmse_decentralized_amd.protocol.verification import ThesisVerifier, Verifier, VerifierState

# ---------------------------------------------------------------------------
# election

MODE_MAJORITY, MODE_VOTE_CAP, MODE_FALLBACK = 1, 2, 4
ELECT_KS = (1, 2, 3, 8, 9, 63, 64, 65, 130, 1024)
# scenarios in which no voter finds a candidate, and every majority election,
# are k^2 work on one lane of the serial path (``Election.quadratic``): above
# QUADRATIC_MAX_K the GPU file runs the former one per test and leaves the
# majority elections out
QUADRATIC_MAX_K = 130
ELECT_P = 2052        # aggregate width: a multiple of 4, of neither 256 nor 1024 (a partial last workgroup)


def host_election(selected: Sequence[int], scores: Dict[int, float], counts: Sequence[int], cap: int, mode: int,
                  noise: Sequence[float], vote_cap: float = 0.0, fallback_u: float = 0.0) -> Tuple[int, int]:
    """(aggregator, voter) of the host protocol functions, -1 for None, under
    the kernel's ``mode`` bits."""
    fn = elect_majority if mode & MODE_MAJORITY else elect_aggregator
    res = fn(list(selected), scores, list(counts), cap, _TableNoise([float(u) for u in noise]), log_enabled=False,
             vote_mse_cap=float(vote_cap) if mode & MODE_VOTE_CAP else None,
             fallback_rng=OneDraw(fallback_u) if mode & MODE_FALLBACK else None)
    return (-1 if res.aggregator is None else int(res.aggregator), -1 if res.voter is None else int(res.voter))


def weight_oracle(rule: int, k: int, mses: Optional[Sequence[float]] = None,
                  hw: Optional[Sequence[float]] = None) -> np.ndarray:
    if rule == 0:
        return np.full(k, np.float32(1.0 / float(k)), dtype=np.float32)
    if rule == 1:
        inv = [1.0 / float(m) for m in mses]
        tot = 0.0
        for v in inv:          # float64, selection order
            tot += v
        return np.array([np.float32(v / tot) for v in inv], dtype=np.float32)
    return np.asarray(hw, dtype=np.float32).copy()


def aggregate_oracle(base: torch.Tensor, rows: Sequence[int], weights: np.ndarray) -> torch.Tensor:
    """``acc = v0 * w0; acc = acc + v_j * w_j`` in fp32, each product and sum
    rounded on its own (as ``test_weighted_sum_and_drift`` builds its reference)."""
    w = torch.from_numpy(np.asarray(weights, dtype=np.float32))
    acc = base[int(rows[0])] * w[0]
    for j in range(1, len(rows)):
        acc = acc + base[int(rows[j])] * w[j]
    return acc


class Election(NamedTuple):
    name: str
    mode: int
    counts: np.ndarray          # int32 [N]
    scores: np.ndarray          # float64 [k], selection order
    noise: np.ndarray           # float64 [k * (k - 1)]
    cap: int = 3
    vote_cap: float = 0.0
    fallback_u: float = 0.0
    quadratic: bool = False


class ElectSetup(NamedTuple):
    k: int
    N: int
    sel: np.ndarray             # int32 [k]: a non-identity permutation of ids drawn from N > k clients
    rows: np.ndarray            # int64 [k]: permuted rows of a base with more rows than k, one row repeated
    n_base: int


def elect_setup(k: int) -> ElectSetup:
    rng = np.random.default_rng(1000 + k)
    N = k + 5
    sel = rng.permutation(N)[:k].astype(np.int32)
    if k > 1 and np.array_equal(sel, np.sort(sel)):
        sel = sel[::-1].copy()
    n_base = k + 3
    rows = rng.permutation(n_base)[:k].astype(np.int64)
    if k >= 3:
        rows[k - 1] = rows[0]     # a source row aggregated twice
    return ElectSetup(k, N, sel, rows, n_base)


def election_scenarios(k: int) -> List[Election]:
    """The election cases of one selection size (issue list: modes, caps, vote
    cap, fallback draw, ties, NaN scores)."""
    S = elect_setup(k)
    rng = np.random.default_rng(2000 + k)
    sel, N = S.sel, S.N
    nn = k * (k - 1)
    scores = rng.uniform(0.5, 2.0, size=k)
    noise = rng.uniform(0.0, 1.0, size=nn)
    flat = np.full(nn, 0.5)                   # noise factor exactly 1
    free = np.zeros(N, dtype=np.int32)
    free[sel[::2]] = 1                        # below the cap, not all equal
    full = np.full(N, 3, dtype=np.int32)
    open_ = np.zeros(N, dtype=np.int32)
    quad = k > 1
    out: List[Election] = []
    med = float(np.median(scores))
    for mode in (0, 1, 2, 3, 4, 6, 7):
        out.append(Election(f"open-m{mode}", mode, free, scores, noise, vote_cap=med, fallback_u=0.3,
                            quadratic=bool(mode & 1)))
    second = full.copy()
    second[sel[0]] = 0                        # only the first voter is eligible: the second voter decides
    out.append(Election("second-voter", 0, second, scores, noise))
    out.append(Election("all-capped", 0, full, scores, noise, quadratic=quad))
    out.append(Election("all-capped-fallback", 4, full, scores, noise, fallback_u=0.5, quadratic=quad))
    out.append(Election("all-capped-majority", 1, full, scores, noise, quadratic=True))
    # vote cap: the overall minimum is out (at its aggregation cap), some above the vote cap
    lo = free.copy()
    lo[sel[int(np.argmin(scores))]] = 3
    out.append(Election("votecap-min-out", 2, lo, scores, noise, vote_cap=med))
    out.append(Election("votecap-none", 2, free, scores, noise, vote_cap=0.25, quadratic=quad))
    some = free.copy()
    some[sel[::3]] = 3                        # the fallback draws among the others
    for u in (0.0, 0.5, float(np.nextafter(1.0, 0.0)), 1.0):
        out.append(Election(f"fallback-u{u!r}", 6, some, scores, noise, vote_cap=0.25, fallback_u=u, quadratic=quad))
    out.append(Election("fallback-majority-u1", 7, some, scores, noise, vote_cap=0.25, fallback_u=1.0,
                        quadratic=True))
    if k >= 2:
        # a score exactly on the vote cap (noise factor 1) and every other one above it
        j = k - 1 if k > 2 else 1
        eq = scores + 1.0
        eq[j] = 1.25
        out.append(Election("votecap-equal", 2, free, eq, flat, vote_cap=1.25))
        out.append(Election("votecap-just-below", 2, free, eq, flat, vote_cap=float(np.nextafter(1.25, 0.0)),
                            quadratic=quad))
        # exact ties of the scores, broken by the noise alone
        tie = np.full(k, 0.75)
        out.append(Election("tie-noise", 0, free, tie, noise))
        out.append(Election("tie-noise-majority", 1, free, tie, noise, quadratic=True))
        # exact ties after the noise: the earliest in selection order wins, ballot and tally
        out.append(Election("tie-exact", 0, free, tie, flat))
        out.append(Election("tie-exact-majority", 1, free, tie, flat, quadratic=True))
        two = scores + 1.0
        two[[0, k - 1]] = 0.5
        if k > 2:
            two[k // 2] = 0.5
        out.append(Election("tie-exact-partial", 0, open_, two, flat))
        out.append(Election("tie-exact-partial-majority", 1, open_, two, flat, quadratic=True))
    # NaN scores (diverged clients): first / middle / last candidate, several, all
    for name, idx in (("first", [0]), ("first-cand", [1] if k > 1 else [0]), ("middle", [k // 2]), ("last", [k - 1]),
                      ("several", sorted({0, 1 % k, k // 2, k - 1})), ("all", list(range(k)))):
        s = scores.copy()
        s[idx] = np.nan
        after = (idx[0] + 1) % k
        if after not in idx:
            s[after] = 0.01       # the lowest number right behind a NaN (a plain float sort leaves it there)
        q = quad and name == "all"
        out.append(Election(f"nan-{name}", 0, open_, s, noise))
        out.append(Election(f"nan-{name}-votecap", 2, open_, s, noise, vote_cap=med, quadratic=q))
        out.append(Election(f"nan-{name}-majority", 1, open_, s, noise, quadratic=True))
    return out


def issue_nan_example() -> Election:
    """Scores [9, 1, NaN, 0.5], caps open, voter 0: a plain float sort keeps the
    ballot (1, NaN, 0.5) as it stands and elects client 1; the rule elects 3."""
    return Election("issue-nan", 0, np.zeros(4, dtype=np.int32), np.array([9.0, 1.0, np.nan, 0.5]), np.full(12, 0.5))


def election_truth(S: ElectSetup, e: Election) -> Tuple[int, int]:
    scores = {int(c): float(s) for c, s in zip(S.sel, e.scores)}
    return host_election(S.sel.tolist(), scores, e.counts.tolist(), e.cap, e.mode, e.noise, e.vote_cap, e.fallback_u)


# ---------------------------------------------------------------------------
# verification

FWD_RTOL, FWD_ATOL = 2e-5, 1e-5          # test_forward_rows_matches_torch
DRIFT_RTOL = 64 * 2.0 ** -24
MARGIN_FACTOR = 10.0
FLT_MAX = float(np.finfo(np.float32).max)
VERIFY_MAX_ROWS = 4096
EXACT_KINDS = ("exact3", "exact3_next", "exact12", "t_equal")

CP_SHAPES = [(115, 27, 7), (5, 3, 2), (1, 1, 1)]        # compact forward order
GENERAL_SHAPES = [(120, 30, 10), (127, 31, 15)]         # identity order
ROW_COUNTS = (0, 1, 15, 16, 17, 127, 129, 130, 131, 4095, 4096)
SPLITS = (1, 2, 3, 8, 64)


class VerifySpec(NamedTuple):
    name: str
    dims: Tuple[int, int, int]
    mode: int
    kinds: Tuple[str, ...]      # per hosted client; "agg" marks the aggregator's slot
    rows: Tuple[int, ...]
    start: int = 0
    hosted: bool = True         # False: the aggregator is a client outside [start, start + n_local)
    thr: float = 3.0
    pthr: float = 0.002
    seed: int = 0
    elected: bool = True        # False: state[0] = -1
    launches: int = 1           # 2: the same aggregate arrives again


VERIFY_SPECS: List[VerifySpec] = [
    # mode 0: every receiver state, mixed row counts, hosted and not hosted aggregator
    VerifySpec("m0-default-hosted", (115, 27, 7), 0, ("first", "accept", "agg", "rej_drift", "rej_perf"),
               (17, 4096, 16, 131, 4095), start=7),
    VerifySpec("m0-general-away", (120, 30, 10), 0, ("rej2", "n0_hist", "n0_first", "exact3", "accept"),
               (129, 0, 0, 15, 127), hosted=False, launches=2),
    VerifySpec("m0-small-hosted", (5, 3, 2), 0, ("agg", "exact3_next", "exact12"), (1, 130, 16), start=7),
    VerifySpec("m0-one-away", (1, 1, 1), 0, ("rej_perf",), (17,), hosted=False),
    VerifySpec("m0-wide-away", (127, 31, 15), 0, ("accept", "rej_drift", "first"), (4096, 1, 131), start=7,
               hosted=False),
    VerifySpec("m0-only-aggregator", (115, 27, 7), 0, ("agg",), (16,)),
    VerifySpec("m0-wide-rows", (127, 31, 15), 0, ("rej_perf", "agg", "exact3", "accept", "rej2"),
               (4095, 130, 131, 17, 4096), launches=2),
    # one past each compact boundary with d_in still compact: the launchers must look at all three dimensions
    VerifySpec("m0-boundary-shape", (115, 28, 8), 0, ("accept", "rej_perf", "first"), (17, 130, 16), hosted=False),
    # mode 1: centralised push
    VerifySpec("m1-default-hosted", (115, 27, 7), 1, ("push", "agg", "push"), (17, 16, 0), start=7),
    VerifySpec("m1-general-away", (120, 30, 10), 1, ("push",), (129,), hosted=False),
    # mode 3: relative drift limit
    VerifySpec("m3-default-away", (115, 27, 7), 3, ("accept", "rej_drift", "zero_hist", "hist_eq_agg", "first"),
               (15, 130, 17, 129, 16), hosted=False, thr=0.5),
    VerifySpec("m3-wide-hosted", (127, 31, 15), 3, ("zero_hist", "agg", "accept"), (131, 1, 4096), start=7, thr=0.5),
    VerifySpec("m3-small-away", (5, 3, 2), 3, ("rej_perf", "hist_eq_agg", "n0_hist"), (127, 4095, 0), start=7,
               hosted=False, thr=0.5),
    # mode 2: thesis rule (fused kernel only)
    VerifySpec("m2-default-hosted", (115, 27, 7), 2, ("t_better", "t_worse", "t_inf", "agg", "n0_hist"),
               (131, 17, 16, 15, 0), start=7, thr=0.1),
    VerifySpec("m2-general-boundary", (120, 30, 10), 2, ("t_equal", "t_better", "t_worse"), (129, 4096, 1),
               hosted=False, thr=0.0),
    # nobody elected
    VerifySpec("none-default", (115, 27, 7), 0, ("accept", "first", "rej_drift"), (17, 16, 0), start=7,
               elected=False),
    VerifySpec("none-general-m3", (120, 30, 10), 3, ("accept",), (130,), elected=False, thr=0.5),
]


def spec_by_name(name: str) -> VerifySpec:
    return next(s for s in VERIFY_SPECS if s.name == name)


STATE_F32 = ("params", "anchor", "hist", "eval_params", "best_stage")
STATE_KEYS = STATE_F32 + ("has_hist", "hist_perf", "rejected", "rej_out", "agg_counts")
REJ_SENTINEL = -7.0


class VerifyCase(NamedTuple):
    spec: VerifySpec
    dims: ModelDims
    a: int                      # aggregator's global id, or -1
    N: int
    agg: torch.Tensor           # [P_PAD]
    seg: torch.Tensor           # int32 [P_PAD]
    vrows: Tuple[torch.Tensor, ...]     # [n, 128] per hosted client
    params: torch.Tensor
    anchor: torch.Tensor
    hist: torch.Tensor
    best: torch.Tensor
    has_hist: torch.Tensor      # int32 [n_local]
    hist_perf: torch.Tensor     # float64 [n_local]
    rejected: torch.Tensor      # int32 [n_local]
    rej_out: torch.Tensor       # float64 [N]
    agg_counts: torch.Tensor    # int32 [N]


def _real_pos(dims: ModelDims, tensor: int) -> int:
    idx, segs = padded_index(dims)
    return int(idx[segs[tensor][0]])


def _scaled_delta(g, dims: ModelDims, target: float) -> torch.Tensor:
    """A canonical perturbation whose drift (sum of the eight tensors' norms) is ``target``."""
    d = torch.randn(dims.num_params, generator=g, dtype=torch.float64)
    _, segs = padded_index(dims)
    tot = sum(float(torch.linalg.vector_norm(d[s:e])) for s, e in segs)
    return (d * (target / tot)).to(torch.float32)


def tensor_norm_sum(canon: torch.Tensor, dims: ModelDims) -> float:
    _, segs = padded_index(dims)
    c = canon.double()
    return sum(float(torch.linalg.vector_norm(c[s:e])) for s, e in segs)


@functools.lru_cache(maxsize=None)
def build_case(spec: VerifySpec) -> VerifyCase:
    """The hosted state of one launch, on the CPU (callers must not modify it)."""
    dims = ModelDims(*spec.dims)
    nl = len(spec.kinds)
    g = torch.Generator().manual_seed(77 + spec.seed)
    N = spec.start + nl + 3
    if not spec.elected:
        a = -1
    elif spec.hosted:
        a = spec.start + spec.kinds.index("agg")
    else:
        a = N - 1
    init, _ = init_client_params(2 * nl + 2, 31 + spec.seed, dims)

    def noisy(i, s=0.05):
        return init[i] + s * torch.randn(dims.num_params, generator=g)

    agg_c = noisy(2 * nl)
    p1, p2 = _real_pos(dims, 0), _real_pos(dims, 2)
    agg = canonical_to_padded(agg_c, dims)
    agg[p1], agg[p2] = 0.5, -0.25            # dyadic values: the exact-boundary receivers differ from them exactly
    agg_c = padded_to_canonical(agg, dims)
    agg_norm = tensor_norm_sum(agg_c, dims)
    rel = spec.mode == 3
    params = torch.stack([canonical_to_padded(noisy(i), dims) for i in range(nl)])
    anchor = torch.stack([canonical_to_padded(noisy(nl + i, 0.1), dims) for i in range(nl)])
    best = canonical_to_padded(torch.randn(nl, dims.num_params, generator=g), dims)
    hist = canonical_to_padded(torch.randn(nl, dims.num_params, generator=g) * 0.3, dims)
    has_hist = torch.ones(nl, dtype=torch.int32)
    hist_perf = torch.zeros(nl, dtype=torch.float64)
    rejected = torch.ones(nl, dtype=torch.int32)
    vrows = []
    for i, (kind, n) in enumerate(zip(spec.kinds, spec.rows)):
        x = torch.zeros(n, 128)
        x[:, :dims.d_in] = torch.randn(n, dims.d_in, generator=g)
        near = canonical_to_padded(agg_c + _scaled_delta(g, dims, 0.1 * agg_norm if rel else 1.0), dims)
        far = canonical_to_padded(agg_c + _scaled_delta(g, dims, 2.0 * agg_norm if rel else 9.0), dims)
        if kind in ("agg", "push"):
            hist_perf[i] = 0.3
        elif kind in ("first", "n0_first"):
            has_hist[i] = 0
            hist_perf[i] = 0.77
        elif kind in ("accept", "n0_hist"):
            hist[i] = near
        elif kind == "rej_drift":
            hist[i] = far
            rejected[i] = 0
        elif kind == "rej_perf":
            hist[i] = near
            hist_perf[i] = 0.999
        elif kind == "rej2":
            hist[i] = far
            rejected[i] = 2
        elif kind == "zero_hist":
            hist[i] = 0.0
        elif kind == "hist_eq_agg":
            hist[i] = agg
        elif kind == "exact3":
            hist[i] = agg
            hist[i, p1] = 3.5
        elif kind == "exact3_next":
            hist[i] = agg
            hist[i, p1] = 0.5 + float(np.nextafter(np.float32(3.0), np.float32(4.0)))
            rejected[i] = 0
        elif kind == "exact12":
            hist[i] = agg
            hist[i, p1] = 1.5
            hist[i, p2] = 1.75
        elif kind == "t_better":
            params[i] = canonical_to_padded(4.0 * init[nl + i] + 0.5 * torch.randn(dims.num_params, generator=g), dims)
        elif kind == "t_worse":
            # the receiver's own model reproduces its (nearly constant) rows: zero weights, output bias = the row
            c = torch.randn(dims.d_in, generator=g)
            x[:, :dims.d_in] = c + 0.01 * torch.randn(n, dims.d_in, generator=g)
            own = torch.zeros(dims.num_params)
            own[dims.num_params - dims.d_in:] = c
            params[i] = canonical_to_padded(own, dims)
        elif kind == "t_inf":
            x[:, :dims.d_in] = 1e30      # every row's SSE leaves the fp32 range
        elif kind == "t_equal":
            params[i] = agg
        else:
            raise ValueError(kind)
        vrows.append(x)
    return VerifyCase(spec, dims, a, N, agg, segment_ids_padded(dims), tuple(vrows), params, anchor, hist, best,
                      has_hist, hist_perf, rejected, torch.full((N,), REJ_SENTINEL, dtype=torch.float64),
                      torch.arange(N, dtype=torch.int32) % 3)


def second_aggregate(case: VerifyCase) -> torch.Tensor:
    """Another aggregate for a second launch on the same scratch: within the
    drift limit of the first one, so the launch's decisions keep wide margins."""
    g = torch.Generator().manual_seed(5)
    c = padded_to_canonical(case.agg, case.dims)
    target = 0.1 * tensor_norm_sum(c, case.dims) if case.spec.mode == 3 else 1.0
    return canonical_to_padded(c + _scaled_delta(g, case.dims, target), case.dims)


def verifying(case: VerifyCase, i: int) -> bool:
    return case.a >= 0 and case.spec.mode != 1 and case.spec.start + i != case.a


def decide_all(case: VerifyCase, mse, old_mse, drift, hnorm) -> Tuple[Dict[str, torch.Tensor], List[Optional[bool]]]:
    """Every buffer after one launch, from per-receiver MSE / drift / history
    norm (entries of clients that do not verify are ignored), by the host
    protocol classes; and the decisions."""
    sp = case.spec
    out = {k: getattr(case, k).clone() for k in ("params", "anchor", "hist", "has_hist", "hist_perf", "rejected",
                                                  "rej_out", "agg_counts")}
    oks: List[Optional[bool]] = [None] * len(sp.kinds)
    if case.a >= 0:
        out["agg_counts"][case.a] += 1
        for i in range(len(sp.kinds)):
            c = sp.start + i
            if sp.mode == 1:
                out["params"][i] = case.agg
                out["anchor"][i] = case.agg
                continue
            if c == case.a:
                out["params"][i] = case.agg
                continue
            st = VerifierState(history_version=0 if int(case.has_hist[i]) else None,
                               history_perf=float(case.hist_perf[i]), rejected_updates=int(case.rejected[i]))
            if sp.mode == 2:
                ver = ThesisVerifier(ratio=sp.thr)
                dec = ver.decide_losses(c, st, 1, float(old_mse[i]), float(mse[i]), 0)
            else:
                ver = Verifier(sp.thr, sp.pthr, drift_rel=sp.thr if sp.mode == 3 else 0.0)
                dec = ver.decide(c, st, 1, 1.0 / (1.0 + float(mse[i])), float(drift[i]), 0,
                                 hist_norm=float(hnorm[i]) if sp.mode == 3 else None)
                out["hist"][i] = case.agg
            ver.apply(c, st, dec)
            oks[i] = bool(dec.verified)
            out["has_hist"][i] = 1
            out["hist_perf"][i] = st.history_perf
            out["rejected"][i] = st.rejected_updates
            out["rej_out"][c] = float(st.rejected_updates)
            if dec.verified:
                out["params"][i] = case.agg
                out["anchor"][i] = case.agg
    out["eval_params"] = out["params"].clone()
    out["best_stage"] = case.best.clone()
    return out, oks


def advance(case: VerifyCase, out: Dict[str, torch.Tensor], agg: Optional[torch.Tensor] = None) -> VerifyCase:
    """The case a further launch starts from."""
    return case._replace(agg=case.agg if agg is None else agg,
                         **{k: out[k] for k in ("params", "anchor", "hist", "has_hist", "hist_perf", "rejected",
                                                "rej_out", "agg_counts")})


def _mse64(flat_padded: torch.Tensor, x: torch.Tensor, dims: ModelDims) -> float:
    n = int(x.shape[0])
    if n == 0:
        return float("nan")
    sse, _ = rowwise_sse(padded_to_canonical(flat_padded, dims).double(), x[:, :dims.d_in].double(), dims)
    sse = torch.where(sse > FLT_MAX, torch.full_like(sse, float("inf")), sse)    # the SSE rows are fp32
    return float(sse.sum()) / (float(n) * dims.d_in)


def tier2_inputs(case: VerifyCase):
    """float64 MSE (aggregate; the receiver's own model under the thesis rule),
    drift and history norm of every hosted client."""
    dims, nl = case.dims, len(case.spec.kinds)
    mse = [_mse64(case.agg, case.vrows[i], dims) for i in range(nl)]
    old = [_mse64(case.params[i], case.vrows[i], dims) if case.spec.mode == 2 else 0.0 for i in range(nl)]
    ac = padded_to_canonical(case.agg, dims)
    drift = [tensor_norm_sum(padded_to_canonical(case.hist[i], dims).double() - ac.double(), dims)
             for i in range(nl)]
    hn = [tensor_norm_sum(padded_to_canonical(case.hist[i], dims), dims) for i in range(nl)]
    return mse, old, drift, hn


def tier2(case: VerifyCase):
    return decide_all(case, *tier2_inputs(case))


def margins(case: VerifyCase) -> List[Tuple[int, str, float, float]]:
    """(client slot, compared pair, gap, movement) of every decision of the
    launch that the margin rule covers (module docstring)."""
    sp, d = case.spec, case.dims.d_in
    mse, old, drift, hn = tier2_inputs(case)
    out = []

    def dm(m):
        return FWD_ATOL / d + FWD_RTOL * m

    for i, kind in enumerate(sp.kinds):
        if not verifying(case, i) or kind in EXACT_KINDS:
            continue
        if sp.mode == 2:
            if math.isfinite(mse[i]):
                out.append((i, "loss", abs(mse[i] - old[i] * (1.0 + sp.thr)), dm(mse[i]) + (1.0 + sp.thr) * dm(old[i])))
            continue
        if not int(case.has_hist[i]):
            continue
        limit = sp.thr * hn[i] if sp.mode == 3 else sp.thr
        out.append((i, "drift", abs(drift[i] - limit), DRIFT_RTOL * (drift[i] + limit)))
        if not math.isnan(mse[i]):
            perf = 1.0 / (1.0 + mse[i])
            out.append((i, "perf", abs(perf - float(case.hist_perf[i]) + sp.pthr), dm(mse[i]) * perf * perf))
    return out


def margin_use(case: VerifyCase) -> float:
    """Largest ``MARGIN_FACTOR * movement / gap`` of the launch (<= 1: the rule holds)."""
    use = 0.0
    for _, _, gap, move in margins(case):
        use = max(use, float("inf") if gap == 0.0 and move > 0.0 else (0.0 if move == 0.0 else
                                                                       MARGIN_FACTOR * move / gap))
    return use


def sse_spread_ok(sse: torch.Tensor) -> bool:
    """A double sum of these fp32 rows is exact in any order: 12 bits of
    count + 24 of mantissa + the rows' spread fit 53."""
    s = sse[torch.isfinite(sse) & (sse > 0)]
    return s.numel() == 0 or float(s.max() / s.min()) <= 2.0 ** 17


def launches_of(spec: VerifySpec, tier=tier2):
    """(case, expected buffers, decisions) of each launch of a spec, chained."""
    case = build_case(spec)
    res = []
    for _ in range(spec.launches):
        out, oks = tier(case)
        res.append((case, out, oks))
        case = advance(case, out)
    return res


# what each receiver kind must come to (None: does not verify) -- the grid is
# only worth its name if the constructed states decide as they were built to
EXPECTED_OK = {"agg": None, "push": None, "first": True, "n0_first": True, "accept": True, "rej_drift": False,
               "rej_perf": False, "rej2": False, "n0_hist": False, "zero_hist": False, "hist_eq_agg": True,
               "exact3": True, "exact3_next": False, "exact12": True, "t_better": True, "t_worse": False,
               "t_inf": False, "t_equal": True}


def production_splits(spec: VerifySpec) -> int:
    """The device round's choice: ceil(tiles / 8) forward workgroups per receiver."""
    tiles = max((int(n) + 15) // 16 for n in spec.rows)
    return max(1, min(64, -(-tiles // 8)))


def split_values(spec: VerifySpec) -> List[int]:
    return sorted(set(SPLITS) | {production_splits(spec)})
