"""Training launches that start from carried-over Adam state (non-zero
moments, ``adam_step > 0``, moved parameters) and non-default ``lr`` / betas,
against the fp64 oracle of ``tests/train_state_oracle.py`` (run with
``pytest -m gpu`` on an MI355X).

Every launch of the other kernel tests starts from ``setup()``: zero moments,
which the scaled-moment load (``m / (1-b1)``, ``v / (1-b2)``) multiplies to
zero again, and step 0, where ``pow(beta, step)`` is 1.  Here launch 1 runs on
the fp64 oracle, its state rounded to fp32 is planted into the kernel's store
and launch 2 is compared: a wrong load or write-back scale, a tile whose role
forgets it, a step that is not read or a snapshot taken in the scaled domain
shows in ``adam_m`` / ``adam_v`` / ``params`` / ``best`` of that launch.
Variants (``train_state_oracle.VARIANTS``): ``carried`` the launch-1 state as
is; ``step1e5`` the same with ``adam_step = 100000``; ``lr1e-2`` / ``lr1e-4``;
``b.5/.9`` (beta1 0.5, beta2 0.9, eps 1e-4) and ``b0/.99`` (beta1 0), whose
moment scales are 2 / 10 and 1 / 100 instead of 10 / 1000.  Families as in
``test_train_shapes_gpu.py``.  ``tests/test_train_state.py`` checks on the CPU
that every case's decisions are clear and that the fp32 oracle alone uses at
most half of each tolerance.

Baseline for later tolerance changes: the largest distance to the fp64 oracle
over a (shape, family, variant)'s cases, as absolute difference and, in
brackets, as the fraction of ``atol + rtol * |ref|`` used (``oracle_f64.usage``;
1 would fail).  The kernel rows (hw, hw_sync, c4, general) were measured on
an MI355X, the fp32 rows are the fp32 oracle on the CPU.  ``launch1`` /
``launch2`` are the two-launch end-to-end runs.  The tests print the same
figures per case (``DIST`` lines, ``pytest -s``).

  shape      family   variant  params           tracking         adam_m           adam_v
  120/30/10  general  carried  1.1e-07 (0.001)  6.9e-07 (0.001)  9.6e-07 (0.377)  2.3e-08 (0.002)
  120/30/10  fp32     carried  1.1e-07 (0.002)  8.6e-07 (0.001)  7.6e-07 (0.182)  7.9e-09 (0.003)
  120/30/10  general  step1e5  1.1e-07 (0.001)  4.8e-07 (0.001)  2.7e-07 (0.056)  9.2e-09 (0.002)
  120/30/10  fp32     step1e5  3.2e-07 (0.004)  4.6e-07 (0.001)  3.0e-07 (0.088)  1.4e-08 (0.004)
  120/30/10  general  lr1e-2   8.2e-08 (0.002)  2.7e-07 (0.001)  1.9e-07 (0.028)  1.9e-08 (0.001)
  120/30/10  fp32     lr1e-2   1.0e-07 (0.002)  3.1e-07 (0.001)  2.7e-07 (0.038)  2.7e-08 (0.002)
  120/30/10  general  lr1e-4   1.0e-07 (0.000)  6.9e-07 (0.001)  2.0e-07 (0.012)  1.1e-08 (0.001)
  120/30/10  fp32     lr1e-4   1.0e-07 (0.000)  5.4e-07 (0.001)  1.7e-07 (0.013)  2.0e-08 (0.001)
  115/27/7   hw       carried  1.2e-07 (0.001)  2.7e-07 (0.000)  1.4e-06 (0.295)  2.3e-08 (0.004)
  115/27/7   hw_sync  carried  7.5e-08 (0.000)  2.7e-07 (0.000)  5.4e-07 (0.034)  2.3e-08 (0.004)
  115/27/7   c4       carried  1.2e-07 (0.001)  2.7e-07 (0.000)  1.4e-06 (0.295)  2.3e-08 (0.004)
  115/27/7   fp32     carried  1.2e-07 (0.001)  3.5e-07 (0.001)  1.0e-06 (0.305)  2.8e-08 (0.003)
  115/27/7   hw       step1e5  9.1e-07 (0.011)  6.3e-07 (0.001)  1.1e-06 (0.074)  5.0e-08 (0.005)
  115/27/7   hw_sync  step1e5  9.1e-07 (0.011)  6.3e-07 (0.001)  1.1e-06 (0.032)  5.0e-08 (0.005)
  115/27/7   c4       step1e5  9.1e-07 (0.011)  6.3e-07 (0.001)  1.1e-06 (0.079)  5.0e-08 (0.005)
  115/27/7   fp32     step1e5  1.5e-06 (0.022)  1.3e-06 (0.003)  1.0e-06 (0.259)  6.5e-08 (0.005)
  115/27/7   hw       lr1e-2   9.9e-08 (0.001)  5.3e-07 (0.001)  3.0e-07 (0.071)  1.8e-08 (0.002)
  115/27/7   hw_sync  lr1e-2   9.9e-08 (0.001)  5.3e-07 (0.001)  3.0e-07 (0.036)  1.8e-08 (0.002)
  115/27/7   c4       lr1e-2   9.9e-08 (0.001)  5.3e-07 (0.001)  3.0e-07 (0.036)  1.8e-08 (0.002)
  115/27/7   fp32     lr1e-2   7.2e-08 (0.001)  6.1e-07 (0.001)  4.4e-07 (0.055)  1.0e-08 (0.002)
  115/27/7   hw       lr1e-4   9.3e-08 (0.000)  4.1e-07 (0.001)  2.4e-07 (0.014)  1.7e-08 (0.013)
  115/27/7   hw_sync  lr1e-4   9.3e-08 (0.000)  4.1e-07 (0.001)  2.4e-07 (0.014)  1.7e-08 (0.013)
  115/27/7   c4       lr1e-4   9.3e-08 (0.000)  4.1e-07 (0.001)  2.4e-07 (0.014)  1.7e-08 (0.013)
  115/27/7   fp32     lr1e-4   9.3e-08 (0.000)  5.8e-07 (0.001)  2.6e-07 (0.015)  1.5e-08 (0.004)
  115/27/7   hw       launch1  7.8e-07 (0.018)  1.5e-07 (0.000)  2.4e-07 (0.020)  5.0e-07 (0.003)
  115/27/7   hw_sync  launch1  8.5e-08 (0.001)  1.3e-07 (0.000)  2.2e-07 (0.020)  5.0e-07 (0.003)
  115/27/7   c4       launch1  2.7e-07 (0.006)  2.7e-07 (0.000)  2.4e-07 (0.020)  5.0e-07 (0.003)
  115/27/7   fp32     launch1  3.6e-06 (0.083)  4.0e-07 (0.001)  1.6e-07 (0.043)  6.5e-09 (0.003)
  115/27/7   hw       launch2  6.7e-07 (0.021)  3.0e-07 (0.001)  4.2e-07 (0.079)  7.3e-07 (0.004)
  115/27/7   hw_sync  launch2  1.2e-07 (0.001)  3.0e-07 (0.001)  4.2e-07 (0.079)  7.3e-07 (0.004)
  115/27/7   c4       launch2  2.3e-07 (0.007)  3.0e-07 (0.001)  4.2e-07 (0.079)  7.3e-07 (0.004)
  115/27/7   fp32     launch2  3.1e-06 (0.095)  4.4e-07 (0.001)  6.4e-07 (0.113)  1.9e-08 (0.001)
  46/28/8    general  b.5/.9   9.0e-08 (0.001)  2.2e-07 (0.000)  5.0e-07 (0.053)  6.9e-07 (0.005)
  46/28/8    fp32     b.5/.9   9.0e-08 (0.000)  3.8e-07 (0.001)  7.2e-07 (0.304)  3.9e-07 (0.003)
  46/28/8    general  b0/.99   7.7e-08 (0.003)  3.1e-07 (0.000)  1.3e-06 (0.080)  7.2e-08 (0.002)
  46/28/8    fp32     b0/.99   7.7e-08 (0.002)  5.7e-07 (0.001)  1.3e-06 (0.136)  7.5e-08 (0.002)
  46/27/7    hw       carried  9.2e-08 (0.001)  3.9e-07 (0.001)  2.9e-07 (0.021)  1.3e-08 (0.001)
  46/27/7    hw_sync  carried  7.8e-08 (0.001)  3.4e-07 (0.000)  2.0e-07 (0.015)  1.3e-08 (0.001)
  46/27/7    c4       carried  9.2e-08 (0.001)  3.9e-07 (0.001)  2.9e-07 (0.021)  1.3e-08 (0.001)
  46/27/7    fp32     carried  9.2e-08 (0.000)  5.8e-07 (0.001)  2.2e-07 (0.016)  1.3e-08 (0.001)
  46/27/7    hw       step1e5  8.9e-08 (0.002)  4.9e-07 (0.001)  3.8e-07 (0.043)  2.5e-08 (0.001)
  46/27/7    hw_sync  step1e5  8.9e-08 (0.001)  4.9e-07 (0.001)  1.8e-07 (0.012)  1.6e-08 (0.001)
  46/27/7    c4       step1e5  8.9e-08 (0.002)  4.9e-07 (0.001)  3.8e-07 (0.043)  2.5e-08 (0.001)
  46/27/7    fp32     step1e5  3.4e-07 (0.002)  6.2e-07 (0.001)  2.7e-07 (0.031)  1.0e-08 (0.001)
  46/27/7    hw       lr1e-2   1.0e-07 (0.001)  3.2e-07 (0.001)  3.2e-07 (0.018)  2.9e-08 (0.001)
  46/27/7    hw_sync  lr1e-2   1.0e-07 (0.001)  3.2e-07 (0.001)  3.2e-07 (0.018)  2.9e-08 (0.001)
  46/27/7    c4       lr1e-2   1.0e-07 (0.001)  3.2e-07 (0.001)  3.2e-07 (0.024)  2.9e-08 (0.001)
  46/27/7    fp32     lr1e-2   8.8e-08 (0.001)  5.0e-07 (0.001)  3.2e-07 (0.024)  2.2e-08 (0.001)
  46/27/7    hw       lr1e-4   7.7e-08 (0.000)  2.5e-07 (0.000)  3.0e-07 (0.009)  1.9e-08 (0.001)
  46/27/7    hw_sync  lr1e-4   7.7e-08 (0.000)  2.5e-07 (0.000)  3.0e-07 (0.009)  1.9e-08 (0.001)
  46/27/7    c4       lr1e-4   7.7e-08 (0.000)  2.5e-07 (0.000)  3.0e-07 (0.009)  1.9e-08 (0.001)
  46/27/7    fp32     lr1e-4   7.7e-08 (0.000)  8.5e-07 (0.001)  1.2e-07 (0.010)  1.7e-08 (0.001)
  46/27/7    hw       b.5/.9   9.5e-08 (0.000)  2.8e-07 (0.000)  6.4e-07 (0.043)  1.0e-06 (0.003)
  46/27/7    hw_sync  b.5/.9   9.5e-08 (0.000)  2.8e-07 (0.000)  6.4e-07 (0.043)  1.0e-06 (0.003)
  46/27/7    c4       b.5/.9   9.5e-08 (0.000)  2.8e-07 (0.000)  6.4e-07 (0.043)  1.0e-06 (0.003)
  46/27/7    fp32     b.5/.9   9.5e-08 (0.001)  6.2e-07 (0.001)  6.8e-07 (0.037)  7.4e-07 (0.001)
  46/27/7    hw       b0/.99   8.8e-08 (0.001)  4.0e-07 (0.001)  1.0e-06 (0.065)  1.4e-07 (0.001)
  46/27/7    hw_sync  b0/.99   8.8e-08 (0.001)  4.0e-07 (0.001)  1.0e-06 (0.065)  1.4e-07 (0.001)
  46/27/7    c4       b0/.99   8.8e-08 (0.001)  4.0e-07 (0.001)  1.0e-06 (0.065)  1.4e-07 (0.001)
  46/27/7    fp32     b0/.99   8.8e-08 (0.002)  1.0e-06 (0.001)  1.3e-06 (0.097)  9.7e-08 (0.002)
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_f64 as O  # noqa: E402
import train_state_oracle as T  # noqa: E402
from fedmse_decentralized_amd.models.layout import real_mask_padded  # noqa: E402
from fedmse_decentralized_amd.ops import _hip  # noqa: E402

DEV = torch.device("cuda", 0)
FAMILY_KW = {"hw": dict(helper=True), "hw_sync": dict(helper=True, async_valid=False), "c4": dict(helper=False),
             "general": dict()}
EVERYTHING = O.STATE + ("adam_step",)


def _hip_engine(case):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    return O.setup_engine(HipEngine(case.dims, DEV), case)


def _planted_engine(shape, si, hp, variant, step0=None):
    """A HipEngine on the case with the oracle's launch-1 state planted."""
    case = T.state_case(shape, si, T.case_seed(shape, si, hp, variant))
    eng = _hip_engine(case)
    T.plant(eng, T.planted_state(shape, si, hp, variant), T.STEP0.get(variant) if step0 is None else step0)
    return case, eng


def _launch(eng, hp, ids=O.TRAINED, **kw) -> O.Trained:
    """One training launch of store rows ``ids``, read back after a sync."""
    trk, er, be = _hip.train(eng.store, list(ids), hp, eng.dims, **kw)
    torch.cuda.synchronize()
    _hip.runtime(DEV).sync()
    er = [int(e) for e in er]
    assert min(er) >= 0, f"training launch failed: epochs_run {er}"
    res = SimpleNamespace(epochs_run=er, best_epoch=[int(b) for b in be],
                          tracking=[[(float(trk[i, e, 0]), float(trk[i, e, 1])) for e in range(er[i])]
                                    for i in range(len(er))])
    return O.snapshot(eng.store, res)


def _assert_matches(got: O.Trained, ref: O.Trained, dims, what: str):
    """Decisions and step counts equal; tracking and state within ``O.TOL``;
    padding exactly zero."""
    assert got.epochs_run == ref.epochs_run, what
    assert got.best_epoch == ref.best_epoch, what
    assert torch.equal(got.state["adam_step"], ref.state["adam_step"]), what
    rtol, atol = O.TOL["tracking"]
    for tg, tr in zip(got.tracking, ref.tracking):
        np.testing.assert_allclose(np.array(tg), np.array(tr), rtol=rtol, atol=atol, err_msg=what)
    for name in O.STATE:
        rtol, atol = O.TOL[name]
        assert got.state[name].dtype == torch.float32
        torch.testing.assert_close(got.state[name][O.TRAINED].double(), ref.state[name][O.TRAINED], rtol=rtol,
                                   atol=atol, msg=lambda m, n=name: f"{what} {n}: {m}")
    pad = ~real_mask_padded(dims)
    for name in O.STATE:
        assert torch.count_nonzero(got.state[name][:, pad]) == 0, f"{what}: {name} padding"


def _family_cases():
    return [(fam, case) for case in T.CASES for fam in T.case_families(case)]


@pytest.mark.parametrize("family,case", _family_cases(), ids=lambda v: v if isinstance(v, str) else T.case_id(v))
def test_launch_from_carried_state_matches_fp64_oracle(family, case):
    """Launch 2 alone, from the oracle's planted launch-1 state: decisions,
    step counts, tracking, parameters, snapshot and both moments against the
    fp64 oracle; padding zero; untrained client, anchor and data bit-unchanged."""
    shape, hp, variant = case
    for si in T.case_sizes(case):
        ref = T.trained_from(shape, si, hp, variant, True)
        cs, eng = _planted_engine(shape, si, hp, variant)
        st = eng.store
        before = {n: getattr(st, n).clone() for n in EVERYTHING + ("anchor", "train", "valid")}
        got = _launch(eng, T.hparams(hp, variant), **FAMILY_KW[family])
        what = f"{family} {shape} sizes {O.DATA_SIZES[si]} hp {hp} {variant}"
        for name, (absd, use) in O.distances(got, ref).items():   # the figures, before anything is asserted
            print(f"DIST {family} {shape} {si} {hp} {variant} {name} abs {absd:.3e} use {use:.4f}")
        _assert_matches(got, ref, cs.dims, what)
        # the stored step: what was planted plus one per batch of every epoch run
        step0 = before["adam_step"][O.TRAINED].tolist()
        assert step0 == [T.STEP0.get(variant, int(s)) for s in T.planted_state(shape, si, hp, variant)["adam_step"][O.TRAINED]]
        steps = [s + e * -(-n // hp[0]) for s, e, n in zip(step0, got.epochs_run, O.DATA_SIZES[si][0])]
        assert got.state["adam_step"][O.TRAINED].tolist() == steps and min(step0) > 0, what
        # nothing of the untrained client moved, nor the anchor and the data of any client
        for name in EVERYTHING:
            assert torch.equal(getattr(st, name)[O.UNTRAINED], before[name][O.UNTRAINED]), f"{what}: untrained {name}"
        for name in ("anchor", "train", "valid"):
            assert torch.equal(getattr(st, name), before[name]), f"{what}: {name} written"


# (115, 27, 7), batch 12, carried: at data size 0 both clients' best epoch is
# the last one run; at size 1 client 0 stops after epoch 1 with epoch 0 its best
BEST_CASE = ((115, 27, 7), O.HPARAMS[0], "carried")


@pytest.mark.parametrize("family", T.COMPACT_FAMILIES)
def test_best_snapshot_is_of_this_launch_and_unscaled(family):
    """``best`` after launch 2 is the kernel's own final ``params``, bit for
    bit, where the best epoch is the last one run, and otherwise neither the
    planted snapshot nor the final parameters (which of the two follows from
    the fp64 oracle's ``best_epoch``; both kinds occur)."""
    shape, hp, variant = BEST_CASE
    kinds = set()
    for si in T.case_sizes(BEST_CASE):
        ref = T.trained_from(shape, si, hp, variant, True)
        planted = T.planted_state(shape, si, hp, variant)
        _, eng = _planted_engine(shape, si, hp, variant)
        got = _launch(eng, T.hparams(hp, variant), **FAMILY_KW[family])
        assert got.epochs_run == ref.epochs_run and got.best_epoch == ref.best_epoch
        for row in O.TRAINED:
            what = f"{family} sizes {O.DATA_SIZES[si]} row {row}"
            best, params = got.state["best"][row], got.state["params"][row]
            last = ref.best_epoch[row] == ref.epochs_run[row] - 1
            kinds.add(last)
            assert not torch.equal(best, planted["best"][row]), what
            assert not torch.equal(params, planted["params"][row]), what
            assert torch.equal(best, params) == last, what
    assert kinds == {True, False}


BITWISE_HP = [hp for hp in O.HPARAMS if hp[0] <= 12]


@pytest.mark.parametrize("variant", ["carried", "b.5/.9"])
@pytest.mark.parametrize("hp", BITWISE_HP, ids=lambda hp: f"b{hp[0]}-mu{hp[1]:g}")
@pytest.mark.parametrize("shape", [(115, 27, 7), (46, 27, 7)], ids=lambda s: "x".join(map(str, s)))
def test_families_agree_bitwise_from_planted_state(shape, hp, variant):
    """Batch <= 12: the helper-wave kernel (asynchronous and synchronous epoch
    tail) and the compact 4-wave kernel give identical state and step counts
    from the same planted state, as they do from zero state; only the fp64
    loss sums are grouped differently.  Any role that scales a tile on its own
    terms breaks it."""
    for si in (0, 1):
        runs = {}
        for fam in T.COMPACT_FAMILIES:
            _, eng = _planted_engine(shape, si, hp, variant)
            runs[fam] = _launch(eng, T.hparams(hp, variant), **FAMILY_KW[fam])
        ra = runs["hw"]
        for fam in ("hw_sync", "c4"):
            rb = runs[fam]
            what = f"{shape} sizes {O.DATA_SIZES[si]} hp {hp} {variant}: hw against {fam}"
            assert ra.epochs_run == rb.epochs_run and ra.best_epoch == rb.best_epoch, what
            for ta, tb in zip(ra.tracking, rb.tracking):
                np.testing.assert_allclose(np.array(ta), np.array(tb), rtol=1e-9, atol=0, err_msg=what)
            for name in EVERYTHING:
                assert torch.equal(ra.state[name], rb.state[name]), f"{what}: {name}"


def _two_launch_rows():
    return [(fam, shape, hp) for shape, hp in T.TWO_LAUNCH_CASES
            for fam in T.case_families((shape, hp, "carried"))]


@pytest.mark.parametrize("family,shape,hp", _two_launch_rows(),
                         ids=[f"{f}-b{hp[0]}-mu{hp[1]:g}" for f, _, hp in _two_launch_rows()])
def test_two_launches_on_the_device_match_fp64_oracle(family, shape, hp):
    """The path the federation takes: the kernel runs launch 1 and launch 2
    itself from ``setup()``, its own launch-1 state carried in the store."""
    ref = T.two_launches(shape, 0, hp, True)
    case = T.state_case(shape, 0, T.case_seed(shape, 0, hp, T.TWO_LAUNCH))
    eng = _hip_engine(case)
    for launch in range(2):
        got = _launch(eng, O.hparams(*hp), **FAMILY_KW[family])
        for name, (absd, use) in O.distances(got, ref[launch]).items():
            print(f"DIST {family} {shape} 0 {hp} launch{launch + 1} {name} abs {absd:.3e} use {use:.4f}")
        _assert_matches(got, ref[launch], case.dims, f"{family} {shape} hp {hp} launch {launch + 1}")


@pytest.mark.parametrize("family,shape", [("hw", (115, 27, 7)), ("hw_sync", (115, 27, 7)), ("c4", (115, 27, 7)),
                                          ("general", (120, 30, 10))],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_concurrent_clients_keep_their_own_step(family, shape):
    """One launch of client 0 at step 0 with zero moments (its ``setup()``
    state) beside client 1 at step 100000 with carried moments: each ends
    exactly as in a launch of its own (the step is per client, not per launch)."""
    hp = O.HPARAMS[0]
    state = T.planted_state(shape, 0, hp, "carried")

    def engine():
        case = T.state_case(shape, 0, T.case_seed(shape, 0, hp, "carried"))
        eng = _hip_engine(case)
        fresh = {n: getattr(eng.store, n)[0].clone() for n in O.STATE}
        T.plant(eng, state, step0=(0, 100000))
        for n in O.STATE:
            getattr(eng.store, n)[0] = fresh[n]
        assert int(torch.count_nonzero(eng.store.adam_m[0])) == 0 and int(torch.count_nonzero(eng.store.adam_m[1])) > 0
        return eng

    both, solo = engine(), [engine(), engine()]
    before = {n: getattr(both.store, n).clone() for n in EVERYTHING + ("anchor", "train", "valid")}
    rb = _launch(both, O.hparams(*hp), **FAMILY_KW[family])
    n_train = O.DATA_SIZES[0][0]
    for row in O.TRAINED:
        rs = _launch(solo[row], O.hparams(*hp), ids=[row], **FAMILY_KW[family])
        what = f"{family} {shape} row {row}"
        assert (rb.epochs_run[row], rb.best_epoch[row]) == (rs.epochs_run[0], rs.best_epoch[0]), what
        assert np.array_equal(np.array(rb.tracking[row]), np.array(rs.tracking[0])), what
        for name in EVERYTHING:
            assert torch.equal(rb.state[name][row], rs.state[name][row]), f"{what}: {name}"
            # and the solo launch left the other trained row as planted
            other = 1 - row
            assert torch.equal(rs.state[name][other], before[name][other].cpu()), f"{what}: other row's {name}"
        assert int(rb.state["adam_step"][row]) == (0, 100000)[row] + rb.epochs_run[row] * -(-n_train[row] // hp[0]), what
    for name in EVERYTHING:
        assert torch.equal(getattr(both.store, name)[O.UNTRAINED], before[name][O.UNTRAINED]), f"untrained {name}"
    for name in ("anchor", "train", "valid"):
        assert torch.equal(getattr(both.store, name), before[name]), f"{name} written"
