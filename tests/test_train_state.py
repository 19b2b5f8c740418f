"""CPU side of the carried-state training cases (``tests/train_state_oracle.py``):
what has to hold for the GPU tests of ``test_train_state_gpu.py`` to be fair.

For every case, launch 2 from the planted launch-1 state: the fp32 and the
fp64 oracle decide alike, every pair of validation losses the early stop
compares is ``DECISION_GAP`` apart in fp64, the fp32 oracle alone uses at
most half of each tolerance, and the planted state exercises every
parameter tile's moment load (non-zero ``adam_m`` / ``adam_v`` in all eight
tensors, ``adam_step > 0``).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_f64 as O  # noqa: E402
import train_state_oracle as T  # noqa: E402
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine  # noqa: E402
from fedmse_decentralized_amd.models.layout import ModelDims, padded_to_canonical, real_mask_padded  # noqa: E402
from fedmse_decentralized_amd.models.reference import unflatten  # noqa: E402


def _check_fair(f32: O.Trained, f64: O.Trained, step0, n_train, batch, what):
    """Same decisions and step counts, clear decisions, fp32 within half."""
    assert f64.state["params"].dtype == torch.float64 and f32.state["params"].dtype == torch.float32
    assert f32.epochs_run == f64.epochs_run, what
    assert f32.best_epoch == f64.best_epoch, what
    assert torch.equal(f32.state["adam_step"], f64.state["adam_step"]), what
    steps = [s + e * -(-n // batch) for s, e, n in zip(step0, f64.epochs_run, n_train)] + [0]
    assert f64.state["adam_step"].tolist() == steps, what
    gaps = O.decision_gaps(f64.tracking)
    assert all(g >= O.DECISION_GAP for g in gaps), (what, gaps)
    for name, (absd, use) in O.distances(f32, f64).items():
        assert use <= 0.5, (what, name, absd, use)


def _check_padding(state, dims, what):
    pad = ~real_mask_padded(dims)
    for name in O.STATE:
        assert torch.count_nonzero(state[name][:, pad]) == 0, f"{what}: {name} padding"


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_launch_from_carried_state_is_a_fair_case(case):
    shape, hp, variant = case
    dims = ModelDims(*shape)
    for si in T.case_sizes(case):
        what = f"{shape} sizes {O.DATA_SIZES[si]} hp {hp} {variant}"
        state = T.planted_state(shape, si, hp, variant)
        case_ = T.state_case(shape, si, T.case_seed(shape, si, hp, variant))
        fresh = O.oracle(dims, case_, case_.anchor, True).store   # as setup() leaves it
        # the planted state: fp32, padding zero, v >= 0, steps taken, and
        # non-zero moments in every tensor (W1..W4 and the four biases) of both rows
        _check_padding(state, dims, what + " planted")
        assert all(state[n].dtype == torch.float32 for n in O.STATE), what
        assert bool((state["adam_v"] >= 0).all()), what
        assert all(int(s) > 0 for s in state["adam_step"][O.TRAINED]), what
        for row in O.TRAINED:
            for name in ("adam_m", "adam_v"):
                tensors = unflatten(padded_to_canonical(state[name][row], dims), dims)
                assert len(tensors) == 8
                assert all(int(torch.count_nonzero(t)) > 0 for t in tensors), f"{what}: {name} row {row}"
            assert not torch.equal(state["params"][row], fresh.params[row].float()), what
        f32 = T.trained_from(shape, si, hp, variant, False)
        f64 = T.trained_from(shape, si, hp, variant, True)
        step0 = [T.STEP0.get(variant, int(s)) for s in state["adam_step"][O.TRAINED]]
        _check_fair(f32, f64, step0, O.DATA_SIZES[si][0], hp[0], what)
        for got in (f32, f64):
            _check_padding(got.state, dims, what)
        # launch 2 moved what it was given, and left the untrained client alone
        for name in O.STATE:
            assert not torch.equal(f64.state[name][O.TRAINED].float(), state[name][O.TRAINED]), f"{what}: {name}"
        for name in ("adam_m", "adam_v", "best"):
            assert torch.equal(f64.state[name][O.UNTRAINED], getattr(fresh, name)[O.UNTRAINED]), f"{what}: {name}"


@pytest.mark.parametrize("shape,hp", T.TWO_LAUNCH_CASES, ids=[f"b{hp[0]}-mu{hp[1]:g}" for _, hp in T.TWO_LAUNCH_CASES])
def test_two_launches_from_setup_are_a_fair_case(shape, hp):
    """Both launches run by the oracle itself: both launches' decisions are
    clear, and the fp32 oracle (its own launch-1 error included) stays within
    half of every tolerance after each."""
    n_train = O.DATA_SIZES[0][0]
    a, b = T.two_launches(shape, 0, hp, False), T.two_launches(shape, 0, hp, True)
    step0 = [0, 0]
    for launch, (f32, f64) in enumerate(zip(a, b)):
        _check_fair(f32, f64, step0, n_train, hp[0], f"{shape} hp {hp} launch {launch}")
        _check_padding(f64.state, ModelDims(*shape), f"{shape} hp {hp} launch {launch}")
        step0 = f64.state["adam_step"][O.TRAINED].tolist()
    assert all(s > 0 for s in step0)


def test_plant_copies_the_trained_rows_only():
    shape, hp = (46, 27, 7), O.HPARAMS[0]
    state = T.planted_state(shape, 0, hp, "carried")
    case = T.state_case(shape, 0, 0)
    for f64 in (False, True):
        eng = O.oracle(case.dims, case, case.anchor, f64)
        before = {n: getattr(eng.store, n).clone() for n in O.STATE + ("adam_step", "anchor")}
        T.plant(eng, state)
        for name in O.STATE:
            got = getattr(eng.store, name)
            assert got.dtype == (torch.float64 if f64 else torch.float32)
            assert torch.equal(got[O.TRAINED].float(), state[name][O.TRAINED]), name
            assert torch.equal(got[O.UNTRAINED], before[name][O.UNTRAINED]), name
        assert torch.equal(eng.store.adam_step[O.TRAINED], state["adam_step"][O.TRAINED])
        assert int(eng.store.adam_step[O.UNTRAINED]) == 0
        assert torch.equal(eng.store.anchor, before["anchor"])
        T.plant(eng, state, step0=100000)
        assert eng.store.adam_step.tolist() == [100000, 100000, 0]
        T.plant(eng, state, step0=(0, 7))
        assert eng.store.adam_step.tolist() == [0, 7, 0]
    # the cached state itself is what launch 1 of the fp64 oracle left, rounded once
    eng = O.oracle(case.dims, case, case.anchor, True)
    eng.train(O.TRAINED, T.hparams(hp, "carried"))
    for name in O.STATE:
        assert torch.equal(getattr(eng.store, name).float(), state[name]), name
    assert isinstance(eng, TorchEngine)


def test_step1e5_bias_corrections_are_one():
    """What ``step1e5`` relies on: both powers underflow to exactly 0 in
    double, so a kernel that reads the step has ``bc1 == bc2 == 1``; one that
    starts from step 0 has ``bc1 = 0.1`` at its first step."""
    assert 0.9 ** 100000 == 0.0 and 0.999 ** 100000 < 1e-43
    assert 1.0 - 0.999 ** 100000 == 1.0
    assert T.hparams(O.HPARAMS[0], "step1e5") == T.hparams(O.HPARAMS[0], "carried")
    assert T.planted_state((46, 27, 7), 0, O.HPARAMS[0], "step1e5") is T.planted_state((46, 27, 7), 0, O.HPARAMS[0],
                                                                                      "carried")


def test_case_list_covers_the_issue():
    """Every family, both FedProx settings, the three batch ranges and each
    variant; every named (shape, family, variant) combination; the extra data
    size for batch 12 and 7."""
    fams = {f for c in T.CASES for f in T.case_families(c)}
    assert fams == {"hw", "hw_sync", "c4", "general"}
    assert {c[1][1] != 0.0 for c in T.CASES} == {True, False}
    batches = {c[1][0] for c in T.CASES}
    assert any(b <= 12 for b in batches) and any(12 < b <= 16 for b in batches) and any(b > 16 for b in batches)
    assert {c[2] for c in T.CASES} == set(T.VARIANTS)
    assert len(set(T.CASES)) == len(T.CASES)
    have = {(c[0], f, c[2]) for c in T.CASES for f in T.case_families(c)}
    for shape in ((115, 27, 7), (46, 27, 7)):
        for fam in T.COMPACT_FAMILIES:
            for v in ("carried", "step1e5", "lr1e-2", "lr1e-4"):
                assert (shape, fam, v) in have
    for v in ("carried", "step1e5", "lr1e-2", "lr1e-4"):
        assert ((120, 30, 10), "general", v) in have
    for v in T.BETA_VARIANTS:
        assert ((46, 28, 8), "general", v) in have
        assert all(((46, 27, 7), fam, v) in have for fam in T.COMPACT_FAMILIES)
    for shape in ((115, 27, 7), (46, 27, 7), (120, 30, 10)):
        for v in ("carried", "step1e5"):
            assert {c[1] for c in T.CASES if c[0] == shape and c[2] == v} == set(O.HPARAMS)
        for v in ("lr1e-2", "lr1e-4"):
            assert {c[1] for c in T.CASES if c[0] == shape and c[2] == v} == {O.HPARAMS[0], O.HPARAMS[3]}
    for c in T.CASES:
        ModelDims(*c[0])
        assert T.case_sizes(c) == ((0, 1) if c[1][0] in (12, 7) else (0,))
        general = c[0][1] > 27 or c[0][2] > 7
        assert T.case_families(c) == (("general",) if general else tuple(
            f for f in T.COMPACT_FAMILIES if f != "hw_sync" or (c[1][0] <= 12 and c[1][1] == 0.0)))
    # every seed on record belongs to a case that runs
    runs = {(c[0], si, c[1], c[2]) for c in T.CASES for si in T.case_sizes(c)}
    assert set(T.SEEDS) <= runs and all(1 <= s <= 39 for s in T.SEEDS.values())
    # non-default settings really differ from the defaults the other tests use
    for v in T.BETA_VARIANTS:
        h = T.hparams(O.HPARAMS[0], v)
        assert (h.beta1, h.beta2) != (0.9, 0.999)
    assert T.hparams(O.HPARAMS[0], "lr1e-2").lr == 1e-2 and T.hparams(O.HPARAMS[0], "lr1e-4").lr == 1e-4
