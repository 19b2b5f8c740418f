"""Training launches that start from carried-over Adam state: builders and
the case list shared by ``test_train_state.py`` (CPU) and
``test_train_state_gpu.py`` (GPU), on top of ``tests/oracle_f64.py``.

Every round after the first starts a client's launch from what the last one
left in the store: moved parameters, non-zero ``adam_m`` / ``adam_v`` and
``adam_step > 0``.  Launch 1 runs on the fp64 oracle; its state, rounded to
fp32, is planted into every engine under comparison (both oracles and the
kernels), so launch 2 is judged alone: no launch-1 kernel error enters.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import oracle_f64 as O
from fedmse_decentralized_amd.engine.base import TrainHParams
from fedmse_decentralized_amd.models.layout import ModelDims

# -- variants ---------------------------------------------------------------------
# what a variant changes: TrainHParams fields of both launches, and ``step0``,
# the adam_step planted into the trained rows instead of launch 1's own.
# pow(0.9, 1e5) and pow(0.999, 1e5) < 1e-43: both bias corrections are 1 to
# the last bit there, so step1e5 checks that the stored step is read at all
# (and written back as 100000 + steps).  b0/.99: the moment scale 1 / (1 - b1)
# is 1, pow(0, 0) is 1 and pow(0, t > 0) is 0.
VARIANTS: Dict[str, dict] = {
    "carried": {},
    "step1e5": {"step0": 100000},
    "lr1e-2": {"lr": 1e-2},
    "lr1e-4": {"lr": 1e-4},
    "b.5/.9": {"beta1": 0.5, "beta2": 0.9, "eps": 1e-4},
    "b0/.99": {"beta1": 0.0, "beta2": 0.99},
}
BETA_VARIANTS = ("b.5/.9", "b0/.99")
STEP0 = {v: kw["step0"] for v, kw in VARIANTS.items() if "step0" in kw}

# kernel families of a shape (tests/test_train_shapes_gpu.py): the helper-wave
# kernel, the same with the synchronous epoch tail, the compact 4-wave kernel;
# the general 4-wave kernel beyond hidden 27 / latent 7
COMPACT_FAMILIES = ("hw", "hw_sync", "c4")
SHAPE_FAMILIES = {(115, 27, 7): COMPACT_FAMILIES, (46, 27, 7): COMPACT_FAMILIES,
                  (120, 30, 10): ("general",), (46, 28, 8): ("general",)}


def _cases() -> List[tuple]:
    out = []
    for shape in ((115, 27, 7), (46, 27, 7), (120, 30, 10)):
        out += [(shape, hp, v) for v in ("carried", "step1e5") for hp in O.HPARAMS]
        out += [(shape, hp, v) for v in ("lr1e-2", "lr1e-4") for hp in (O.HPARAMS[0], O.HPARAMS[3])]
    # low beta1 lets adam_m follow the fp32 rounding of single gradients, which
    # the adam_m tolerance cannot judge at the wide shapes: the beta variants
    # run at d_in 46 in both kernel families
    for shape in ((46, 27, 7), (46, 28, 8)):
        out += [(shape, hp, v) for v in BETA_VARIANTS for hp in (O.HPARAMS[0], O.HPARAMS[3])]
    return out


# (shape, (batch, mu, lambda), variant), each at data-size index 0
CASES: List[tuple] = _cases()
# the two-launch end-to-end runs (both launches from ``setup()`` on one engine)
TWO_LAUNCH_CASES = [((115, 27, 7), O.HPARAMS[0]), ((115, 27, 7), O.HPARAMS[3])]
TWO_LAUNCH = "two-launch"   # their name in SEEDS


def case_sizes(case) -> Tuple[int, ...]:
    """Data-size indices of a case: batch 12 and batch 7 also take index 1
    (one training row; one row over a batch)."""
    return (0, 1) if case[1][0] in (12, 7) else (0,)


def case_families(case) -> Tuple[str, ...]:
    """The kernel families a case runs on.  The helper-wave kernel validates
    asynchronously only in its plain instantiation (batch <= 12, no FedProx):
    only there is the synchronous tail another code path."""
    (batch, mu, _) = case[1]
    return tuple(f for f in SHAPE_FAMILIES[case[0]] if f != "hw_sync" or (batch <= 12 and mu == 0.0))


def case_id(case) -> str:
    (d, h, z), (batch, mu, lam), variant = case
    return f"{d}x{h}x{z}-b{batch}-mu{mu:g}-{variant}"


# Seed of a (shape, data-size index, hparams, variant) whose seed-0 data puts an
# fp64 early-stop comparison inside O.DECISION_GAP, or lets the fp32 oracle
# alone use more than half of a tolerance: the first seed in 1..39 that clears
# both, with what seed 0 gave and the smallest fp64 gap / largest fp32 usage
# at the chosen seed (CPU figures).  Every other case, the two-launch runs
# included, runs at seed 0.
SEEDS: Dict[tuple, int] = {
    # seed 0: fp64 gap 1.72e-04; seed 2: gap 2.77e-03, fp32 usage 0.011
    ((115, 27, 7), 1, (7, 1e-3, 5.0), "carried"): 2,
    # seed 0: gap 6.34e-04; seed 1: gap 5.94e-03, usage 0.003
    ((46, 27, 7), 1, (12, 0.0, 5.0), "carried"): 1,
    # seed 0: gap 5.27e-05; seed 1: gap 1.08e-03, usage 0.005
    ((46, 27, 7), 1, (12, 0.0, 5.0), "lr1e-4"): 1,
    # seed 0: gap 3.81e-04; seed 1: gap 3.85e-03, usage 0.007
    ((46, 27, 7), 1, (12, 0.0, 5.0), "b.5/.9"): 1,
    # seed 0: gap 1.91e-04; seed 1: gap 2.90e-03, usage 0.020
    ((46, 27, 7), 1, (12, 0.0, 5.0), "b0/.99"): 1,
    # seed 0: the fp32 oracle alone uses 4.68 x the params tolerance (gap 1.34e-02);
    # seed 1: gap 1.36e-02, usage 0.022
    ((120, 30, 10), 0, (12, 0.0, 5.0), "carried"): 1,
    # seed 0: gap 7.03e-04; seeds 1..10 below DECISION_GAP too; seed 11: gap 1.23e-03, usage 0.009
    ((120, 30, 10), 1, (12, 0.0, 5.0), "lr1e-4"): 11,
}
# The (46, 28, 8) beta rows keep O.TOL["adam_m"] (rtol 5e-3, atol 1e-6): the
# fp32 oracle's largest adam_m distance to fp64 over them is 1.32e-06, at most
# 0.30 of that tolerance (b.5/.9, batch 12), under the half that would call
# for a wider atol.


def case_seed(shape, size_idx: int, hp, variant: str) -> int:
    return SEEDS.get((tuple(shape), int(size_idx), tuple(hp), variant), 0)


def hparams(hp, variant: str) -> TrainHParams:
    """``O.hparams`` with the variant's Adam settings, the betas as the
    kernels read them: ``TrainArgs`` carries them in fp32, and fp32(0.999) is
    0.99900001287, whose ``1 - beta2`` is 1.29e-5 (relative) below 0.001.
    From zero state that cancels between ``v`` and its bias correction (the
    zero-state tests run the oracle at 0.999); a launch that continues a
    planted ``v`` history does not cancel it, so an oracle at the double 0.999
    would run another recursion than the kernel was asked for: on the CPU,
    the fp64 oracle at fp32(0.999) against itself at 0.999 is 4.6e-06 apart
    in ``adam_m`` (1.67 x its tolerance at (120, 30, 10), batch 7, carried).
    Like data, parameters and anchor, the betas are therefore the fp32 values
    in every run; ``two_launches`` keeps the plain 0.999, where the kernel
    carries its own history and the rounding cancels again."""
    out = O.hparams(*hp)
    for k, v in VARIANTS.get(variant, {}).items():
        if k != "step0":
            setattr(out, k, v)
    out.beta1 = float(np.float32(out.beta1))
    out.beta2 = float(np.float32(out.beta2))
    return out


@functools.lru_cache(maxsize=None)
def state_case(shape, size_idx: int, seed: int) -> O.Case:
    n_train, n_valid = O.DATA_SIZES[size_idx]
    return O.make_case(ModelDims(*shape), n_train, n_valid, seed)


def _settings(variant: str) -> str:
    """The variant whose TrainHParams launch 1 ran with (``step1e5`` plants
    the state of ``carried``)."""
    return "carried" if variant in STEP0 or variant == TWO_LAUNCH else variant


@functools.lru_cache(maxsize=None)
def carried_state(shape, size_idx: int, hp, seed: int, variant: str = "carried") -> Dict[str, torch.Tensor]:
    """What launch 1 of the fp64 oracle leaves in the store, with the
    variant's Adam settings: ``params``, ``best``, ``adam_m``, ``adam_v``
    rounded to fp32, and ``adam_step``.  Computed once per process; callers
    must not modify it."""
    case = state_case(shape, size_idx, seed)
    eng = O.oracle(case.dims, case, case.anchor, True)
    eng.train(O.TRAINED, hparams(hp, _settings(variant)))
    state = {n: getattr(eng.store, n).detach().to(torch.float32).clone() for n in O.STATE}
    state["adam_step"] = eng.store.adam_step.detach().clone()
    return state


def plant(engine, state, step0=None):
    """Copy ``state`` into the trained rows of ``engine``'s store, cast to the
    store's dtype; ``step0`` (one int, or one per trained row) replaces their
    ``adam_step``.  The untrained row keeps its ``setup()`` state."""
    st = engine.store
    rows = list(O.TRAINED)
    for name in O.STATE:
        dst = getattr(st, name)
        dst[rows] = state[name][rows].to(dtype=dst.dtype, device=dst.device)
    steps = state["adam_step"][rows].to(torch.int32)
    if step0 is not None:
        steps = torch.tensor([step0] * len(rows) if isinstance(step0, int) else list(step0), dtype=torch.int32)
    st.adam_step[rows] = steps.to(st.adam_step.device)
    return engine


def planted_state(shape, size_idx: int, hp, variant: str) -> Dict[str, torch.Tensor]:
    return carried_state(shape, size_idx, hp, case_seed(shape, size_idx, hp, variant), _settings(variant))


@functools.lru_cache(maxsize=None)
def trained_from(shape, size_idx: int, hp, variant: str, f64: bool, seed: Optional[int] = None) -> O.Trained:
    """The oracle's launch 2 from the planted state (``seed``: instead of the
    case's own).  Computed once per process; callers must not modify it."""
    seed = case_seed(shape, size_idx, hp, variant) if seed is None else seed
    case = state_case(shape, size_idx, seed)
    eng = O.oracle(case.dims, case, case.anchor, f64)
    plant(eng, carried_state(shape, size_idx, hp, seed, _settings(variant)), STEP0.get(variant))
    return O.snapshot(eng.store, eng.train(O.TRAINED, hparams(hp, variant)))


@functools.lru_cache(maxsize=None)
def two_launches(shape, size_idx: int, hp, f64: bool, seed: Optional[int] = None) -> Tuple[O.Trained, O.Trained]:
    """The oracle running launch 1 and launch 2 itself from ``setup()``: the
    path the federation takes."""
    seed = case_seed(shape, size_idx, hp, TWO_LAUNCH) if seed is None else seed
    case = state_case(shape, size_idx, seed)
    eng = O.oracle(case.dims, case, case.anchor, f64)
    first = O.snapshot(eng.store, eng.train(O.TRAINED, O.hparams(*hp)))
    return first, O.snapshot(eng.store, eng.train(O.TRAINED, O.hparams(*hp)))
