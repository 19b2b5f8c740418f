"""The training launch's validation pass and early stop: case lists, builders
and seed tables shared by ``test_train_epochs.py`` (CPU) and
``test_train_epochs_gpu.py`` (GPU), on top of ``tests/oracle_f64.py``.

Part A (``SIZE_CASES``) trains two epochs on small training sets and validates
on sets whose sizes sit on the edges of the kernels' validation loops: the
16-row tiles of the helper-wave kernel's ``epoch_tail`` and validator
workgroup, and the per-batch / per-chunk loops of the 4-wave kernels.  Part B
(``CONTROL_CASES``) trains up to eight epochs at a learning rate that makes
the validation loss rise, so that the patience rule and the best snapshot
take every decision pattern listed in ``PATTERNS``.  Each case trains two
clients per launch, beside the untrained third row of ``oracle_f64.make_case``.
"""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

import oracle_f64 as O
from fedmse_decentralized_amd.engine.base import TrainHParams
from fedmse_decentralized_amd.models.layout import ModelDims, padded_to_canonical
from fedmse_decentralized_amd.models.reference import unflatten

COMPACT_FAMILIES = ("hw", "hw_sync", "c4")
FAMILY_KW = {"hw": dict(helper=True), "hw_sync": dict(helper=True, async_valid=False), "c4": dict(helper=False),
             "general": dict()}
COMPACT_A_SHAPES = [(115, 27, 7), (46, 27, 7)]
GENERAL_SHAPE = (120, 30, 10)
LAMBDA = 5.0
NO_STOP = 10 ** 6      # a patience no launch reaches
AV_CHECK = 6           # fedmx_train_hw.hip: the step before which a trainer needs the last epoch's decision
TILE = 16              # rows of one validation tile (helper-wave kernel) / chunk (4-wave kernels)


class EpochCase(NamedTuple):
    part: str                  # "A" (validation sizes) or "B" (epoch control)
    shape: Tuple[int, int, int]
    batch: int
    mu: float
    lr: float
    patience: int
    epochs: int
    n_train: Tuple[int, int]
    n_valid: Tuple[int, int]
    tag: str = ""              # tells apart cases that differ in their seed alone

    @property
    def data_key(self) -> tuple:
        """What fixes the data and the trajectory (not when it is cut off):
        the key of ``SEEDS``, shared by a case and its patience / epochs variants."""
        return (self.shape, self.batch, self.mu, self.lr, self.n_train, self.n_valid, self.tag)


# -- Part A: validation-set sizes ----------------------------------------------------
A_TRAIN = (13, 24)
# n_valid of the two clients.  15 / 16 / 17: the first tile edge; 48 / 49 at
# batch 12: four and five batches (the 4-wave kernel's second pass); 50 at
# batch 33: a last batch of 17 rows, whose second chunk holds one; 127 / 128 /
# 129: eight and nine tiles (the validator's second preloaded tile, the second
# pass of epoch_tail); 255 / 256 / 257: sixteen and seventeen tiles (the
# validator's reload loop); 385: wave 0's second reload iteration.
A_VALID = [(15, 16), (17, 48), (49, 50), (127, 128), (129, 255), (256, 257), (385, 129)]
# (batch, mu): 7 straddles the tiles unevenly, 16 is the tile, 33 spans three
# tiles (with FedProx: the helper-wave kernel's synchronous multi-chunk
# instantiation), 64 is the thesis's batch
A_BATCHES = [(12, 0.0), (7, 0.0), (16, 0.0), (33, 1e-3), (64, 0.0)]


def size_case(shape, batch: int, mu: float, n_valid) -> EpochCase:
    return EpochCase("A", tuple(shape), batch, mu, 1e-3, NO_STOP, 2, A_TRAIN, tuple(n_valid))


SIZE_CASES: List[EpochCase] = [size_case(s, b, mu, nv) for s in COMPACT_A_SHAPES + [GENERAL_SHAPE]
                               for b, mu in A_BATCHES for nv in A_VALID]

# -- Part B: epoch control -------------------------------------------------------------
B_SHAPE = (115, 27, 7)
B_TRAIN = (100, 40)     # at batch 12: 9 and 4 steps an epoch, either side of AV_CHECK
B_VALID = (129, 257)


def control_case(patience: int, lr: float = 3e-2, epochs: int = 8, shape=B_SHAPE, batch: int = 12, mu: float = 0.0,
                 n_train=B_TRAIN, n_valid=B_VALID, tag: str = "") -> EpochCase:
    return EpochCase("B", tuple(shape), batch, mu, lr, patience, epochs, tuple(n_train), tuple(n_valid), tag)


# name -> case.  ``p3`` and ``p2`` are the CPU probe's cases of the issue;
# ``p3-e6`` / ``p3-e5`` cut ``p3`` off at its later client's stop epoch and one
# before; ``p2r`` is the data on which a counter resets.
CONTROL: Dict[str, EpochCase] = {
    "p3": control_case(3),
    "p2": control_case(2),
    "p1": control_case(1),
    "p0": control_case(0),
    "p3-e6": control_case(3, epochs=6),
    "p3-e5": control_case(3, epochs=5),
    "p3-e1": control_case(3, epochs=1),
    "p2r": control_case(2, tag="reset"),
    "improving": control_case(2, lr=1e-2),
    "prox": control_case(2, mu=1e-3),
    "b33": control_case(2, batch=33, mu=1e-3, n_valid=(50, 129)),
    "general": control_case(2, shape=GENERAL_SHAPE),
}
CONTROL_CASES: List[EpochCase] = list(CONTROL.values())
ALL_CASES: List[EpochCase] = SIZE_CASES + CONTROL_CASES

# Seed of a data key whose seed-0 data puts an fp64 early-stop comparison
# inside O.DECISION_GAP, lets the fp32 oracle alone use more than half of a
# tolerance, or (Part B) does not show the decision pattern the case is there
# for: the first seed in 1..39 that clears all of it, with the smallest fp64
# gap / largest fp32 usage at the chosen seed (CPU figures).  Every other case
# runs at seed 0.
def _a_key(shape, batch, mu, n_valid):
    return size_case(shape, batch, mu, n_valid).data_key


SEEDS: Dict[tuple, int] = {
    # Part A is fair at seed 0 everywhere; at the seeds in use its smallest fp64
    # gap is 8.7e-03 and its largest fp32 usage 0.07.  These seeds are the first at which the single stale
    # row of n_valid 129 / 257 also moves the loss by twice the tolerance
    # (test_train_epochs.py, mistake (c)); behind each, that ratio at seed 0
    # and at the chosen seed.
    _a_key((115, 27, 7), 12, 0.0, (129, 255)): 1,      # 0.42 -> 1.23
    _a_key((115, 27, 7), 12, 0.0, (385, 129)): 8,      # 0.75 -> 1.25
    _a_key((115, 27, 7), 7, 0.0, (129, 255)): 1,       # 0.67 -> 1.71
    _a_key((46, 27, 7), 12, 0.0, (129, 255)): 5,       # 0.07 -> 1.07
    _a_key((46, 27, 7), 12, 0.0, (256, 257)): 6,       # 0.30 -> 1.13
    _a_key((46, 27, 7), 12, 0.0, (385, 129)): 3,       # 0.27 -> 1.27
    _a_key((46, 27, 7), 7, 0.0, (129, 255)): 5,        # 0.52 -> 2.23
    _a_key((46, 27, 7), 7, 0.0, (256, 257)): 35,       # 0.34 -> 1.13
    _a_key((46, 27, 7), 7, 0.0, (385, 129)): 1,        # 0.60 -> 2.55
    _a_key((120, 30, 10), 12, 0.0, (129, 255)): 10,    # 0.49 -> 1.17
    _a_key((120, 30, 10), 12, 0.0, (256, 257)): 5,     # 0.88 -> 1.38
    _a_key((120, 30, 10), 12, 0.0, (385, 129)): 16,    # 0.57 -> 1.02
    _a_key((120, 30, 10), 7, 0.0, (256, 257)): 5,      # 0.77 -> 1.43
    _a_key((120, 30, 10), 7, 0.0, (385, 129)): 1,      # 0.96 -> 1.08
    _a_key((120, 30, 10), 33, 1e-3, (385, 129)): 30,   # 0.37 -> 1.16
    # Part B.  Seed 0 is the issue's probe: at patience 3 client 0 never
    # improves after epoch 0 and stops after 4 epochs, client 1 has best epoch
    # 2 and stops after 6 (fp64 gap 7.6e-03, fp32 usage 0.14); at patience 2
    # they stop after 3 and 5.  No counter resets there, so ``p2r`` takes the
    # first fair seed on which one resets with epochs to go: at seed 10 client
    # 0 is worse in epochs 2 and 6 and better in 3 and 7, client 1 stops after
    # 7 epochs with best epoch 4 (gap 2.0e-02, usage 0.18).  Seeds 2, 3, 6, 8
    # and 9 are not fair: the fp32 oracle alone uses 0.6 to 3.6 of a tolerance
    # or a decision is inside the gap.  The FedProx, batch-33 and general cases
    # run at seed 0 (smallest gap of Part B 6.3e-03, at the general shape;
    # largest fp32 usage 0.18, adam_m of ``p2r``).
    control_case(2, tag="reset").data_key: 10,
}
# Part A sizes at which no seed in 0..39 lets the single stale row of mistake
# (c) move the loss by twice the tolerance (batch 33: the row shares its batch
# with 29 or 25 others): (shape, n_valid) -> the largest ratio over the seeds.
# They run at seed 0.  The helper-wave kernel validates these synchronously,
# from its current parameters: it has no second copy a tile could come from.
STALE_ROW_TOO_LIGHT: Dict[tuple, float] = {
    ((115, 27, 7), (129, 255)): 0.86, ((115, 27, 7), (256, 257)): 0.67, ((115, 27, 7), (385, 129)): 0.92,
    ((46, 27, 7), (129, 255)): 0.78, ((46, 27, 7), (256, 257)): 0.39, ((46, 27, 7), (385, 129)): 0.75,
    ((120, 30, 10), (129, 255)): 0.83, ((120, 30, 10), (256, 257)): 0.44,
}
STALE_ROW_BATCH = 33


def case_seed(case: EpochCase) -> int:
    return SEEDS.get(case.data_key, 0)


def case_id(case: EpochCase) -> str:
    d, h, z = case.shape
    if case.part == "A":
        return f"{d}x{h}x{z}-b{case.batch}-mu{case.mu:g}-v{case.n_valid[0]}+{case.n_valid[1]}"
    name = [k for k, v in CONTROL.items() if v == case]
    return name[0] if name else f"{d}x{h}x{z}-b{case.batch}-p{case.patience}-e{case.epochs}"


def hparams(case: EpochCase) -> TrainHParams:
    return TrainHParams(epochs=case.epochs, batch_size=case.batch, lr=case.lr, shrink_lambda=LAMBDA,
                        fedprox_mu=case.mu, patience=case.patience)


def is_general(shape) -> bool:
    return shape[1] > 27 or shape[2] > 7


def case_families(case: EpochCase) -> Tuple[str, ...]:
    """The kernel families a case runs on.  The helper-wave kernel validates
    asynchronously only in its plain instantiation (batch <= 12, no FedProx):
    only there is the synchronous tail another code path."""
    if is_general(case.shape):
        return ("general",)
    return tuple(f for f in COMPACT_FAMILIES if f != "hw_sync" or (case.batch <= 12 and case.mu == 0.0))


def validators_expected(case: EpochCase, family: str) -> bool:
    """Whether the launch carries one validator workgroup per trained client."""
    return family == "hw" and case.batch <= 12 and case.mu == 0.0


@functools.lru_cache(maxsize=None)
def epoch_case(case: EpochCase, seed: Optional[int] = None) -> O.Case:
    seed = case_seed(case) if seed is None else seed
    return O.make_case(ModelDims(*case.shape), case.n_train, case.n_valid, seed)


@functools.lru_cache(maxsize=None)
def trained(case: EpochCase, f64: bool, seed: Optional[int] = None) -> O.Trained:
    """The oracle's result on one case (``seed``: instead of the case's own),
    computed once per process and shared by every test that needs it
    (callers must not modify it)."""
    data = epoch_case(case, seed)
    eng = O.oracle(data.dims, data, data.anchor, f64)
    return O.snapshot(eng.store, eng.train(O.TRAINED, hparams(case)))


# -- what the tests read off a result ---------------------------------------------------
def valid_losses(t: O.Trained, row: int) -> List[float]:
    return [vl for _, vl in t.tracking[row]]


def worse_runs(losses) -> List[int]:
    """The patience counter after each epoch (0 where the epoch improved on
    the lowest loss before it)."""
    out, best, worse = [], float("inf"), 0
    for vl in losses:
        if vl < best:
            best, worse = vl, 0
        else:
            worse += 1
        out.append(worse)
    return out


def stopped_by_patience(case: EpochCase, t: O.Trained, row: int) -> bool:
    w = worse_runs(valid_losses(t, row))
    return w[-1] > 0 and w[-1] >= case.patience


def steps_per_epoch(case: EpochCase) -> Tuple[int, ...]:
    return tuple(-(-n // case.batch) for n in case.n_train)


# -- parameters as the tests' own numpy validation loss reads them -------------------------
def numpy_params(padded_row: torch.Tensor, dims: ModelDims) -> List[np.ndarray]:
    """w1, b1, .., w4, b4 of one padded store row as float64 arrays."""
    return [t.double().numpy() for t in unflatten(padded_to_canonical(padded_row, dims), dims)]


def prox_term(params_row: torch.Tensor, anchor_row: torch.Tensor, mu: float) -> float:
    d = params_row.double() - anchor_row.double()
    return float(mu * (d * d).sum())


# -- Part B's decision patterns -----------------------------------------------------------
# pattern -> the CONTROL cases whose fp64 decisions must show it (``shows``)
PATTERNS: Dict[str, Tuple[str, ...]] = {
    "snapshot-two-epochs-old": ("p2",),         # patience 2 stops with best_epoch == epochs_run - 3
    "three-worse-epochs": ("p3",),              # patience 3 stops after exactly three worse epochs
    "never-improves": ("p3", "p2"),             # no epoch after epoch 0 improves
    "counter-resets": ("p2r",),                 # patience >= 2: a worse epoch, then a better one, and on
    "last-epoch-best": ("improving",),          # all 8 epochs run, the last one the best
    "stop-on-the-limit": ("p3-e6",),            # the patience stop falls on the last allowed epoch
    "limit-one-short-of-stop": ("p3-e5",),      # the launch ends with worse == patience - 1
    "patience-0-as-1": ("p0",),                 # decides as patience 1 does
    "one-epoch": ("p3-e1",),
    "clients-stop-apart": ("p3",),              # two clients of one launch stop at different epochs
}


def shows(pattern: str, case: EpochCase, t: O.Trained) -> bool:
    """Whether the decisions in ``t`` (``epochs_run``, ``best_epoch`` and the
    validation losses) show ``pattern``."""
    rows = range(len(t.epochs_run))
    runs = [worse_runs(valid_losses(t, r)) for r in rows]
    er, be = t.epochs_run, t.best_epoch
    stopped = [stopped_by_patience(case, t, r) for r in rows]
    if pattern == "snapshot-two-epochs-old":
        return case.patience == 2 and any(stopped[r] and runs[r][-1] == 2 and be[r] == er[r] - 3 for r in rows)
    if pattern == "three-worse-epochs":
        return case.patience == 3 and any(stopped[r] and runs[r][-3:] == [1, 2, 3] for r in rows)
    if pattern == "never-improves":
        return any(er[r] > 1 and be[r] == 0 and runs[r] == list(range(er[r])) for r in rows)
    if pattern == "counter-resets":
        return case.patience >= 2 and any(
            a > 0 and b == 0 and er[r] > e + 2 for r in rows for e, (a, b) in enumerate(zip(runs[r], runs[r][1:])))
    if pattern == "last-epoch-best":
        return case.epochs == 8 and any(er[r] == 8 and be[r] == 7 for r in rows)
    if pattern == "stop-on-the-limit":
        return any(stopped[r] and er[r] == case.epochs and runs[r][-1] == case.patience for r in rows)
    if pattern == "limit-one-short-of-stop":
        return case.patience >= 2 and any(er[r] == case.epochs and runs[r][-1] == case.patience - 1 for r in rows)
    if pattern == "patience-0-as-1":
        one = trained(case._replace(patience=1), t.state["params"].dtype == torch.float64)
        return case.patience == 0 and (er, be, t.tracking) == (one.epochs_run, one.best_epoch, one.tracking) \
            and any(stopped)
    if pattern == "one-epoch":
        return case.epochs == 1 and all(er[r] == 1 and be[r] == 0 for r in rows)
    if pattern == "clients-stop-apart":
        return all(stopped) and er[0] != er[1] and max(er) < case.epochs
    raise KeyError(pattern)
