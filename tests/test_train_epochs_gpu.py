"""The training launch's validation pass and early stop against the fp64
oracle, at validation-set sizes on the edges of the kernels' validation loops
(Part A) and over the decision patterns of the patience rule (Part B); cases
and seeds in ``tests/train_epochs_oracle.py`` (run with ``pytest -m gpu`` on
an MI355X).  Families as in ``test_train_shapes_gpu.py``: ``hw`` the
helper-wave kernel (with validator workgroups at batch <= 12 without FedProx,
which the tests assert through ``fedmx_train_hw_last_grid``), ``hw_sync`` the
same with the synchronous epoch tail, ``c4`` the compact-shape 4-wave kernel,
``general`` the identity-order 4-wave kernel.  ``tests/test_train_epochs.py``
checks on the CPU that every case's decisions are clear, that the fp32 oracle
alone uses at most half of each tolerance, and that a dropped row, a wrongly
weighted last batch or a stale tile would move the loss out of tolerance.

Which case reaches which branch (n_valid, per client):

  15 / 16 / 17     one tile, full and one row short; the second tile (wave 1 validates)
  48 / 49, b12     4-wave kernels: four batches, one per wave; a fifth sends wave 0 round
                   ``for (vb = w; vb < nvb; vb += 4)`` again, for a batch of one row
  50, b33          4-wave kernels: a last batch of 17 rows, the chunk loop's second
                   chunk holds one row; helper-wave kernel: a batch over three tiles
  b16 / b33 / b64  4-wave kernels: the chunk loop over a validation batch (b33, b64);
                   helper-wave kernel: its synchronous multi-chunk instantiation
  127 / 128        eight tiles, one per wave, the last one row short and full
  129              a ninth tile: epoch_tail's ``vt += 8`` second pass on wave 0; the
                   validator's second preloaded tile ``vx1`` (wave 0 alone)
  255 / 256        sixteen tiles: ``vx1`` on every wave
  257              a seventeenth: the validator's reload loop ``vt = w8 + 16``
  385              25 tiles: wave 0 reloads twice (tiles 16 and 24)
  b7               batches straddle the tiles unevenly: ``(row / B) * B`` and
                   ``min(B, n - start)`` differ from row to row of a tile
  p3, p2, ...      the patience rule: ``train_epochs_oracle.PATTERNS``; epochs of 9
                   and 4 steps, so one client's stop is met at the check before step
                   AV_CHECK and rolls back mid-epoch, the other's at an epoch's end

Baseline for later tolerance changes: the largest distance to the fp64 oracle
over a (part, shape, family)'s cases, as absolute difference and, in brackets,
as the fraction of ``atol + rtol * |ref|`` used (``oracle_f64.usage``; 1 would
fail).  The kernel rows were measured on an MI355X, the fp32 rows are the fp32
oracle on the CPU.  The tests print the same figures per case (``DIST``
lines, ``pytest -s``).

  part  shape      family   params           tracking         adam_m           adam_v
  A     115/27/7   hw       6.0e-06 (0.033)  2.8e-07 (0.000)  2.5e-07 (0.020)  9.3e-07 (0.004)
  A     115/27/7   hw_sync  6.0e-06 (0.033)  2.8e-07 (0.000)  2.5e-07 (0.020)  9.3e-07 (0.004)
  A     115/27/7   c4       6.0e-06 (0.033)  3.8e-07 (0.000)  2.5e-07 (0.020)  9.3e-07 (0.004)
  A     115/27/7   fp32     1.3e-05 (0.070)  5.6e-07 (0.001)  1.6e-07 (0.033)  1.6e-08 (0.003)
  A     46/27/7    hw       6.0e-08 (0.001)  2.9e-07 (0.000)  2.8e-07 (0.044)  7.6e-07 (0.004)
  A     46/27/7    hw_sync  6.0e-08 (0.001)  2.9e-07 (0.000)  2.8e-07 (0.044)  7.6e-07 (0.004)
  A     46/27/7    c4       6.0e-08 (0.001)  2.9e-07 (0.000)  2.8e-07 (0.044)  7.6e-07 (0.004)
  A     46/27/7    fp32     1.0e-06 (0.008)  5.1e-07 (0.001)  1.8e-07 (0.016)  1.5e-08 (0.002)
  A     120/30/10  general  1.9e-06 (0.018)  4.5e-07 (0.001)  3.2e-07 (0.022)  8.9e-07 (0.006)
  A     120/30/10  fp32     7.3e-06 (0.050)  9.9e-07 (0.001)  7.2e-07 (0.061)  1.9e-08 (0.016)
  B     115/27/7   hw       8.4e-06 (0.060)  3.9e-06 (0.009)  2.1e-06 (0.152)  3.8e-06 (0.004)
  B     115/27/7   hw_sync  2.1e-06 (0.060)  3.9e-06 (0.009)  2.1e-06 (0.152)  2.8e-06 (0.004)
  B     115/27/7   c4       1.8e-05 (0.063)  3.9e-06 (0.009)  2.1e-06 (0.152)  4.0e-06 (0.005)
  B     115/27/7   fp32     1.9e-05 (0.068)  2.4e-06 (0.007)  2.8e-06 (0.179)  7.1e-07 (0.007)
  B     120/30/10  general  1.3e-06 (0.018)  6.7e-07 (0.001)  1.2e-06 (0.093)  1.3e-06 (0.004)
  B     120/30/10  fp32     3.4e-06 (0.031)  9.2e-07 (0.002)  1.9e-06 (0.074)  8.3e-08 (0.002)
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_f64 as O  # noqa: E402
import train_epochs_oracle as E  # noqa: E402
from fedmse_decentralized_amd.models.layout import real_mask_padded  # noqa: E402
from fedmse_decentralized_amd.ops import _hip  # noqa: E402

DEV = torch.device("cuda", 0)
EVERYTHING = O.STATE + ("adam_step",)
READ_ONLY = ("anchor", "train", "valid")


@functools.lru_cache(maxsize=None)
def kernel_run(family: str, case: E.EpochCase) -> SimpleNamespace:
    """One launch of ``case`` on ``family``, read back after a sync: the result
    as ``O.Trained``, the whole tracking buffer, the helper-wave launcher's
    grid before and after, and what the launch left of the rows it must not
    write.  Run once per process and shared (callers must not modify it)."""
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    data = E.epoch_case(case)
    eng = O.setup_engine(HipEngine(data.dims, DEV), data)
    st = eng.store
    before = {n: getattr(st, n).clone() for n in EVERYTHING + READ_ONLY}
    grid0 = _hip.lib().fedmx_train_hw_last_grid()
    trk, er, be = _hip.train(st, list(O.TRAINED), E.hparams(case), eng.dims, **E.FAMILY_KW[family])
    torch.cuda.synchronize()
    _hip.runtime(DEV).sync()
    grid = _hip.lib().fedmx_train_hw_last_grid()
    er, be, trk = [int(e) for e in er], [int(b) for b in be], np.array(trk, dtype=np.float64, copy=True)
    assert min(er) >= 0, f"training launch failed: epochs_run {er}"
    res = SimpleNamespace(epochs_run=er, best_epoch=be,
                          tracking=[[(float(trk[i, e, 0]), float(trk[i, e, 1])) for e in range(er[i])]
                                    for i in range(len(er))])
    untouched = {n: torch.equal(getattr(st, n)[O.UNTRAINED], before[n][O.UNTRAINED]) for n in EVERYTHING}
    untouched.update({n: torch.equal(getattr(st, n), before[n]) for n in READ_ONLY})
    return SimpleNamespace(got=O.snapshot(st, res), tracking=trk, grid0=grid0, grid=grid, untouched=untouched)


def check_against_oracle(family: str, case: E.EpochCase):
    """The assertions of test_train_kernel_matches_fp64_oracle, and that the
    tracking entries of epochs not run still hold the launcher's NaN."""
    ref = E.trained(case, True)
    run = kernel_run(family, case)
    got = run.got
    what = f"{family} {E.case_id(case)}"
    for name, (absd, use) in O.distances(got, ref).items():   # the figures, before anything is asserted
        print(f"DIST {case.part} {family} {case.shape} {E.case_id(case)} {name} abs {absd:.3e} use {use:.4f}")
    k = len(O.TRAINED)
    if family == "general":   # the helper-wave launcher never ran
        assert run.grid == run.grid0, what
    elif family in ("hw", "hw_sync"):   # validator workgroups beside the trainers exactly where expected
        assert run.grid == (2 * k if E.validators_expected(case, family) else k), what
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
    # padding exactly zero
    pad = ~real_mask_padded(E.epoch_case(case).dims)
    for name in O.STATE:
        assert torch.count_nonzero(got.state[name][:, pad]) == 0, f"{what}: {name} padding"
    # nothing of the untrained client moved, nor the anchor and the data of any client
    for name, same in run.untouched.items():
        assert same, f"{what}: {name} written"
    # epochs at or past epochs_run: still the NaN the launcher filled in (a
    # trainer that ran ahead of its validator and was rolled back leaves nothing)
    assert run.tracking.shape == (k, case.epochs, 2), what
    for i in range(k):
        assert np.isfinite(run.tracking[i, :got.epochs_run[i]]).all(), what
        assert np.isnan(run.tracking[i, got.epochs_run[i]:]).all(), f"{what}: client {i} wrote past its last epoch"


def _size_rows():
    """(family, shape, (batch, mu)): every validation-size pair in one test."""
    rows = []
    for shape in E.COMPACT_A_SHAPES + [E.GENERAL_SHAPE]:
        for b, mu in E.A_BATCHES:
            for fam in E.case_families(E.size_case(shape, b, mu, E.A_VALID[0])):
                rows.append((fam, shape, (b, mu)))
    return rows


def _row_id(v):
    if isinstance(v, str):
        return v
    return "x".join(map(str, v)) if len(v) == 3 else f"b{v[0]}-mu{v[1]:g}"


@pytest.mark.parametrize("family,shape,bmu", _size_rows(), ids=_row_id)
def test_validation_sizes_match_fp64_oracle(family, shape, bmu):
    """Part A: two epochs, nothing stops; the validation sets sit on the tile,
    batch and chunk edges of the validation loops."""
    for n_valid in E.A_VALID:
        check_against_oracle(family, E.size_case(shape, bmu[0], bmu[1], n_valid))


def _control_rows():
    return [(fam, name) for name, case in E.CONTROL.items() for fam in E.case_families(case)]


@pytest.mark.parametrize("family,name", _control_rows())
def test_epoch_control_matches_fp64_oracle(family, name):
    """Part B: the stop epoch, the best epoch and the snapshot that far behind
    the final parameters, over the decision patterns of the patience rule."""
    case = E.CONTROL[name]
    check_against_oracle(family, case)
    got, ref = kernel_run(family, case).got, E.trained(case, True)
    for pattern, names in E.PATTERNS.items():   # the kernel's own decisions show the pattern too
        if name in names and pattern != "patience-0-as-1":
            assert E.shows(pattern, case, got), (family, name, pattern)
    # the snapshot is the best epoch's model, not the last one's, wherever they differ
    for row in O.TRAINED:
        last = ref.best_epoch[row] == ref.epochs_run[row] - 1
        assert torch.equal(got.state["best"][row], got.state["params"][row]) == last, (family, name, row)


@pytest.mark.parametrize("family", E.COMPACT_FAMILIES)
def test_patience_zero_is_patience_one_bitwise(family):
    """``worse >= patience && worse > 0``: patience 0 stops where patience 1
    does, with identical tracking, state and step counts."""
    a, b = kernel_run(family, E.CONTROL["p0"]), kernel_run(family, E.CONTROL["p1"])
    assert a.got.epochs_run == b.got.epochs_run and a.got.best_epoch == b.got.best_epoch
    assert max(a.got.epochs_run) < E.CONTROL["p0"].epochs   # both clients stopped
    assert np.array_equal(a.tracking, b.tracking, equal_nan=True)
    for name in EVERYTHING:
        assert torch.equal(a.got.state[name], b.got.state[name]), name


def _cross_cases():
    return [c for c in E.ALL_CASES if not E.is_general(c.shape) and c.batch <= 12]


@pytest.mark.parametrize("case", _cross_cases(), ids=E.case_id)
def test_families_agree_bitwise_at_compact_shapes(case):
    """Batch <= 12: the helper-wave kernel (asynchronous and synchronous epoch
    tail) and the compact 4-wave kernel give identical state and step counts;
    only the fp64 loss sums are grouped differently (the terms of
    test_helper_waves_match_four_waves_bitwise_at_compact_shapes)."""
    fams = E.case_families(case)
    assert fams[0] == "hw" and len(fams) >= 2
    ra = kernel_run("hw", case).got
    for fam in fams[1:]:
        rb = kernel_run(fam, case).got
        what = f"{E.case_id(case)}: hw against {fam}"
        assert ra.epochs_run == rb.epochs_run and ra.best_epoch == rb.best_epoch, what
        for ta, tb in zip(ra.tracking, rb.tracking):
            np.testing.assert_allclose(np.array(ta), np.array(tb), rtol=1e-9, atol=0, err_msg=what)
        for name in EVERYTHING:
            assert torch.equal(ra.state[name], rb.state[name]), f"{what}: {name}"
