"""CPU side of the training-shape grid (``tests/oracle_f64.py``): what has to
hold for the GPU tests of ``test_train_shapes_gpu.py`` to be fair.

The GPU tests assert that the kernels take the fp64 oracle's early-stop
decisions and stay within the project's fp32 tolerances of it.  Here, for
every case of the same grid: the fp32 and the fp64 oracle decide alike, every
pair of validation losses the early stop compares is ``DECISION_GAP`` apart
in fp64 (no coin toss), and the fp32 oracle alone uses at most half of each
tolerance, so the other half is the kernels'.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_f64 as O  # noqa: E402
from fedmse_decentralized_amd.models.layout import ModelDims, real_mask_padded  # noqa: E402

ROWS = O.grid_rows(O.ALL_SHAPES)


@pytest.mark.parametrize("row", ROWS, ids=O.row_id)
def test_oracles_agree_and_decisions_are_clear(row):
    shape, hp, sizes = row
    for si in sizes:
        f32 = O.trained_oracle(shape, si, hp, False)
        f64 = O.trained_oracle(shape, si, hp, True)
        what = f"{shape} sizes {O.DATA_SIZES[si]} hp {hp}"
        assert f64.state["params"].dtype == torch.float64 and f32.state["params"].dtype == torch.float32
        assert f64.state["adam_step"].dtype == torch.int32
        assert f32.epochs_run == f64.epochs_run, what
        assert f32.best_epoch == f64.best_epoch, what
        assert torch.equal(f32.state["adam_step"], f64.state["adam_step"]), what
        # one Adam step per batch of every epoch run; the untrained client none
        n_train = O.DATA_SIZES[si][0]
        steps = [e * -(-n // hp[0]) for e, n in zip(f64.epochs_run, n_train)] + [0]
        assert f64.state["adam_step"].tolist() == steps, what
        gaps = O.decision_gaps(f64.tracking)
        assert all(g >= O.DECISION_GAP for g in gaps), (what, gaps)
        for name, (absd, use) in O.distances(f32, f64).items():
            assert use <= 0.5, (what, name, absd, use)


def test_grid_covers_the_issue_shapes_and_edges():
    """The grid itself: both kernel families' shapes, the data-size edges and
    every launcher split (batch <= 12 / <= 16 / larger, FedProx or not)."""
    assert all(h <= 27 and z <= 7 for _, h, z in O.COMPACT_SHAPES)
    assert all(h > 27 or z > 7 for _, h, z in O.GENERAL_SHAPES)
    assert (115, 28, 7) in O.GENERAL_SHAPES and (115, 27, 8) in O.GENERAL_SHAPES   # one past each boundary
    for s in O.ALL_SHAPES:
        ModelDims(*s)
    batches = {hp[0] for hp in O.HPARAMS}
    assert any(b <= 12 for b in batches) and any(12 < b <= 16 for b in batches) and any(b > 16 for b in batches)
    assert {hp[1] != 0 for hp in O.HPARAMS} == {True, False}
    sizes = [n for nt, _ in O.DATA_SIZES for n in nt]
    assert 1 in sizes and any(n % 12 == 0 for n in sizes) and any(n < 7 for n in sizes)
    assert 1 in [n for _, nv in O.DATA_SIZES for n in nv]
    fam = {tuple(r[0]) in O.COMPACT_SHAPES for r in O.LAMBDA0_ROWS}
    assert fam == {True, False} and all(r[1][2] == 0.0 for r in O.LAMBDA0_ROWS)


@pytest.mark.parametrize("shape", [(46, 27, 7), (127, 31, 15), (1, 1, 1)])
def test_case_and_anchor_keep_padding_zero(shape):
    case = O.make_case(shape, (5, 24), (3, 12), seed=0)
    pad = ~real_mask_padded(case.dims)
    assert len(case.train) == 3 and case.init.shape[0] == 3
    assert [t.shape for t in case.train] == [(5, shape[0]), (24, shape[0]), (O.UNTRAINED_ROWS[0], shape[0])]
    assert torch.count_nonzero(case.anchor[:, pad]) == 0
    eng = O.oracle(case.dims, case, case.anchor, True)
    assert torch.count_nonzero(eng.store.params[:, pad]) == 0
    # the anchor is non-trivial at every real position's tensor, and shared
    assert not torch.equal(eng.store.anchor.float(), eng.store.params.float())
    assert torch.equal(O.make_case(shape, (5, 24), (3, 12), seed=0).anchor, case.anchor)


def test_oracle_padding_and_untrained_rows():
    """The oracle itself leaves padding zero and the untrained client alone
    (the GPU tests assert the same of the kernels)."""
    shape, hp = (46, 27, 7), O.HPARAMS[1]
    case = O.grid_case(shape, 0, hp)
    got = O.trained_oracle(shape, 0, hp, True)
    pad = ~real_mask_padded(case.dims)
    fresh = O.oracle(case.dims, case, case.anchor, True).store
    for name in O.STATE:
        assert torch.count_nonzero(got.state[name][:, pad]) == 0, name
        assert torch.equal(got.state[name][O.UNTRAINED], getattr(fresh, name)[O.UNTRAINED]), name
    assert np.isfinite(np.array(got.tracking[0])).all()
