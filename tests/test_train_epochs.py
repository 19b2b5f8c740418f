"""CPU side of the validation-size and epoch-control cases
(``tests/train_epochs_oracle.py``): what has to hold for the GPU tests of
``test_train_epochs_gpu.py`` to be fair, and to have teeth.

Fair, for every case: the fp32 and the fp64 oracle decide alike, every pair of
validation losses the early stop compares is ``DECISION_GAP`` apart in fp64,
and the fp32 oracle alone uses at most half of each tolerance.

Teeth, Part A: the validation loss is written out below in plain numpy
(``numpy_valid_loss``) and reproduces what the fp64 oracle tracked.  It is
then recomputed with one mistake a kernel's validation loop could make, and
each must move the loss by more than twice the tracking tolerance
``atol + rtol * |loss|``, or a kernel that made it would still pass:
(a) any single row dropped from its batch sum; (b) the last batch's rows
weighted with ``1 / B`` instead of ``1 / bt``, where these differ; (c) in
epoch 2, the rows of tiles >= 8, and of tiles >= 16, computed from the
parameters of epoch 1.  (a), (b) and (c) hold at every size with more than
one stale row.  Where the stale tile carries a single row, n_valid 129 (tiles
>= 8) and 257 (tiles >= 16), that row must carry enough of the loss: it does
at batch 16 and 64 (it is a batch of its own), and at batch 12 and 7 at the
seeds recorded in ``train_epochs_oracle.SEEDS``.  At batch 33 the row is one
of 30 or 26 in its batch and no seed in 0..39 reaches twice the tolerance at
eight of the nine sizes: ``train_epochs_oracle.STALE_ROW_TOO_LIGHT`` holds the
best ratio of each (0.39 to 0.92).  Those sizes stay in the grid for what (a)
and (b) see at them.

Teeth, Part B: every decision pattern of ``train_epochs_oracle.PATTERNS`` is
read from the fp64 oracle's ``epochs_run``, ``best_epoch`` and validation
losses, by name.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_f64 as O  # noqa: E402
import train_epochs_oracle as E  # noqa: E402
from fedmse_decentralized_amd.models.layout import ModelDims  # noqa: E402


def check_fair(case, seed=None):
    """Same decisions and step counts, clear decisions, fp32 within half.
    Returns (smallest fp64 decision gap, largest fp32 usage)."""
    f32, f64 = E.trained(case, False, seed), E.trained(case, True, seed)
    what = E.case_id(case)
    assert f64.state["params"].dtype == torch.float64 and f32.state["params"].dtype == torch.float32
    assert f32.epochs_run == f64.epochs_run, what
    assert f32.best_epoch == f64.best_epoch, what
    assert torch.equal(f32.state["adam_step"], f64.state["adam_step"]), what
    steps = [e * s for e, s in zip(f64.epochs_run, E.steps_per_epoch(case))] + [0]
    assert f64.state["adam_step"].tolist() == steps, what
    gaps = O.decision_gaps(f64.tracking)
    assert all(g >= O.DECISION_GAP for g in gaps), (what, gaps)
    dist = O.distances(f32, f64)
    for name, (absd, use) in dist.items():
        assert use <= 0.5, (what, name, absd, use)
    return min(gaps, default=float("inf")), max(use for _, use in dist.values())


@pytest.mark.parametrize("case", E.ALL_CASES, ids=E.case_id)
def test_oracles_agree_and_decisions_are_clear(case):
    check_fair(case)
    f64 = E.trained(case, True)
    assert all(1 <= e <= case.epochs for e in f64.epochs_run)
    if case.part == "A":   # nothing stops: epoch 2 validates moved parameters
        assert f64.epochs_run == (2, 2)


# -- Part A: the validation loss in plain numpy -------------------------------------------
def row_losses(params, x, lam=E.LAMBDA):
    """Per validation row: SSE / d_in + lambda * ||z||, in float64."""
    w1, b1, w2, b2, w3, b3, w4, b4 = params
    x = x.astype(np.float64)
    h1 = np.maximum(x @ w1.T + b1, 0.0)
    z = h1 @ w2.T + b2
    h3 = np.maximum(z @ w3.T + b3, 0.0)
    y = h3 @ w4.T + b4
    return ((y - x) ** 2).sum(1) / x.shape[1] + lam * np.sqrt((z * z).sum(1))


def row_weights(n, batch, every_batch_full=False):
    """Each row's share of the mean over batches of the batch means:
    1 / bt(its batch) / nvb.  ``every_batch_full``: mistake (b), 1 / B."""
    nvb = -(-n // batch)
    bt = np.minimum(batch, n - (np.arange(n) // batch) * batch)
    return 1.0 / (np.full(n, batch) if every_batch_full else bt) / nvb


def numpy_valid_loss(params, x, batch):
    """The mean over the batches of each batch's mean row loss, batch by batch."""
    rows = row_losses(params, x)
    means = [rows[s:s + batch].mean() for s in range(0, len(rows), batch)]
    return float(np.mean(means))


def teeth(case, seed=None):
    """Per mistake, the smallest |change of the loss| / (2 x tracking tolerance)
    over both clients (and both epochs); > 1 is a mistake the GPU test sees.
    Absent where the mistake changes nothing (a full last batch, no such tile)."""
    assert case.part == "A" and case.epochs == 2
    data = E.epoch_case(case, seed)
    dims = ModelDims(*case.shape)
    runs = [E.trained(case._replace(epochs=1), True, seed), E.trained(case, True, seed)]
    rtol, atol = O.TOL["tracking"]
    out = {}

    def note(name, change, loss):
        ratio = abs(change) / (2.0 * (atol + rtol * abs(loss)))
        out[name] = min(out.get(name, float("inf")), ratio)

    for row in O.TRAINED:
        x, n, B = data.valid[row], case.n_valid[row], case.batch
        w = row_weights(n, B)
        assert abs(w.sum() - 1.0) < 1e-12
        per_epoch = []
        for ep, run in enumerate(runs):
            assert run.epochs_run[row] == ep + 1
            params = E.numpy_params(run.state["params"][row], dims)
            rows = row_losses(params, x)
            prox = E.prox_term(run.state["params"][row], data.anchor[row], case.mu)
            loss = numpy_valid_loss(params, x, B) + prox
            # the weighted form is the batch-by-batch form, and both are the oracle's value
            assert abs(float(rows @ w) + prox - loss) <= 1e-12 * abs(loss)
            tracked = runs[1].tracking[row][ep][1]
            assert abs(loss - tracked) <= 1e-10 * abs(tracked), (E.case_id(case), row, ep, loss, tracked)
            per_epoch.append(rows)
            note("a: one row dropped", float((rows * w).min()), loss)
            if n % B:
                note("b: last batch as a full one", float(rows @ (w - row_weights(n, B, True))), loss)
            if ep == 1:
                for tile0 in (8, 16):
                    stale = np.arange(n) >= E.TILE * tile0
                    if stale.any():
                        change = float(((per_epoch[0] - per_epoch[1]) * w)[stale].sum())
                        name = f"c: tiles >= {tile0} stale"
                        note(name + (" (one row)" if stale.sum() == 1 else ""), change, loss)
    return out


def _too_light(case):
    return case.batch == E.STALE_ROW_BATCH and (case.shape, case.n_valid) in E.STALE_ROW_TOO_LIGHT


@pytest.mark.parametrize("case", E.SIZE_CASES, ids=E.case_id)
def test_validation_mistakes_would_show(case):
    got = teeth(case)
    assert "a: one row dropped" in got
    assert ("b: last batch as a full one" in got) == any(n % case.batch for n in case.n_valid)
    for t in (8, 16):
        assert (f"c: tiles >= {t} stale" in got) == any(n > E.TILE * t + 1 for n in case.n_valid)
        assert (f"c: tiles >= {t} stale (one row)" in got) == any(n == E.TILE * t + 1 for n in case.n_valid)
    for name, ratio in got.items():
        if name.endswith("(one row)") and _too_light(case):
            # on record as out of reach, and no better than the record says
            assert ratio <= E.STALE_ROW_TOO_LIGHT[(case.shape, case.n_valid)] < 1.0, (E.case_id(case), name, ratio)
        else:
            assert ratio > 1.0, (E.case_id(case), name, ratio)


def test_too_light_sizes_are_batch_33_single_rows():
    cases = {(c.shape, c.n_valid) for c in E.SIZE_CASES if c.batch == E.STALE_ROW_BATCH}
    assert set(E.STALE_ROW_TOO_LIGHT) <= cases
    assert all(any(n in (129, 257) for n in nv) for _, nv in E.STALE_ROW_TOO_LIGHT)


# -- Part B: the decision patterns ---------------------------------------------------------
@pytest.mark.parametrize("pattern", sorted(E.PATTERNS))
def test_fp64_decisions_show_the_pattern(pattern):
    for name in E.PATTERNS[pattern]:
        case = E.CONTROL[name]
        f64 = E.trained(case, True)
        assert E.shows(pattern, case, f64), (pattern, name, f64.epochs_run, f64.best_epoch,
                                             [E.worse_runs(E.valid_losses(f64, r)) for r in O.TRAINED])
        # and the fp32 oracle shows it too (it decides alike)
        assert E.shows(pattern, case, E.trained(case, False)), (pattern, name)


def test_cut_off_cases_are_the_base_case_cut_off():
    """``p3-e6`` / ``p3-e5`` / ``p3-e1`` share ``p3``'s data and trajectory:
    each epoch they run is bit for bit ``p3``'s, and the limits are the later
    client's stop epoch and one before."""
    base = E.trained(E.CONTROL["p3"], True)
    assert max(base.epochs_run) == E.CONTROL["p3-e6"].epochs == E.CONTROL["p3-e5"].epochs + 1
    for name in ("p3-e6", "p3-e5", "p3-e1"):
        case = E.CONTROL[name]
        assert case.data_key == E.CONTROL["p3"].data_key
        cut = E.trained(case, True)
        for row in O.TRAINED:
            assert cut.epochs_run[row] == min(base.epochs_run[row], case.epochs)
            assert cut.tracking[row] == base.tracking[row][:cut.epochs_run[row]]


def test_worse_runs_and_pattern_reader():
    assert E.worse_runs([3.0, 4.0, 2.0, 2.0, 5.0, 1.0]) == [0, 1, 0, 1, 2, 0]
    with pytest.raises(KeyError):
        E.shows("no such pattern", E.CONTROL["p3"], E.trained(E.CONTROL["p3"], True))
    # a pattern is not shown by a case that lacks it
    assert not E.shows("last-epoch-best", E.CONTROL["p3"], E.trained(E.CONTROL["p3"], True))
    assert not E.shows("never-improves", E.CONTROL["improving"], E.trained(E.CONTROL["improving"], True))


# -- the grid itself -------------------------------------------------------------------------
def test_grid_covers_the_issue_boundaries_and_patterns():
    A = E.SIZE_CASES
    assert all(c.epochs == 2 and c.patience == E.NO_STOP and c.lr == 1e-3 for c in A)
    fams = {f for c in E.ALL_CASES for f in E.case_families(c)}
    assert fams == {"hw", "hw_sync", "c4", "general"}
    assert {c.shape for c in A} == {(115, 27, 7), (46, 27, 7), (120, 30, 10)}
    assert {(c.batch, c.mu) for c in A} == {(12, 0.0), (7, 0.0), (16, 0.0), (33, 1e-3), (64, 0.0)}

    def sizes(family, batch=None, validators=None):
        return {n for c in A for f in E.case_families(c) if f == family and (batch is None or c.batch == batch)
                and (validators is None or E.validators_expected(c, f) == validators) for n in c.n_valid}

    every = {15, 16, 17, 48, 49, 50, 127, 128, 129, 255, 256, 257, 385}
    # the tile edges of epoch_tail: hw_sync, and hw wherever it validates synchronously
    assert every <= sizes("hw_sync") and every <= sizes("hw", validators=False)
    # the validator workgroup's three regimes: vx0 only, vx1, the reload loop once and twice
    assert every <= sizes("hw", validators=True)
    for b in (12, 7):
        assert every <= sizes("hw", batch=b, validators=True)
    # the 4-wave kernels: a second pass over batches (n_valid > 4 B) and its
    # edge at batch 12; a validation batch of more than one chunk, with a
    # one-row last chunk at batch 33
    for fam in ("c4", "general"):
        assert {48, 49} <= sizes(fam, batch=12) and every <= sizes(fam)
        assert 50 in sizes(fam, batch=33) and 50 % 33 == E.TILE + 1
        assert any(n > 4 * 64 for n in sizes(fam, batch=64))
    # a last batch of exactly one row, per family
    for fam in fams:
        assert any(n % c.batch == 1 for c in A if fam in E.case_families(c) for n in c.n_valid)
    # hw_sync only where validators would otherwise run
    for c in E.ALL_CASES:
        assert ("hw_sync" in E.case_families(c)) == (not E.is_general(c.shape) and c.batch <= 12 and c.mu == 0.0)
        assert E.is_general(c.shape) == (E.case_families(c) == ("general",))
        ModelDims(*c.shape)
    # Part B: eight epochs, every patience, both learning rates, epochs either
    # side of the asynchronous check interval, Part A's sizes at batch 12
    B = E.CONTROL
    assert {c.patience for c in B.values()} == {0, 1, 2, 3}
    assert {c.lr for c in B.values()} == {3e-2, 1e-2}
    assert all(c.epochs == 8 for n, c in B.items() if "-e" not in n)
    for c in B.values():
        if c.batch == 12:
            assert c.n_valid == (129, 257)
            steps = E.steps_per_epoch(c)
            assert min(steps) < E.AV_CHECK < max(steps)
    assert set(E.PATTERNS) == {"snapshot-two-epochs-old", "three-worse-epochs", "never-improves", "counter-resets",
                               "last-epoch-best", "stop-on-the-limit", "limit-one-short-of-stop", "patience-0-as-1",
                               "one-epoch", "clients-stop-apart"}
    assert all(n in B for names in E.PATTERNS.values() for n in names)
    assert B["prox"].mu == 1e-3 and B["prox"].batch == 12 and set(E.case_families(B["prox"])) == {"hw", "c4"}
    assert B["b33"].batch == 33 and set(E.case_families(B["b33"])) == {"hw", "c4"}
    assert E.case_families(B["general"]) == ("general",) and B["general"].shape == (120, 30, 10)
    for n in ("p3", "p2", "p1", "p0", "p2r", "improving"):
        assert E.case_families(B[n]) == E.COMPACT_FAMILIES and B[n].shape == (115, 27, 7)
    # every seed on record belongs to a case that runs
    assert set(E.SEEDS) <= {c.data_key for c in E.ALL_CASES} and all(1 <= s <= 39 for s in E.SEEDS.values())
    assert len(set(E.ALL_CASES)) == len(E.ALL_CASES)
