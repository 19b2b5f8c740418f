"""The training kernels at model shapes other than 115 / 27 / 7, against the
fp64 oracle of ``tests/oracle_f64.py``, and the scoring / utility kernels at
the same shapes (run with ``pytest -m gpu`` on an MI355X).

Kernel families: ``hw`` the helper-wave kernel (fedmx_train_hw.hip; with
asynchronous validation where the launcher applies it), ``hw_sync`` the same
with the synchronous epoch tail, ``c4`` the compact 4-wave kernel
(``helper=False``), ``general`` the identity-order 4-wave kernel the wider
shapes are routed to.  ``tests/test_train_shapes.py`` checks on the CPU that
every case's early-stop decisions are clear and that the fp32 oracle alone
uses at most half of each tolerance.

Baseline for later tolerance changes: the largest distance to the fp64 oracle
over a shape's cases, measured on an MI355X (kernels) and on the CPU (fp32
oracle), as absolute difference and, in brackets, as the fraction of
``atol + rtol * |ref|`` used (``oracle_f64.usage``; 1 would fail).  The test
prints the same figures per case (``DIST`` lines, ``pytest -s``).

  shape      family   params           tracking         adam_m           adam_v
  46/27/7    hw       3.0e-07 (0.002)  3.5e-07 (0.001)  2.6e-07 (0.022)  1.2e-06 (0.004)
  46/27/7    hw_sync  2.9e-07 (0.002)  2.6e-07 (0.000)  2.2e-07 (0.009)  8.8e-07 (0.003)
  46/27/7    c4       3.0e-07 (0.002)  4.7e-07 (0.001)  3.7e-07 (0.022)  1.2e-06 (0.004)
  46/27/7    fp32     9.5e-07 (0.008)  8.0e-07 (0.001)  2.0e-07 (0.036)  2.1e-08 (0.001)
  127/27/7   hw       3.8e-06 (0.010)  3.8e-07 (0.001)  2.8e-07 (0.024)  9.0e-07 (0.005)
  127/27/7   hw_sync  3.7e-06 (0.010)  3.6e-07 (0.001)  2.4e-07 (0.013)  6.5e-07 (0.004)
  127/27/7   c4       4.0e-06 (0.011)  3.8e-07 (0.001)  2.8e-07 (0.024)  9.0e-07 (0.005)
  127/27/7   fp32     2.9e-06 (0.008)  7.2e-07 (0.001)  3.6e-07 (0.039)  1.9e-08 (0.003)
  115/20/5   hw       1.2e-06 (0.013)  6.6e-07 (0.002)  3.5e-07 (0.051)  8.8e-07 (0.004)
  115/20/5   hw_sync  1.2e-06 (0.013)  5.7e-07 (0.002)  2.5e-07 (0.018)  5.7e-07 (0.003)
  115/20/5   c4       1.2e-06 (0.013)  6.9e-07 (0.002)  3.5e-07 (0.051)  8.8e-07 (0.003)
  115/20/5   fp32     1.1e-06 (0.012)  4.2e-07 (0.001)  3.2e-07 (0.057)  1.6e-08 (0.003)
  5/3/2      hw       1.5e-07 (0.000)  5.4e-07 (0.001)  5.6e-07 (0.004)  1.8e-06 (0.003)
  5/3/2      hw_sync  1.5e-07 (0.000)  4.3e-07 (0.001)  5.6e-07 (0.001)  1.3e-06 (0.003)
  5/3/2      c4       1.5e-07 (0.000)  5.4e-07 (0.001)  5.6e-07 (0.004)  1.8e-06 (0.003)
  5/3/2      fp32     1.5e-07 (0.000)  4.0e-07 (0.001)  4.0e-07 (0.003)  5.4e-08 (0.000)
  1/1/1      hw       1.3e-07 (0.000)  2.7e-07 (0.001)  2.9e-07 (0.000)  2.0e-06 (0.003)
  1/1/1      hw_sync  1.1e-07 (0.000)  1.8e-07 (0.001)  2.9e-07 (0.000)  6.2e-07 (0.003)
  1/1/1      c4       1.3e-07 (0.000)  2.7e-07 (0.001)  2.9e-07 (0.000)  2.0e-06 (0.003)
  1/1/1      fp32     1.3e-07 (0.000)  3.4e-07 (0.001)  3.3e-07 (0.000)  1.3e-08 (0.000)
  115/28/7   general  4.1e-06 (0.018)  4.3e-07 (0.001)  2.7e-07 (0.050)  9.0e-07 (0.004)
  115/28/7   fp32     2.0e-06 (0.009)  4.8e-07 (0.001)  2.8e-07 (0.055)  1.1e-08 (0.005)
  115/27/8   general  4.6e-06 (0.035)  6.6e-07 (0.001)  2.6e-07 (0.043)  8.3e-07 (0.003)
  115/27/8   fp32     3.7e-06 (0.029)  6.9e-07 (0.001)  3.0e-07 (0.045)  1.9e-08 (0.003)
  120/30/10  general  1.8e-06 (0.006)  4.6e-07 (0.001)  2.2e-07 (0.041)  4.7e-07 (0.004)
  120/30/10  fp32     1.6e-06 (0.005)  6.7e-07 (0.001)  2.0e-07 (0.038)  1.0e-08 (0.003)
  127/31/15  general  2.3e-06 (0.074)  6.9e-07 (0.001)  2.5e-07 (0.023)  9.8e-07 (0.003)
  127/31/15  fp32     3.0e-06 (0.061)  6.9e-07 (0.001)  1.7e-07 (0.028)  2.7e-08 (0.001)
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_f64 as O  # noqa: E402
from fedmse_decentralized_amd.engine.base import batch_mean_scores  # noqa: E402
from fedmse_decentralized_amd.engine.torch_engine import cen_score_numpy  # noqa: E402
from fedmse_decentralized_amd.models.layout import (P_PAD, ModelDims, canonical_to_padded, padded_index,  # noqa: E402
                                                    real_mask_padded)
from fedmse_decentralized_amd.models.reference import init_client_params, rowwise_sse  # noqa: E402
from fedmse_decentralized_amd.ops import _hip, _host  # noqa: E402

DEV = torch.device("cuda", 0)
FAMILY_KW = {"hw": dict(helper=True), "hw_sync": dict(helper=True, async_valid=False), "c4": dict(helper=False),
             "general": dict()}


def _hip_engine(case):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    return O.setup_engine(HipEngine(case.dims, DEV), case)


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


def _family_rows():
    rows = []
    for fam, shapes in (("hw", O.COMPACT_SHAPES), ("c4", O.COMPACT_SHAPES), ("general", O.GENERAL_SHAPES)):
        for row in O.grid_rows(shapes):
            rows.append((fam, row))
            # the helper-wave kernel validates asynchronously only in its plain
            # instantiation (batch <= 12, no FedProx): there, the synchronous tail too
            if fam == "hw" and row[1][0] <= 12 and row[1][1] == 0.0:
                rows.append(("hw_sync", row))
    return rows


@pytest.mark.parametrize("family,row", _family_rows(), ids=lambda v: v if isinstance(v, str) else O.row_id(v))
def test_train_kernel_matches_fp64_oracle(family, row):
    """Decisions, tracking, parameters, snapshot and Adam moments against the
    fp64 oracle at the default-shape test's tolerances; padding exactly zero;
    the untrained client's rows bit-unchanged."""
    shape, hp, sizes = row
    for si in sizes:
        case = O.grid_case(shape, si, hp)
        ref = O.trained_oracle(shape, si, hp, True)
        eng = _hip_engine(case)
        st = eng.store
        before = {n: getattr(st, n).clone() for n in O.STATE + ("adam_step", "anchor", "train", "valid")}
        grid0 = _hip.lib().fedmx_train_hw_last_grid()
        got = _launch(eng, O.hparams(*hp), **FAMILY_KW[family])
        what = f"{family} {shape} sizes {O.DATA_SIZES[si]} hp {hp}"
        dist = O.distances(got, ref)
        for name, (absd, use) in dist.items():   # the figures, before anything is asserted
            print(f"DIST {family} {shape} {si} {hp} {name} abs {absd:.3e} use {use:.4f}")
        if family == "general":   # the helper-wave launcher never ran
            assert _hip.lib().fedmx_train_hw_last_grid() == grid0, what
        elif family in ("hw", "hw_sync"):
            assert _hip.lib().fedmx_train_hw_last_grid() in (len(O.TRAINED), 2 * len(O.TRAINED)), what
        assert got.epochs_run == ref.epochs_run, what
        assert got.best_epoch == ref.best_epoch, what
        assert torch.equal(got.state["adam_step"], ref.state["adam_step"]), what
        rtol, atol = O.TOL["tracking"]
        np.testing.assert_allclose(np.array(got.tracking[0]), np.array(ref.tracking[0]), rtol=rtol, atol=atol,
                                   err_msg=what)
        np.testing.assert_allclose(np.array(got.tracking[1]), np.array(ref.tracking[1]), rtol=rtol, atol=atol,
                                   err_msg=what)
        for name in O.STATE:
            rtol, atol = O.TOL[name]
            assert got.state[name].dtype == torch.float32
            torch.testing.assert_close(got.state[name][O.TRAINED].double(), ref.state[name][O.TRAINED], rtol=rtol,
                                       atol=atol, msg=lambda m, n=name: f"{what} {n}: {m}")
        # padding exactly zero: a bias unit left behind on staging out, Adam moving a padded slot
        pad = ~real_mask_padded(case.dims)
        for name in O.STATE:
            assert torch.count_nonzero(got.state[name][:, pad]) == 0, f"{what}: {name} padding"
        # nothing of the untrained client moved, nor the anchor and the data of any client
        for name in O.STATE + ("adam_step",):
            assert torch.equal(getattr(st, name)[O.UNTRAINED], before[name][O.UNTRAINED]), f"{what}: untrained {name}"
        for name in ("anchor", "train", "valid"):
            assert torch.equal(getattr(st, name), before[name]), f"{what}: {name} written"


CROSS_SHAPES = [(46, 27, 7), (115, 20, 5), (5, 3, 2)]
CROSS_HP = [hp for hp in O.HPARAMS if hp[0] <= 12]


@pytest.mark.parametrize("hp", CROSS_HP, ids=lambda hp: f"b{hp[0]}-mu{hp[1]:g}")
@pytest.mark.parametrize("shape", CROSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_helper_waves_match_four_waves_bitwise_at_compact_shapes(shape, hp):
    """Batch <= 12: the helper-wave kernel and the compact 4-wave kernel give
    identical parameters, snapshots, moments and step counts over two
    consecutive launches (persistent Adam state); only the fp64 loss sums are
    grouped differently."""
    for si in range(len(O.DATA_SIZES)):
        case = O.grid_case(shape, si, hp)
        a, b = _hip_engine(case), _hip_engine(case)
        for launch in range(2):
            ra = _launch(a, O.hparams(*hp), helper=True)
            rb = _launch(b, O.hparams(*hp), helper=False)
            what = f"{shape} sizes {O.DATA_SIZES[si]} hp {hp} launch {launch}"
            assert ra.epochs_run == rb.epochs_run and ra.best_epoch == rb.best_epoch, what
            for ta, tb in zip(ra.tracking, rb.tracking):
                np.testing.assert_allclose(np.array(ta), np.array(tb), rtol=1e-9, atol=0, err_msg=what)
            for name in O.STATE + ("adam_step",):
                assert torch.equal(ra.state[name], rb.state[name]), f"{what}: {name}"


@pytest.mark.parametrize("hp", CROSS_HP, ids=lambda hp: f"b{hp[0]}-mu{hp[1]:g}")
@pytest.mark.parametrize("shape", CROSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compact_order_matches_identity_order_at_compact_shapes(shape, hp):
    """4-wave kernel, compact against identity order, at the tolerances of
    test_train_kernel_compact_order_matches_identity_order."""
    for si in range(len(O.DATA_SIZES)):
        case = O.grid_case(shape, si, hp)
        a, b = _hip_engine(case), _hip_engine(case)
        ra = _launch(a, O.hparams(*hp), helper=False, compact=True)
        rb = _launch(b, O.hparams(*hp), helper=False, compact=False)
        what = f"{shape} sizes {O.DATA_SIZES[si]} hp {hp}"
        assert ra.epochs_run == rb.epochs_run and ra.best_epoch == rb.best_epoch, what
        for ta, tb in zip(ra.tracking, rb.tracking):
            np.testing.assert_allclose(np.array(ta), np.array(tb), rtol=1e-5, atol=1e-7, err_msg=what)
        pad = ~real_mask_padded(case.dims)
        for name in O.STATE:
            torch.testing.assert_close(ra.state[name], rb.state[name], rtol=1e-3, atol=1e-6,
                                       msg=lambda m, n=name: f"{what} {n}: {m}")
            assert torch.count_nonzero(ra.state[name][:, pad]) == 0, f"{what}: {name} padding"
            assert torch.count_nonzero(rb.state[name][:, pad]) == 0, f"{what}: {name} padding (identity)"
        assert torch.equal(ra.state["adam_step"], rb.state["adam_step"]), what


# -- routing ----------------------------------------------------------------------
class _CaptureTrainArgs:
    """Stands in for the loaded library: ``fedmx_train`` keeps a copy of the
    TrainArgs ``_hip.train`` built (real store pointers) and launches nothing."""

    def __init__(self, real):
        self._real, self.args, self.k, self.stream = real, None, 0, None

    def __getattr__(self, name):
        return getattr(self._real, name)

    def fedmx_train(self, args, k, stream):
        self.args = _hip.TrainArgs.from_buffer_copy(args._obj)
        self.k, self.stream = k, stream
        return 0


def _captured_args(eng, hp, monkeypatch):
    real = _hip.lib()
    cap = _CaptureTrainArgs(real)
    with monkeypatch.context() as m:
        m.setattr(_hip, "_lib", cap)
        _hip.train(eng.store, O.TRAINED, hp, eng.dims, async_valid=False)
    assert cap.args is not None and cap.k == len(O.TRAINED)
    return real, cap


def _state(eng):
    torch.cuda.synchronize()
    _hip.runtime(DEV).sync()
    return {n: getattr(eng.store, n).clone() for n in O.STATE + ("adam_step",)}


@pytest.mark.parametrize("shape", O.GENERAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_helper_wave_launcher_refuses_general_shapes(shape, monkeypatch):
    case = O.grid_case(shape, 0, O.HPARAMS[0])
    eng = _hip_engine(case)
    real, cap = _captured_args(eng, O.hparams(*O.HPARAMS[0]), monkeypatch)
    real.fedmx_train_hw.argtypes = [ctypes.POINTER(_hip.TrainArgs), ctypes.c_int, ctypes.c_void_p]
    real.fedmx_train_hw.restype = ctypes.c_int
    before, grid0 = _state(eng), real.fedmx_train_hw_last_grid()
    assert (cap.args.d_in, cap.args.hidden, cap.args.latent) == shape
    assert real.fedmx_train_hw(ctypes.byref(cap.args), cap.k, cap.stream) == -4
    assert real.fedmx_train_hw_last_grid() == grid0
    after = _state(eng)
    assert all(torch.equal(before[n], after[n]) for n in before)


@pytest.mark.parametrize("shape", O.COMPACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compact_shapes_run_the_helper_wave_kernel(shape):
    """``fedmx_train_hw_last_grid`` follows the launches: k workgroups with
    asynchronous validation off, k or 2k (validators beside the trainers) with
    it on."""
    case = O.grid_case(shape, 0, O.HPARAMS[0])
    eng = _hip_engine(case)
    hp = O.hparams(*O.HPARAMS[0])
    L = _hip.lib()
    _launch(eng, hp, ids=[0], helper=True, async_valid=False)
    assert L.fedmx_train_hw_last_grid() == 1
    _launch(eng, hp, ids=O.TRAINED, helper=True, async_valid=True)
    assert L.fedmx_train_hw_last_grid() in (2, 4)
    _launch(eng, hp, ids=[1], helper=True, async_valid=False)
    assert L.fedmx_train_hw_last_grid() == 1
    _launch(eng, hp, ids=O.TRAINED, helper=True, async_valid=False)
    assert L.fedmx_train_hw_last_grid() == 2


@pytest.mark.parametrize("dims", [(128, 27, 7), (115, 32, 7), (115, 27, 16), (0, 27, 7), (115, 0, 7), (115, 27, 0)])
def test_out_of_range_dims_are_rejected(dims, monkeypatch):
    with pytest.raises(ValueError):
        ModelDims(*dims)
    case = O.grid_case((46, 27, 7), 0, O.HPARAMS[0])
    eng = _hip_engine(case)
    hp = O.hparams(*O.HPARAMS[0])
    real, cap = _captured_args(eng, hp, monkeypatch)
    before, grid0 = _state(eng), real.fedmx_train_hw_last_grid()
    cap.args.d_in, cap.args.hidden, cap.args.latent = dims
    assert real.fedmx_train(ctypes.byref(cap.args), cap.k, cap.stream) == -3
    with pytest.raises(ValueError, match="d_in 1..127"):
        _hip.train(eng.store, O.TRAINED, hp, SimpleNamespace(d_in=dims[0], hidden=dims[1], latent=dims[2]))
    # rejected before any kernel started
    assert real.fedmx_train_hw_last_grid() == grid0
    after = _state(eng)
    assert all(torch.equal(before[n], after[n]) for n in before)


@pytest.mark.parametrize("shape", [(46, 27, 7), (127, 31, 15)], ids=lambda s: "x".join(map(str, s)))
def test_batch_zero_is_rejected(shape, monkeypatch):
    case = O.grid_case(shape, 0, O.HPARAMS[0])
    eng = _hip_engine(case)
    real, cap = _captured_args(eng, O.hparams(*O.HPARAMS[0]), monkeypatch)
    before, grid0 = _state(eng), real.fedmx_train_hw_last_grid()
    for batch in (0, -5):
        cap.args.batch = batch
        assert real.fedmx_train(ctypes.byref(cap.args), cap.k, cap.stream) == -2
    with pytest.raises(ValueError, match="batch_size"):
        _hip.train(eng.store, O.TRAINED, O.hparams(0, 0.0, 5.0), eng.dims)
    assert real.fedmx_train_hw_last_grid() == grid0
    after = _state(eng)
    assert all(torch.equal(before[n], after[n]) for n in before)


# -- scoring and utility kernels at the same shapes ---------------------------------
def _engine(dims):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    return HipEngine(ModelDims(*dims), DEV)


@pytest.mark.parametrize("latent", [1, 8, 15])
def test_cen_scores_other_latent_widths(latent):
    """Regular data, a one-row train set (variance 0 on every dimension: the
    scale-1 branch) and one constant train feature, against cen_score_numpy."""
    rng = np.random.default_rng(20 + latent)
    eng = _engine((46, 27, latent))
    te = (rng.normal(size=(391, latent)) * 5).astype(np.float32)
    tr_full = (rng.normal(size=(683, latent)) * 3 + 1).astype(np.float32)
    tr_one = tr_full[:1].copy()
    tr_const = tr_full.copy()
    tr_const[:, latent // 2] = np.float32(1.7)
    trains = [tr_full, tr_one, tr_const]
    out = eng.cen_scores([torch.from_numpy(t).to(DEV) for t in trains], [torch.from_numpy(te).to(DEV)] * 3)
    torch.cuda.synchronize()
    for t, o in zip(trains, out):
        np.testing.assert_allclose(o.cpu().numpy(), cen_score_numpy(t, te), rtol=1e-12, atol=1e-12)
    # the one-row fit is distance to that row, unscaled
    d = (te - tr_one).astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(out[1].cpu().numpy(), np.sqrt((d * d).sum(1)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n", [2, 3, 170])
@pytest.mark.parametrize("d_in", [1, 46, 127])
def test_standardize_ddof1_other_widths_and_row_counts(d_in, n):
    g = torch.Generator().manual_seed(100 * d_in + n)
    x = torch.zeros(n, 128)
    x[:, :d_in] = torch.randn(n, d_in, generator=g) * 4.0 + 2.0
    x[:, 127] = 1.0   # the stores' bias column: not a feature at any width
    y = _hip.standardize_ddof1(x.to(DEV), d_in).cpu()
    xr = x[:, :d_in].double()
    ref = (xr - xr.mean(0)) / (xr.std(0) + 1e-8)
    torch.testing.assert_close(y[:, :d_in].double(), ref, rtol=1e-5, atol=1e-5)
    assert torch.count_nonzero(y[:, d_in:]) == 0


@pytest.mark.parametrize("dims", [(46, 27, 7), (127, 31, 15)], ids=lambda s: "x".join(map(str, s)))
def test_param_drift_other_shapes(dims):
    md = ModelDims(*dims)
    g = torch.Generator().manual_seed(31)
    canon = torch.randn(5, md.num_params, generator=g)
    stack = canonical_to_padded(canon, md)
    eng = _engine(dims)
    d = eng.param_drift(stack[:4].to(DEV), stack[4].to(DEV))
    _, segs = padded_index(md)
    diff = canon[:4].double() - canon[4].double()
    ref = sum(torch.linalg.vector_norm(diff[:, s:e], dim=1) for s, e in segs)
    torch.testing.assert_close(d.cpu().double(), ref, rtol=1e-5, atol=1e-5)
    # padded slots belong to no tensor: whatever they hold is not counted
    dirty = stack.clone()
    dirty[:, ~real_mask_padded(md)] = torch.randn(5, int((~real_mask_padded(md)).sum()), generator=g)
    d2 = eng.param_drift(dirty[:4].to(DEV), dirty[4].to(DEV))
    assert torch.equal(d2, d)


@pytest.mark.parametrize("dims", [(46, 27, 7), (127, 31, 15)], ids=lambda s: "x".join(map(str, s)))
def test_score_reduce_other_shapes(dims):
    """The 1 / d_in scale: batch-mean score and overall MSE of forward SSEs,
    against fp64 computed from the canonical parameters, and of given SSE
    vectors against their own fp64 sums."""
    md = ModelDims(*dims)
    params, _ = init_client_params(1, 5, md)
    g = torch.Generator().manual_seed(6)
    xs = []
    for n in (1, 5, 300):
        x = torch.zeros(n, 128)
        x[:, :md.d_in] = torch.randn(n, md.d_in, generator=g)
        xs.append(x.to(DEV))
    pad = canonical_to_padded(params, md).to(DEV)
    sse, _ = _hip.forward_rows(pad, [(0, x) for x in xs], md, True, False)
    batches = [0, 7, 128]
    red = _hip.score_reduce(sse, batches, md.d_in)
    _hip.runtime(DEV).sync()
    red = np.array(red)
    for i, (x, s, bs) in enumerate(zip(xs, sse, batches)):
        # the kernel's reduction of the fp32 SSEs it was given: fp64 sums
        vote, mse = batch_mean_scores(s, bs or (1 << 30), md.d_in)
        np.testing.assert_allclose(red[i], [vote, mse], rtol=1e-12, atol=0)
        # forward + reduction against fp64: every row's SSE is within the forward
        # tests' 2e-5 * sse + 1e-5, so the means are within 2e-5 * mean + 1e-5 / d_in
        rs, _ = rowwise_sse(params[0].double(), x[:, :md.d_in].cpu().double(), md)
        vote64, mse64 = batch_mean_scores(rs, bs or (1 << 30), md.d_in)
        np.testing.assert_allclose(red[i], [vote64, mse64], rtol=2e-5, atol=1e-5 / md.d_in)


def _auc_numpy(s, y):
    """Mann-Whitney with ties counted 1/2, from the definition."""
    s = np.asarray(s, dtype=np.float64)
    pos, neg = s[y != 0], np.sort(s[y == 0])
    if len(pos) == 0 or len(neg) == 0:
        return float("nan")
    less = np.searchsorted(neg, pos, side="left").astype(np.float64)
    leq = np.searchsorted(neg, pos, side="right").astype(np.float64)
    return float((less.sum() + 0.5 * (leq - less).sum()) / (len(pos) * len(neg)))


def _auc_both(eng, s, y):
    st, yt = torch.from_numpy(s).to(DEV), torch.from_numpy(y.astype(np.int32)).to(DEV)
    raw = _hip.auc([st], [yt])
    _hip.runtime(DEV).sync()
    raw = float(raw[0])
    return raw, float(eng.auc([st], [yt])[0])


def test_auc_edges():
    eng = _engine((115, 27, 7))
    rng = np.random.default_rng(8)
    # a single class: undefined
    for lab in (0, 1):
        raw, got = _auc_both(eng, rng.normal(size=9), np.full(9, lab))
        assert np.isnan(raw) and np.isnan(got)
    # n = 2
    for s, want in (([0.1, 0.7], 1.0), ([0.7, 0.1], 0.0), ([0.3, 0.3], 0.5)):
        raw, got = _auc_both(eng, np.array(s), np.array([0, 1]))
        assert raw == want and got == want
    # all scores tied
    y = rng.integers(0, 2, size=777)
    raw, got = _auc_both(eng, np.full(777, 2.5), y)
    assert raw == 0.5 and got == 0.5
    # NaN / +-inf scores read as numpy.nan_to_num reads them, in both score types
    s = rng.normal(size=500)
    s[::7], s[1::11], s[2::13] = np.nan, np.inf, -np.inf
    y = rng.integers(0, 2, size=500)
    for dt in (np.float64, np.float32):
        sd = s.astype(dt)
        want = _host.roc_auc(np.nan_to_num(sd.astype(np.float64)), y)
        assert abs(want - _auc_numpy(np.nan_to_num(sd.astype(np.float64)), y)) < 1e-12
        raw, got = _auc_both(eng, sd, y)
        assert abs(raw - want) < 1e-12 and abs(got - want) < 1e-12


@pytest.mark.parametrize("small,on_device", [(8192, True), (8193, False)])
@pytest.mark.parametrize("small_is_positive", [True, False])
def test_auc_at_the_lds_sort_limit(small, on_device, small_is_positive):
    """The smaller class at exactly the 8192 keys the LDS sort holds, and one
    more: there the kernel answers -1 and engine.auc returns the host value."""
    eng = _engine((115, 27, 7))
    rng = np.random.default_rng(small)
    y = np.r_[np.full(small, int(small_is_positive)), np.full(small + 9, int(not small_is_positive))]
    rng.shuffle(y)
    s = np.round(rng.normal(size=len(y)) + 0.3 * y, 2)   # ties
    want = _host.roc_auc(s, y)
    assert abs(want - _auc_numpy(s, y)) < 1e-12
    raw, got = _auc_both(eng, s, y)
    assert (raw != -1.0) == on_device
    if on_device:
        assert abs(raw - want) < 1e-12
    assert abs(got - want) < 1e-12
