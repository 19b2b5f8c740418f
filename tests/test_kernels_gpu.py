"""Numerics of the hand-written gfx950 kernels vs plain PyTorch fp32/fp64
references of the same ops (run with ``pytest -m gpu`` on an MI355X)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.engine.base import TrainHParams
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine, cen_score_numpy
from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS, P_PAD, canonical_to_padded, padded_to_canonical
from fedmse_decentralized_amd.models.reference import init_client_params, rowwise_sse
from fedmse_decentralized_amd.ops import _hip, _host

DEV = torch.device("cuda", 0)


def _engine():
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    return HipEngine(DEFAULT_DIMS, DEV)


def _data(n, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, 128)
    x[:, :115] = torch.randn(n, 115, generator=g) * scale
    return x


def test_native_library_is_loaded():
    import ctypes

    L = _hip.lib()
    assert isinstance(L, ctypes.CDLL)
    assert "libfedmx_hip.so" in L._name


def test_mfma_f32_16x16x4_lane_layout():
    D = _hip.probe_mfma(DEV)
    i = np.arange(16)
    A = i[:, None] + 100.0 * np.arange(4)[None, :]
    B = 1000.0 * np.arange(4)[:, None] + i[None, :]
    assert np.array_equal(D, A @ B)


def test_forward_rows_matches_torch():
    params, _ = init_client_params(3, 7)
    params = params + 0.05 * torch.randn(params.shape, generator=torch.Generator().manual_seed(1))
    pad = canonical_to_padded(params).to(DEV)
    xs = [_data(n, seed=n).to(DEV) for n in (1, 17, 300, 12)]
    items = [(0, xs[0]), (1, xs[1]), (2, xs[2]), (1, xs[3])]
    sse, lat = _hip.forward_rows(pad, items, DEFAULT_DIMS, True, True)
    for (row, x), s, z in zip(items, sse, lat):
        rs, rz = rowwise_sse(params[row].double(), x[:, :115].cpu().double())
        torch.testing.assert_close(s.cpu().double(), rs, rtol=2e-5, atol=1e-5)
        torch.testing.assert_close(z.cpu().double(), rz, rtol=2e-5, atol=1e-5)


@pytest.mark.parametrize("dims", [(46, 27, 7), (115, 20, 5), (120, 30, 10), (127, 27, 7),
                                  # around the compact order's input columns 113 / 114 (one real, one
                                  # padding; neither), and the first shape past each compact bound
                                  (112, 27, 7), (113, 27, 7), (114, 27, 7), (116, 27, 7), (115, 28, 7), (115, 27, 8)])
def test_forward_rows_other_shapes_match_torch(dims):
    """Shapes other than the reference's: the compact forward order (d_in <=
    115, hidden <= 27, latent <= 7) and the identity-order fallback (wider
    models) both match the fp64 reference, SSE and latents; row counts on
    both sides of one 16-row tile and of one 64-row block."""
    from fedmse_decentralized_amd.models.layout import ModelDims

    md = ModelDims(*dims)
    params, _ = init_client_params(2, 11, md)
    params = params + 0.05 * torch.randn(params.shape, generator=torch.Generator().manual_seed(3))
    pad = canonical_to_padded(params, md).to(DEV)
    g = torch.Generator().manual_seed(4)
    xs = []
    for n in (5, 40, 257, 15, 16, 17, 63, 64, 65):
        x = torch.zeros(n, 128)
        x[:, :md.d_in] = torch.randn(n, md.d_in, generator=g)
        xs.append(x.to(DEV))
    items = [(0, xs[0]), (1, xs[1]), (0, xs[2])] + [(i % 2, x) for i, x in enumerate(xs[3:])]
    sse, lat = _hip.forward_rows(pad, items, md, True, True)
    for (row, x), s, z in zip(items, sse, lat):
        rs, rz = rowwise_sse(params[row].double(), x[:, :md.d_in].cpu().double(), md)
        torch.testing.assert_close(s.cpu().double(), rs, rtol=2e-5, atol=1e-5)
        torch.testing.assert_close(z.cpu().double(), rz, rtol=2e-5, atol=1e-5)


def test_weighted_sum_and_drift():
    g = torch.Generator().manual_seed(2)
    stack = canonical_to_padded(torch.randn(5, DEFAULT_DIMS.num_params, generator=g)).to(DEV)
    w = [0.1, 0.3, 0.2, 0.25, 0.15]
    out = _hip.weighted_sum(stack, w)
    ref = torch.zeros(P_PAD)
    for k in range(5):
        ref = ref + stack[k].cpu() * torch.tensor(w[k], dtype=torch.float32)
    assert torch.equal(out.cpu(), ref)
    eng = _engine()
    d = eng.param_drift(stack[:3], stack[4])
    tref = TorchEngine(DEFAULT_DIMS, torch.device("cpu")).param_drift(stack[:3].cpu(), stack[4].cpu())
    torch.testing.assert_close(d.cpu(), tref, rtol=1e-5, atol=1e-5)


def test_standardize_ddof1():
    x = (_data(170, seed=3, scale=4.0) + 2.0)
    x[:, 115:] = 0
    y = _hip.standardize_ddof1(x.to(DEV), 115).cpu()
    xr = x[:, :115].double()
    ref = (xr - xr.mean(0)) / (xr.std(0) + 1e-8)
    torch.testing.assert_close(y[:, :115].double(), ref, rtol=1e-5, atol=1e-5)
    assert torch.count_nonzero(y[:, 115:]) == 0


def test_cen_scores_and_auc():
    rng = np.random.default_rng(4)
    tr = (rng.normal(size=(680, 7)) * 3 + 1).astype(np.float32)
    te = (rng.normal(size=(3900, 7)) * 5).astype(np.float32)
    eng = _engine()
    out = eng.cen_scores([torch.from_numpy(tr).to(DEV)], [torch.from_numpy(te).to(DEV)])[0].cpu().numpy()
    ref = cen_score_numpy(tr, te)
    np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12)
    y = rng.integers(0, 2, size=3900).astype(np.int32)
    s = np.round(out + y * 0.5, 1)  # ties
    got = eng.auc([torch.from_numpy(s).to(DEV)], [torch.from_numpy(y).to(DEV)])
    assert abs(got[0] - _host.roc_auc(s, y)) < 1e-12
    s32 = torch.from_numpy(s.astype(np.float32)).to(DEV)
    got32 = eng.auc([s32], [torch.from_numpy(y).to(DEV)])
    assert abs(got32[0] - _host.roc_auc(s.astype(np.float32).astype(np.float64), y)) < 1e-12


def _setup_pair(n_train=(53, 40), n_valid=(14, 9), seed=0):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    rng = np.random.default_rng(seed)
    tr = [rng.normal(size=(n, 115)).astype(np.float32) for n in n_train]
    va = [rng.normal(size=(n, 115)).astype(np.float32) for n in n_valid]
    te = [rng.normal(size=(20, 115)).astype(np.float32) for _ in n_train]
    lab = [np.r_[np.zeros(10), np.ones(10)].astype(np.int64) for _ in n_train]
    init, _ = init_client_params(len(n_train), seed)
    ref = TorchEngine(DEFAULT_DIMS, torch.device("cpu"))
    ref.setup(tr, va, te, lab, init)
    hip = HipEngine(DEFAULT_DIMS, DEV)
    hip.setup(tr, va, te, lab, init)
    return ref, hip


@pytest.mark.parametrize("lam,mu,batch", [(5.0, 0.0, 12), (0.0, 0.0, 12), (5.0, 0.001, 12), (10.0, 0.0, 16),
                                          (1.0, 0.01, 7), (5.0, 0.0, 33), (5.0, 0.001, 64), (5.0, 0.0, 128)])
def test_train_kernel_matches_torch_engine(lam, mu, batch):
    ref, hip = _setup_pair()
    # non-trivial FedProx anchor
    anchor = ref.store.params + 0.01 * torch.randn(ref.store.params.shape, generator=torch.Generator().manual_seed(5))
    anchor = canonical_to_padded(padded_to_canonical(anchor))
    ref.store.anchor.copy_(anchor)
    hip.store.anchor.copy_(anchor.to(DEV))
    hp = TrainHParams(epochs=3, batch_size=batch, lr=1e-3, shrink_lambda=lam, fedprox_mu=mu, patience=1)
    r1 = ref.train([0, 1], hp)
    r2 = hip.train([0, 1], hp)
    assert list(r1.epochs_run) == list(r2.epochs_run)
    assert list(r1.best_epoch) == list(r2.best_epoch)
    for a, b in zip(r1.tracking, r2.tracking):
        np.testing.assert_allclose(np.array(b), np.array(a), rtol=2e-4, atol=1e-6)
    torch.testing.assert_close(hip.store.params.cpu(), ref.store.params, rtol=2e-3, atol=2e-5)
    torch.testing.assert_close(hip.store.best.cpu(), ref.store.best, rtol=2e-3, atol=2e-5)
    torch.testing.assert_close(hip.store.adam_m.cpu(), ref.store.adam_m, rtol=5e-3, atol=1e-6)
    torch.testing.assert_close(hip.store.adam_v.cpu(), ref.store.adam_v, rtol=5e-3, atol=1e-9)
    assert torch.equal(hip.store.adam_step.cpu(), ref.store.adam_step)
    # padding stays exactly zero
    from fedmse_decentralized_amd.models.layout import real_mask_padded

    pad = ~real_mask_padded().to(DEV)
    assert torch.count_nonzero(hip.store.params[:, pad]) == 0


@pytest.mark.parametrize("batch,lam,mu", [(12, 5.0, 0.0), (7, 1.0, 0.001), (1, 5.0, 0.0), (12, 0.0, 0.01)])
def test_train_kernel_compact_order_matches_identity_order(batch, lam, mu):
    """The compact internal order (padded hidden / latent / batch k-steps
    skipped) computes the same training as the identity order up to fp32
    summation order."""
    from fedmse_decentralized_amd.models.layout import real_mask_padded

    _, a = _setup_pair(seed=11)
    _, b = _setup_pair(seed=11)
    anchor = a.store.params + 0.01 * torch.randn(a.store.params.shape, generator=torch.Generator().manual_seed(6),
                                                 device="cpu").to(DEV)
    anchor = canonical_to_padded(padded_to_canonical(anchor.cpu())).to(DEV)
    a.store.anchor.copy_(anchor)
    b.store.anchor.copy_(anchor)
    hp = TrainHParams(epochs=3, batch_size=batch, lr=1e-3, shrink_lambda=lam, fedprox_mu=mu, patience=1)
    ta, ea, ba = _hip.train(a.store, [0, 1], hp, a.dims, compact=True)
    tb, eb, bb = _hip.train(b.store, [0, 1], hp, b.dims, compact=False)
    torch.cuda.synchronize()
    _hip.runtime(DEV).sync()
    assert list(ea) == list(eb) and list(ba) == list(bb)
    np.testing.assert_allclose(np.array(ta), np.array(tb), rtol=1e-5, atol=1e-7)
    for name in ("params", "best", "adam_m", "adam_v"):
        torch.testing.assert_close(getattr(a.store, name), getattr(b.store, name), rtol=1e-3, atol=1e-6)
    pad = ~real_mask_padded().to(DEV)
    for name in ("params", "best", "adam_m", "adam_v"):
        assert torch.count_nonzero(getattr(a.store, name)[:, pad]) == 0


@pytest.mark.parametrize("batch,lam,mu,epochs,patience", [(12, 5.0, 0.0, 4, 1), (7, 1.0, 0.001, 3, 1),
                                                           (1, 5.0, 0.0, 2, 1), (12, 0.0, 0.01, 5, 10 ** 6)])
def test_train_kernel_helper_waves_match_four_waves(batch, lam, mu, epochs, patience):
    """The helper-wave kernel (fedmx_train_hw.hip: W4's gradient and Adam on a
    second wave per SIMD, validation over 8 waves) performs the same per-element
    operations as the 4-wave compact kernel: identical parameters, optimizer
    state, snapshots and early-stop decisions; only the fp64 loss sums are
    grouped differently."""
    _, a = _setup_pair(seed=13)
    _, b = _setup_pair(seed=13)
    anchor = a.store.params + 0.01 * torch.randn(a.store.params.shape, generator=torch.Generator().manual_seed(7),
                                                 device="cpu").to(DEV)
    anchor = canonical_to_padded(padded_to_canonical(anchor.cpu())).to(DEV)
    a.store.anchor.copy_(anchor)
    b.store.anchor.copy_(anchor)
    hp = TrainHParams(epochs=epochs, batch_size=batch, lr=1e-3, shrink_lambda=lam, fedprox_mu=mu, patience=patience)
    for _ in range(2):   # second launch: persistent Adam state and step counts
        ta, ea, ba = _hip.train(a.store, [0, 1], hp, a.dims, helper=True)
        tb, eb, bb = _hip.train(b.store, [0, 1], hp, b.dims, helper=False)
        torch.cuda.synchronize()
        _hip.runtime(DEV).sync()
        assert list(ea) == list(eb) and list(ba) == list(bb)
        np.testing.assert_allclose(np.array(ta), np.array(tb), rtol=1e-9, atol=1e-12)
        for name in ("params", "best", "adam_m", "adam_v", "adam_step"):
            assert torch.equal(getattr(a.store, name), getattr(b.store, name)), name


@pytest.mark.parametrize("batch,lam,mu", [(64, 5.0, 0.0), (33, 1.0, 0.001), (13, 5.0, 0.0), (128, 0.0, 0.01)])
def test_train_kernel_helper_waves_multi_chunk_batches(batch, lam, mu):
    """Batches over 12 rows on the helper-wave kernel (16-row chunks, weight
    gradients accumulated over a batch's chunks, one Adam step per batch)
    against the 4-wave kernel (also 16-row chunks): the same training up to
    the fp32 summation order of the two kernels' products (VERDICT r3 Next
    #7; the kernel-vs-oracle test covers batch 16 / 33 / 64 / 128 too)."""
    _, a = _setup_pair(n_train=(301, 150), n_valid=(70, 33), seed=17)
    _, b = _setup_pair(n_train=(301, 150), n_valid=(70, 33), seed=17)
    anchor = a.store.params + 0.01 * torch.randn(a.store.params.shape, generator=torch.Generator().manual_seed(8),
                                                 device="cpu").to(DEV)
    anchor = canonical_to_padded(padded_to_canonical(anchor.cpu())).to(DEV)
    a.store.anchor.copy_(anchor)
    b.store.anchor.copy_(anchor)
    hp = TrainHParams(epochs=3, batch_size=batch, lr=1e-3, shrink_lambda=lam, fedprox_mu=mu, patience=10 ** 6)
    for _ in range(2):   # second launch: persistent Adam state and step counts
        ta, ea, ba = _hip.train(a.store, [0, 1], hp, a.dims, helper=True)
        tb, eb, bb = _hip.train(b.store, [0, 1], hp, b.dims, helper=False)
        torch.cuda.synchronize()
        _hip.runtime(DEV).sync()
        assert list(ea) == list(eb) and list(ba) == list(bb)
        np.testing.assert_allclose(np.array(ta), np.array(tb), rtol=1e-5, atol=1e-7)
        for name in ("params", "best", "adam_m", "adam_v"):
            torch.testing.assert_close(getattr(a.store, name), getattr(b.store, name), rtol=1e-3, atol=1e-6)
        assert torch.equal(a.store.adam_step, b.store.adam_step)


def test_train_kernel_single_step_tight():
    # one Adam step from identical state: errors are pure fp32 rounding
    ref, hip = _setup_pair(n_train=(12,), n_valid=(12,), seed=3)
    hp = TrainHParams(epochs=1, batch_size=12, lr=1e-3, shrink_lambda=5.0, patience=1)
    ref.train([0], hp)
    hip.train([0], hp)
    torch.testing.assert_close(hip.store.params.cpu(), ref.store.params, rtol=1e-4, atol=1e-6)


def test_train_kernel_many_clients_concurrently():
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    rng = np.random.default_rng(9)
    C = 40
    tr = [rng.normal(size=(int(rng.integers(20, 80)), 115)).astype(np.float32) for _ in range(C)]
    va = [rng.normal(size=(int(rng.integers(5, 20)), 115)).astype(np.float32) for _ in range(C)]
    te = [rng.normal(size=(10, 115)).astype(np.float32) for _ in range(C)]
    lab = [np.r_[np.zeros(5), np.ones(5)].astype(np.int64) for _ in range(C)]
    init, _ = init_client_params(C, 1)
    hip = HipEngine(DEFAULT_DIMS, DEV)
    hip.setup(tr, va, te, lab, init)
    hp = TrainHParams(epochs=2, batch_size=12, lr=1e-3, shrink_lambda=5.0, patience=1)
    sel = list(range(0, C, 3))
    res = hip.train(sel, hp)
    # each client's result equals training it alone
    solo = HipEngine(DEFAULT_DIMS, DEV)
    solo.setup(tr, va, te, lab, init)
    for c in sel[:4]:
        solo.train([c], hp)
        assert torch.equal(solo.store.params[c], hip.store.params[c])
    untouched = [c for c in range(C) if c not in sel]
    assert torch.equal(hip.store.params[untouched].cpu(), canonical_to_padded(init[untouched]))


def test_copy_rows_gather_scatter():
    """Row copies through mapped index arrays (multi-rank exchange packing)."""
    rt = _hip.runtime(DEV)
    src = torch.randn(9, 40, device=DEV)
    dst = torch.zeros(6, 40, device=DEV)
    sidx, didx = rt.desc.put(np.array([8, 0, 3], dtype=np.int32), np.array([5, 1, 2], dtype=np.int32))
    _hip.copy_rows(dst.data_ptr(), 40, didx, src.data_ptr(), 40, sidx, 3, 40, DEV)
    # identity destination, row length shorter than the stride
    dst2 = torch.zeros(3, 40, device=DEV)
    _hip.copy_rows(dst2.data_ptr(), 40, 0, src.data_ptr(), 40, sidx, 3, 16, DEV)
    torch.cuda.synchronize()
    ref = torch.zeros(6, 40)
    ref[5], ref[1], ref[2] = src[8].cpu(), src[0].cpu(), src[3].cpu()
    assert torch.equal(dst.cpu(), ref)
    assert torch.equal(dst2[:, :16].cpu(), src[[8, 0, 3], :16].cpu())
    assert torch.count_nonzero(dst2[:, 16:]) == 0


def test_forward_rows_independent_of_block_length():
    params, _ = init_client_params(2, 3)
    pad = canonical_to_padded(params).to(DEV)
    x = _data(1000, seed=9).to(DEV)
    outs = []
    for rpb in (64, 256, 1024):
        desc = _hip.build_fwd_desc(pad.data_ptr() + 4 * P_PAD * np.array([0, 1]), np.array([x.data_ptr()] * 2),
                                   np.array([1000, 700]), np.zeros(2, np.int64), np.zeros(2, np.int64),
                                   DEFAULT_DIMS, rows_per_block=rpb)
        assert desc["nrows"].max() <= rpb
    sse_a, _ = _hip.forward_rows(pad, [(0, x), (1, x[:700])], DEFAULT_DIMS, True, False)
    import os
    os.environ["FEDMX_FWD_ROWS_PER_BLOCK"] = "64"
    try:
        sse_b, _ = _hip.forward_rows(pad, [(0, x), (1, x[:700])], DEFAULT_DIMS, True, False)
    finally:
        del os.environ["FEDMX_FWD_ROWS_PER_BLOCK"]
    for a, b in zip(sse_a, sse_b):
        assert torch.equal(a, b)


def test_device_event_orders_two_streams():
    """_hiprt.DeviceEvent (fence-less: the round's kernel-only stream
    dependencies, engine/device_round.py): a side-stream copy waiting on it
    sees what the main stream's kernels wrote before the record, every time
    the one event is re-recorded."""
    from fedmse_decentralized_amd.ops import _hiprt

    ev = _hiprt.DeviceEvent()
    main = torch.cuda.current_stream(DEV)
    side = torch.cuda.Stream(DEV)
    big = torch.empty(1 << 24, device=DEV)
    src = torch.zeros(1 << 20, device=DEV)
    outs = []
    for it in range(20):
        big.fill_(float(it))        # keeps the main stream busy (~64 MB write)
        src.fill_(float(it + 1))    # the value the side stream must see
        ev.record(main.cuda_stream)
        out = torch.empty_like(src)
        with torch.cuda.stream(side):
            ev.wait(side.cuda_stream)
            out.copy_(src)
        outs.append(out)
        main.wait_stream(side)      # the next fill_ of src comes after the copy
    torch.cuda.synchronize()
    for it, out in enumerate(outs):
        assert bool((out == float(it + 1)).all()), it


def test_side_wait_returns_on_the_word_and_times_out_without_it():
    """side_wait_kernel (the round's evaluation waiting on verify_split's
    hand-off word, engine/device_round.py): it returns once the word reaches
    the sequence number (wrap-safe), and without the word it gives up after
    its timeout and sets the host-visible status word."""
    from fedmse_decentralized_amd.ops import _hiprt

    khz = _hip.lib().fedmx_ipc_wall_khz()
    ticks_per_ms = khz if khz > 0 else 100_000
    status = _hiprt.MappedBuffer(64)
    view = status.view(0, np.int32, 1)
    word = torch.zeros(2, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    for stored, seq in ((7, 7), (9, 7), (-2, 0xFFFFFFFE), (1, 0xFFFFFFFF)):   # reached (the last two across the wrap)
        view[0] = 0
        word[1] = stored
        torch.cuda.synchronize()
        _hip.side_wait(word.data_ptr() + 4, seq, status.dev_ptr, 1000 * ticks_per_ms, side.cuda_stream)
        side.synchronize()
        assert int(view[0]) == 0, (stored, seq)
    view[0] = 0
    word[1] = 5
    torch.cuda.synchronize()
    _hip.side_wait(word.data_ptr() + 4, 6, status.dev_ptr, 20 * ticks_per_ms, side.cuda_stream)   # never reached
    side.synchronize()
    assert int(view[0]) == 1
