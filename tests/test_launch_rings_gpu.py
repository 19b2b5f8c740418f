"""The launch rings (ops/_hiprt.py) under live launches: ``fedmx_detect``
launches of tiny clients on a private ``Runtime`` (1 MiB rings) while plain
torch matmuls keep its stream busy, against the numpy oracle of
tests/test_detection_metrics.py, bit for bit.

Wrap: launch 2's descriptors stand at offset 576000 of the descriptor ring (a
multiple of both 64 and the 72-byte descriptor) behind a synchronisation of
the stream; launch 3's array needs more room than the ring has left and more
than lies below launch 2's, so a ring that reused offset 0 without waiting
would put launch 3's own, valid descriptors 8000.. over launch 2's: launch 2
would then compute other clients into another output (a failed comparison, no
fault).  A correct ring can only wait for launch 2 here, and the wait ends the
blocker, so "the blocker is still running" is asserted at the last moment at
which it can hold: on entry to the ring's device synchronisation inside launch
3's ``put`` -- or, for a ring that does not wait, right after launch 3 is
queued.

Growth: with a launch queued behind a blocker, one launch whose result
reservation exceeds the result ring and whose descriptors exceed the
descriptor ring."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_detection_metrics import assert_same_bits, case, oracle_all

DEV = torch.device("cuda", 0)
SENTINEL = -7.0
BASE = 16          # distinct tiny clients; a launch's client i is client i % BASE
DESC = 72
RING = 1 << 20


@pytest.fixture(scope="module")
def clients():
    """BASE tiny clients on the device and their oracle rows [8, BASE]."""
    rng = np.random.default_rng(515)
    cases = []
    for i in range(BASE):
        c = np.round(rng.gamma(2.0, 3.0, size=3 + i % 5), 2)
        s = np.r_[rng.choice(c, size=4), np.round(rng.gamma(2.0, 3.0, size=5 + i % 3), 2)]
        y = (np.arange(s.size) % 2).astype(np.int32)
        cases.append(case(c, s, y, i % c.size))
    want = oracle_all(cases)
    want.setflags(write=False)
    assert np.isfinite(want).all() and len({want[:, i].tobytes() for i in range(BASE)}) > BASE // 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    dev = [(t(c["calib"]), t(c["scores"]), t(c["labels"]), c["j"]) for c in cases]
    return dev, want


def descriptors(clients, k, out_ptr, stride, first=0):
    """DetectDesc array of k clients (client i is base client (first + i) % BASE)."""
    from fedmse_decentralized_amd.ops import _hip

    dev, _ = clients
    base = _hip.detect_desc([d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev], [d[3] for d in dev],
                            0, stride if stride >= BASE else BASE)
    desc = base[(first + np.arange(k)) % BASE].copy()
    desc["out"] = out_ptr + 8 * np.arange(k, dtype=np.int64)
    desc["out_stride"] = stride
    assert desc.dtype.itemsize == DESC
    return desc


def expected(clients, k, first=0):
    return clients[1][:, (first + np.arange(k)) % BASE]


def launch(rt, desc, *filler):
    """``put`` (the filler arrays first) and the launch; returns the descriptors' ring offset."""
    from fedmse_decentralized_amd.ops import _hip

    ptrs = rt.desc.put(*filler, desc)
    _hip._check(_hip.lib().fedmx_detect(ptrs[-1], len(desc), rt.stream), "fedmx_detect")
    return ptrs[-1] - rt.desc.buf.dev_ptr


def matmuls(a, count):
    for _ in range(count):
        torch.mm(a, a)


def blocker_count(a, target_ms):
    """Matmuls of ``a`` that keep the current stream busy for about ``target_ms`` (timed with events)."""
    matmuls(a, 2)   # (the first call loads the GEMM kernel)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    matmuls(a, 4)
    t1.record()
    t1.synchronize()
    each = max(t0.elapsed_time(t1) / 4, 1e-3)
    return int(min(max(target_ms / each, 4), 2000))


class DrainProbe:
    """Wraps ``_hiprt.device_sync``: counts the calls and, on entry to each, notes whether ``event`` had completed."""

    def __init__(self, monkeypatch, event):
        from fedmse_decentralized_amd.ops import _hiprt

        self.done_at_entry, self.at = [], []
        real = _hiprt.device_sync

        def device_sync():
            self.done_at_entry.append(event.query())
            self.at.append(time.perf_counter())
            real()

        monkeypatch.setattr(_hiprt, "device_sync", device_sync)


def test_wrap_under_a_busy_stream(clients, monkeypatch):
    from fedmse_decentralized_amd.ops import _hip

    rt = _hip.Runtime(DEV, private=True)
    assert rt.desc.buf.nbytes == RING
    k1, k2, k3, extra = 8, 64, 8100, 3
    assert 576000 % 64 == 0 and 576000 % DESC == 0 and (k2 * DESC) % 64 == 0
    assert 576000 + k2 * DESC + k3 * DESC > RING       # launch 3 does not fit behind launch 2 ...
    assert k3 * DESC > 576000 + k2 * DESC              # ... and from offset 0 it extends past launch 2's descriptors
    with _hip.use_runtime(rt):
        res = [torch.full((8, k + extra), SENTINEL, dtype=torch.float64, device=DEV) for k in (k1, k2, k3)]
        d1 = descriptors(clients, k1, res[0].data_ptr(), k1 + extra)
        d2 = descriptors(clients, k2, res[1].data_ptr(), k2 + extra, first=5)
        d3 = descriptors(clients, k3, res[2].data_ptr(), k3 + extra, first=3)
        a = torch.randn(4096, 4096, device=DEV)
        count = blocker_count(a, 150.0)
        # 1. the ring stands at 576000
        filler = np.zeros(576000 - k1 * DESC, np.uint8)
        assert launch(rt, d1, filler) == 576000 - k1 * DESC and rt.desc.off == 576000
        rt.sync()                                                                     # 2.
        t0, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        matmuls(a, count)                                                             # 3.
        done.record()
        probe = DrainProbe(monkeypatch, done)
        h0 = time.perf_counter()
        assert launch(rt, d2) == 576000                                               # 4.
        off3 = launch(rt, d3)                                                         # 5.
        h1 = time.perf_counter()
        still_running = not done.query()                                              # 6.
        rt.sync()                                                                     # 7.
        torch.cuda.synchronize(DEV)
        blocker_ms = t0.elapsed_time(done)
        host_ms = 1e3 * ((probe.at[0] if probe.at else h1) - h0)
        print(f"wrap: blocker {blocker_ms:.3f} ms ({count} matmuls), host time from launch 2 to the ring's "
              f"decision on launch 3 {host_ms:.3f} ms, drains {len(probe.at)}, launch 3 at offset {off3}")
        assert off3 == 0
        assert blocker_ms >= 20 * host_ms, (blocker_ms, host_ms)
        if probe.at:
            assert probe.done_at_entry == [False], "the blocker had ended before the ring had to decide"
        else:
            assert still_running, "the blocker had ended before launch 3 was queued"
        for r, k, first, name in ((res[0], k1, 0, "launch 1"), (res[1], k2, 5, "launch 2"), (res[2], k3, 3, "launch 3")):
            host = r.cpu().numpy()
            assert np.all(host[:, k:] == SENTINEL), name + ": columns beyond the launch's clients were written"
            assert_same_bits(host[:, :k], expected(clients, k, first), name)


def test_growth_with_a_launch_queued(clients, monkeypatch):
    from fedmse_decentralized_amd.ops import _hip

    rt = _hip.Runtime(DEV, private=True)
    assert rt.desc.buf.nbytes == RING and rt.out.buf.nbytes == RING
    k1, k2 = 40, 16400
    assert 8 * 8 * k2 > RING and DESC * k2 > RING
    with _hip.use_runtime(rt):
        a = torch.randn(4096, 4096, device=DEV)
        count = blocker_count(a, 40.0)
        old_desc, old_out = rt.desc.buf, rt.out.buf
        t0, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        matmuls(a, count)
        done.record()
        probe = DrainProbe(monkeypatch, done)
        h0 = time.perf_counter()
        p1, v1 = rt.out.take(np.float64, 8 * (k1 + 2))
        v1[:] = SENTINEL
        launch(rt, descriptors(clients, k1, p1, k1 + 2, first=7))
        d2 = descriptors(clients, k2, 0, k2 + 2, first=1)
        p2, v2 = rt.out.take(np.float64, 8 * (k2 + 2))      # larger than the result ring: drains, then grows
        v2[:] = SENTINEL
        d2["out"] += p2
        launch(rt, d2)                                      # larger than the descriptor ring
        rt.sync()
        torch.cuda.synchronize(DEV)
        blocker_ms = t0.elapsed_time(done)
        host_ms = 1e3 * (probe.at[0] - h0)
        print(f"growth: blocker {blocker_ms:.3f} ms ({count} matmuls), host time to the first growth {host_ms:.3f} ms")
        assert probe.done_at_entry == [False, True], probe.done_at_entry   # launch 1 was queued behind the blocker
        assert rt.out._retired == [old_out] and rt.desc._retired == [old_desc]
        assert rt.out.buf.nbytes >= 8 * 8 * (k2 + 2) and rt.desc.buf.nbytes >= DESC * k2
        assert p2 == rt.out.buf.dev_ptr and p1 == old_out.dev_ptr
        assert np.shares_memory(v1, old_out.np) and np.shares_memory(v2, rt.out.buf.np)
        for v, k, first, name in ((v1, k1, 7, "the launch before the growth"), (v2, k2, 1, "the launch that grew both")):
            host = np.array(v).reshape(8, k + 2)
            assert np.all(host[:, k:] == SENTINEL), name + ": columns beyond the launch's clients were written"
            assert_same_bits(host[:, :k], expected(clients, k, first), name)
