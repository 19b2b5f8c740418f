"""The launch rings of ops/_hiprt.py (``_Ring``, ``DescRing``, ``OutRing``) on
a model of the device: a fake buffer, a recorded ``device_sync`` and a set of
live regions -- those handed out since the last synchronisation that covers
the ring's stream, which a queued kernel may still read or write.  No
allocation may overlap a live region, whatever the order of allocations,
wraps, growths and synchronisations; and the steady round pattern must never
pay for a device synchronisation."""
import numpy as np
import pytest

from fedmse_decentralized_amd.ops import _hiprt

MIB = 1 << 20
KIB = 1 << 10
STREAM, OTHER = 0x5EED0, 0x5EED1   # made-up stream handles


class FakeBuffer:
    made = 0

    def __init__(self, nbytes):
        FakeBuffer.made += 1
        self.nbytes = nbytes
        self.np = np.zeros(nbytes, dtype=np.uint8)
        self.dev_ptr = FakeBuffer.made << 40
        EVENTS.append(("buffer", nbytes))

    view = _hiprt.MappedBuffer.view


class FakeRing(_hiprt._Ring):
    buffer_type = FakeBuffer


class FakeDescRing(_hiprt.DescRing):
    buffer_type = FakeBuffer


class FakeOutRing(_hiprt.OutRing):
    buffer_type = FakeBuffer


EVENTS = []   # ("sync",) and ("buffer", nbytes) in the order they happened
MODELS = []   # every Model of the running test: a device synchronisation covers them all


@pytest.fixture(autouse=True)
def fake_device(monkeypatch):
    """``device_sync`` recorded instead of run; the process-wide clock restored."""
    clock = _hiprt.SyncClock
    monkeypatch.setattr(clock, "gen", clock.gen)
    monkeypatch.setattr(clock, "_stream_gen", dict(clock._stream_gen))

    def device_sync():
        EVENTS.append(("sync",))
        clock.tick()
        for m in MODELS:
            m.live = []

    monkeypatch.setattr(_hiprt, "device_sync", device_sync)
    del EVENTS[:], MODELS[:]
    yield
    del EVENTS[:], MODELS[:]


def syncs():
    return EVENTS.count(("sync",))


class Model:
    """A ring with the regions that may still be in use on the device."""

    def __init__(self, nbytes, ring=None):
        self.ring = ring if ring is not None else FakeRing(nbytes, STREAM)
        self.live = []    # (buffer, start, end)
        self.wraps = 0
        MODELS.append(self)

    def tick(self, stream=None):
        _hiprt.SyncClock.tick(stream)
        for m in MODELS:
            if stream is None or stream == m.ring.stream:
                m.live = []

    def alloc(self, nbytes, via=None):
        """One ``_alloc`` of ``nbytes`` (made by ``via()``, which returns the
        offset, when given) with every invariant checked; returns (offset, drained)."""
        before, size, prev_off = syncs(), self.ring.buf.nbytes, self.ring.off
        old = self.ring.buf
        first = len(EVENTS)
        o = self.ring._alloc(nbytes) if via is None else via()
        drained = syncs() > before   # (which emptied self.live)
        buf = self.ring.buf
        end = o + ((nbytes + 63) & ~63)
        assert o % 64 == 0 and 0 <= o and end <= buf.nbytes, (o, nbytes, buf.nbytes)
        assert self.ring.off == end
        if nbytes > size:
            # growth: drained before the new buffer exists, old buffer kept, offset 0
            assert EVENTS[first] == ("sync",) and EVENTS[first + 1][0] == "buffer"
            assert buf is not old and any(b is old for b in self.ring._retired)
            assert o == 0 and buf.nbytes >= nbytes
        else:
            assert buf is old
        if o < prev_off and buf is old:
            self.wraps += 1
        for b, s, e in self.live:
            assert b is not buf or end <= s or e <= o, \
                f"[{o}, {end}) overlaps the region [{s}, {e}) a queued kernel may still use"
        self.live.append((buf, o, end))
        return o, drained


# ---------------------------------------------------------------------------
def test_wrap_after_a_mid_pass_synchronisation_drains():
    """3 MiB, synchronise, 900 KiB for a kernel that stays queued, 3.5 MiB:
    the last wraps over the 900 KiB region, so it must drain first."""
    m = Model(4 * MIB)
    assert m.alloc(3 * MIB) == (0, False)
    m.tick(STREAM)
    assert m.alloc(900 * KIB) == (3 * MIB, False)
    o, drained = m.alloc(3 * MIB + 512 * KIB)
    assert o == 0 and drained and syncs() == 1


def test_wrap_below_the_live_regions_needs_no_drain():
    m = Model(4 * MIB)
    m.alloc(3 * MIB)
    m.tick(STREAM)
    m.alloc(900 * KIB)
    assert m.alloc(3 * MIB) == (0, False)          # ends exactly where the live region starts
    assert syncs() == 0
    # the live span now runs [3 MiB, end) + [0, 3 MiB): nothing more fits without a drain
    assert m.alloc(64) == (3 * MIB, True)


def test_a_synchronisation_of_another_stream_does_not_release_the_ring():
    m = Model(4 * MIB)
    m.alloc(3 * MIB)
    m.tick(OTHER)
    m.alloc(900 * KIB)
    for _ in range(3):
        m.tick(OTHER)
    o, drained = m.alloc(3 * MIB + 512 * KIB)
    assert o == 0 and drained
    # ... nor on a plain wrap with nothing but other streams' synchronisations
    m = Model(4 * MIB)
    m.alloc(3 * MIB)
    m.tick(OTHER)
    o, drained = m.alloc(2 * MIB)
    assert o == 0 and drained


def test_device_synchronisation_releases_the_ring():
    m = Model(4 * MIB)
    m.alloc(3 * MIB)
    m.alloc(512 * KIB)
    m.tick()
    assert m.alloc(3 * MIB) == (0, False) and syncs() == 0


def test_request_larger_than_the_ring_grows_it():
    m = Model(4 * MIB)
    m.alloc(MIB)
    old = m.ring.buf
    o, drained = m.alloc(6 * MIB)     # the model checks order, _retired, offset and size
    assert o == 0 and drained and m.ring._retired == [old]
    assert EVENTS[-2:] == [("sync",), ("buffer", m.ring.buf.nbytes)]
    assert m.ring.buf.nbytes >= 6 * MIB
    # right after a stream synchronisation too: other streams may still read the old ring
    m = Model(4 * MIB)
    m.alloc(MIB)
    m.tick(STREAM)
    assert m.alloc(4 * MIB + 1) == (0, True)
    # the request that just fits does not grow
    m = Model(4 * MIB)
    assert m.alloc(4 * MIB) == (0, False) and m.ring._retired == []


@pytest.mark.parametrize("seed", range(8))
def test_random_walk_never_hands_out_a_live_region(seed):
    """A few thousand steps: allocations of 1 byte to 1.5 rings (mostly small,
    so that passes hold many regions), synchronisations of the ring's stream,
    of another stream and of the device."""
    rng = np.random.default_rng(1000 + seed)
    size = 64 * KIB
    m = Model(size)
    grown = 0
    for _ in range(4000):
        r = rng.random()
        if r < 0.08:
            m.tick(STREAM)
        elif r < 0.14:
            m.tick(OTHER)
        elif r < 0.16:
            m.tick()
        else:
            cur = m.ring.buf.nbytes
            kind = rng.random()
            if kind < 0.6:
                n = int(rng.integers(1, cur // 16))
            elif kind < 0.97:
                n = int(rng.integers(1, cur + 1))
            else:
                n = int(rng.integers(cur + 1, cur + cur // 2 + 1))
            grown += n > cur
            m.alloc(n)
        if m.ring.buf.nbytes > 64 * size:   # keep growing rings small: start over
            m = Model(size)
    assert m.wraps + grown > 0


def test_random_walk_covers_wraps_drains_and_growth():
    """The walk above is worth something only if it wraps with and without a
    drain and grows: counted here on one seed."""
    rng = np.random.default_rng(1000)
    m = Model(64 * KIB)
    wraps = drains = free_wraps = 0
    for _ in range(4000):
        r = rng.random()
        if r < 0.08:
            m.tick(STREAM)
        elif r < 0.14:
            m.tick(OTHER)
        else:
            before = m.wraps
            _, drained = m.alloc(int(rng.integers(1, m.ring.buf.nbytes // 8)))
            wraps += m.wraps - before
            drains += drained
            free_wraps += (m.wraps - before) and not drained
    assert wraps > 50 and drains > 5 and free_wraps > 5


def test_steady_rounds_never_drain():
    """A few allocations, a stream synchronisation, repeat -- across many
    wraps of the 4 MiB ring, at round sizes that do not divide it: the ring
    never asks for a device synchronisation."""
    rng = np.random.default_rng(7)
    m = Model(4 * MIB)
    for _ in range(600):
        for _ in range(int(rng.integers(2, 7))):
            m.alloc(int(rng.integers(1, 200 * KIB)))
        m.tick(STREAM)
    assert m.wraps > 40
    assert syncs() == 0


# ---------------------------------------------------------------------------
def test_put_lays_arrays_out_contiguously_and_intact():
    ring = FakeDescRing(MIB, STREAM, device_memory=False)
    ring._alloc(100)   # start away from 0
    rng = np.random.default_rng(3)
    a = rng.integers(0, 255, size=72 * 5, dtype=np.uint8).view(np.dtype([("x", "u8", (9,))]))   # 360 bytes
    b = rng.normal(size=(3, 7))                                                                  # 168 bytes
    c = rng.normal(size=(8, 8)).astype(np.float32)[:, ::2]                                       # not contiguous
    d = np.arange(16, dtype=np.int32)                                                            # 64 bytes exactly
    ptrs = ring.put(a, b, c, d)
    base = ring.buf.dev_ptr
    offs = [p - base for p in ptrs]
    assert offs == [128, 128 + 384, 128 + 384 + 192, 128 + 384 + 192 + 128]
    assert ring.off == offs[-1] + 64
    for o, arr in zip(offs, (a, b, c, d)):
        want = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert o % 64 == 0 and np.array_equal(ring.buf.np[o:o + want.size], want)
    # one put never straddles the end of the ring
    ring._alloc(MIB - ring.off - 256)
    (p,) = ring.put(np.ones(100, dtype=np.float64))
    assert p == base


def test_put_and_take_under_the_model():
    """The two public entry points obey the same invariants as ``_alloc``."""
    desc = Model(0, FakeDescRing(64 * KIB, STREAM, device_memory=False))
    out = Model(0, FakeOutRing(64 * KIB, STREAM))
    rng = np.random.default_rng(11)
    for _ in range(1500):
        if rng.random() < 0.1:
            desc.tick(STREAM)
        arrs = [rng.integers(0, 255, size=int(rng.integers(1, 3000)), dtype=np.uint8)
                for _ in range(rng.integers(1, 4))]
        got = {}

        def put():
            got["ptrs"] = desc.ring.put(*arrs)
            return got["ptrs"][0] - desc.ring.buf.dev_ptr

        desc.alloc(sum((a.size + 63) & ~63 for a in arrs), via=put)
        for p, a in zip(got["ptrs"], arrs):
            o = p - desc.ring.buf.dev_ptr
            assert np.array_equal(desc.ring.buf.np[o:o + a.size], a)
        n = int(rng.integers(0, 700))

        def take():
            got["ptr"], got["view"] = out.ring.take(np.float64, n)
            return got["ptr"] - out.ring.buf.dev_ptr

        o, _ = out.alloc(max(8 * n, 1), via=take)
        view = got["view"]
        assert view.shape == (n,) and view.dtype == np.float64
        assert n == 0 or np.shares_memory(view, out.ring.buf.np[o:o + 8 * n])
    assert desc.wraps > 5 and out.wraps > 5


def test_view_taken_before_a_growth_reads_the_old_buffer():
    ring = FakeOutRing(64 * KIB, STREAM)
    ptr, view = ring.take(np.float64, 100)
    old = ring.buf
    view[:] = np.arange(100)
    big_ptr, big = ring.take(np.float64, 64 * KIB // 8 + 1)
    assert ring.buf is not old and ring._retired == [old] and syncs() == 1
    assert big_ptr == ring.buf.dev_ptr and big.size == 64 * KIB // 8 + 1
    big[:] = -1.0
    ring.take(np.float64, 100)[1][:] = -2.0
    assert np.array_equal(view, np.arange(100, dtype=np.float64))
    assert np.shares_memory(view, old.np) and not np.shares_memory(view, ring.buf.np)
    assert ptr == old.dev_ptr
