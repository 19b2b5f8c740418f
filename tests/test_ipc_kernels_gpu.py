"""The three kernels of ``fedmx_ipc.hip`` (``ipc_push_kernel``,
``ipc_wait_gather_kernel``, ``ipc_wait_reduce_f64_kernel``) launched directly
from hand-built ``IpcArgs`` blocks in ONE process.  The kernels see addresses
only, so a "rank" is an argument block: W ranks are W receive areas (ordinary
zero-filled int32 device tensors, no ``fedmx_ipc_alloc``, no IPC handles:
uncached memory and cross-process mappings stay with ``test_ipc_gpu.py``), W
sources, W outputs and one shared status word.

Every call is checked three ways, all bit for bit:

* the outputs against a host oracle (the stack of contributions; for the
  reduce the float64 loop ``acc = 0.0; for s in range(W): acc += x[s]``) and
  a sentinel tail behind them;
* EVERY word of every receive area against a host model of the protocol: flag
  (parity, s, c) = seq for s != rank and c < chunks, slot (parity, s) holds
  rank s's words, and everything else -- the other parity's data and flags,
  the flags at c >= chunks, the rank's own row and own slot, the slots' tails
  of earlier longer calls -- is what it was;
* the status word (0, except in the bounded-wait test).

NaN results of the reduce: IEEE 754 leaves the sign and payload of a NaN that
an operation makes or passes on to the implementation, so the oracle's NaN
bits are a property of the host that runs it.  An entry whose oracle value
is NaN must be NaN; every other entry must have the oracle's bits; and the W
ranks' outputs must agree in every bit, NaNs included.

The order-dependence of the reduce inputs is itself asserted on the host (for
W >= 3; float addition is commutative, so with one or two ranks every order
gives the same bits): another summation order changes the bits of every
designated entry, and the reverse order changes the vector.

Measured on an MI355X (gfx950), all 16 tests passing in 3.3 s together:

* Gather: 23 / 24 / 24 / 23 / 23 cases at worlds 1 / 2 / 3 / 8 / 16 (the
  65,536-word case at worlds 2 and 3 only; 9,216 x r for r = 1 .. 7 at caps
  64 and 56 at every world, 132 MB of areas for r = 7 at world 16);
  0.03 .. 0.29 s per world, 0.58 s at world 16.  Three sequences of 8 calls
  on one set of areas, 0.03 s each at most.
* Reduce: 10 calls per world (5 lengths, out of place and in place) on one
  set of areas, 0.02 s per world at most.  (With an x86 host the GPU's NaN
  results had the oracle's sign and payload too.)
* Refusals: 51 refused launches and 2 accepted collectives, under 5 ms.
  Bounded wait: 4 waits, 3 of them running into their 5 ms bound, 0.02 s.
* Bugs found in the kernels: none.  Each of these changes to
  ``fedmx_ipc.hip``, tried on a scratch copy, fails tests of this file: the
  other parity in ``ipc_data`` (13 of 16 tests fail), ``* A.n_words`` for
  ``* A.slot_words`` there (13), the reduce summing ranks W-1 .. 0 (3: worlds
  3, 8, 16), the own block read from the area in the gather (10) and in the
  reduce (7), the flag published only when ``lo < hi`` (7).
* Not tested, on purpose: a flag across the wrap of the sequence number.
  ``(int)(flag - seq) < 0`` is a signed subtraction, so its wrap is not defined,
  and ``ipc_check`` refuses ``seq <= 0``: a channel ends before call 2^31.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.ops import _hip, _hiprt  # noqa: E402
from fedmse_decentralized_amd.parallel.ipc import chunk_plan  # noqa: E402

DEV = torch.device("cuda", 0)
MAXC = _hip.IPC_MAX_CHUNKS
SENTINEL = 0x5A5A5A5A      # every output word before a call, and the tail behind the output for ever
TAIL = 64                  # sentinel words behind every output
# float32 bit patterns a copy must not touch: quiet / signalling NaNs with payloads, +-inf, -0.0, subnormals
SPECIAL_BITS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFBFFFFF, 0x7F800000, 0xFF800000, 0x80000000,
                         0x00000001, 0x807FFFFF, 0x00400000], dtype=np.uint32).view(np.int32)


def _sync():
    _hip.runtime(DEV).sync()
    torch.cuda.synchronize()


def _bits(world, n_words, seed):
    """[world, n_words] int32: random bit patterns, the special float32 patterns
    at random places (rotated by rank, so that short calls see all of them)."""
    g = np.random.default_rng(seed)
    x = g.integers(-2**31, 2**31, size=(world, n_words), dtype=np.int64).astype(np.int32)
    for r in range(world):
        k = min(n_words, SPECIAL_BITS.size)
        x[r, g.choice(n_words, k, replace=False)] = np.roll(SPECIAL_BITS, r)[:k]
    return x


def _with(a, **over):
    """The block with some fields replaced (``area1=0``: entry 1 of area[])."""
    for k, v in over.items():
        if k.startswith("area"):
            a.area[int(k[4:])] = v
        else:
            setattr(a, k, v)
    return a


_STATUS = []     # the one host-visible status word (64 mapped bytes) every block of this file points to


class _World:
    """W ranks in one process: their receive areas, the host model of every
    area word, one status word."""

    def __init__(self, world, slot_words, timeout_ms=50):
        rt = _hip.runtime(DEV)
        self.L, self.stream = _hip.lib(), rt.stream
        self.W, self.slot = world, slot_words
        self.flag0 = 2 * world * slot_words                 # first flag word of an area
        self.words = self.flag0 + 2 * world * MAXC
        self.areas = [torch.zeros(self.words, dtype=torch.int32, device=DEV) for _ in range(world)]
        self.model = np.zeros((world, self.words), dtype=np.int32)
        if not _STATUS:
            _STATUS.append(_hiprt.MappedBuffer(64))
        self.status = _STATUS[0]
        self.view = self.status.view(0, np.int32, 1)
        self.view[0] = 0
        khz = self.L.fedmx_ipc_wall_khz()
        self.ticks_per_ms = khz if khz > 0 else 100_000
        # no wait of this file spins (see exchange), so the bound is only how long a broken kernel can sit
        self.timeout_ticks = int(timeout_ms * self.ticks_per_ms)

    def data_at(self, parity, src):
        return (parity * self.W + src) * self.slot

    def flag_at(self, parity, src):
        return self.flag0 + (parity * self.W + src) * MAXC

    def args(self, rank, src, out, n_words, chunks, chunk_words, seq):
        a = _hip.IpcArgs()
        for r in range(self.W):
            a.area[r] = self.areas[r].data_ptr()
        # (area[world:] stay null: only the first `world` entries are the launchers' business)
        a.src, a.out, a.status = src, out, self.status.dev_ptr
        a.timeout_ticks = self.timeout_ticks
        a.world, a.rank, a.n_words, a.slot_words = self.W, rank, n_words, self.slot
        a.parity, a.seq, a.chunks, a.chunk_words = seq & 1, seq, chunks, chunk_words
        return a

    def buffers(self, x, out_words, inplace=False):
        """Device sources of the rows of x (int32 [W, n]) and sentinel outputs of
        out_words + TAIL words; in place the output IS the source, tail and all."""
        srcs, outs = [], []
        for r in range(self.W):
            s = torch.full((x.shape[1] + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
            s[:x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x[r])).to(DEV)
            srcs.append(s)
            outs.append(s if inplace else torch.full((out_words + TAIL,), SENTINEL, dtype=torch.int32, device=DEV))
        return srcs, outs

    def exchange(self, kind, x, chunks, chunk_words, seq, inplace=False):
        """One collective of all W ranks on the runtime's stream; returns the
        ranks' outputs, int32 [W, out_words], after checking their tails, every
        area word and the status word.

        ORDERING RULE: the pushes of ALL W ranks are enqueued first, then the
        waits of all W ranks, on one stream.  Every flag is therefore set
        before any wait kernel starts and nothing ever spins.  (A wait enqueued
        before its peers' pushes on the same stream would sit until its timeout:
        only the bounded-wait test does that, once, on purpose.)"""
        W, n = x.shape
        wait = self.L.fedmx_ipc_wait_gather if kind == "gather" else self.L.fedmx_ipc_wait_reduce_f64
        out_words = W * n if kind == "gather" else n
        srcs, outs = self.buffers(x, out_words, inplace)
        blocks = [self.args(r, srcs[r].data_ptr(), outs[r].data_ptr(), n, chunks, chunk_words, seq) for r in range(W)]
        self.view[0] = 0
        torch.cuda.synchronize()
        for a in blocks:
            assert self.L.fedmx_ipc_push(ctypes.byref(a), self.stream) == 0
        for a in blocks:
            assert wait(ctypes.byref(a), self.stream) == 0
        _sync()
        p = seq & 1
        for r in range(W):
            for s in range(W):
                if s != r:
                    self.model[r, self.data_at(p, s):self.data_at(p, s) + n] = x[s]
                    self.model[r, self.flag_at(p, s):self.flag_at(p, s) + chunks] = seq
        got = torch.stack(outs).cpu().numpy()
        assert (got[:, out_words:] == SENTINEL).all(), "a wait wrote behind its output"
        if not inplace:
            for r in range(W):
                assert np.array_equal(srcs[r].cpu().numpy()[:n], x[r]), "a source was written"
        self.check_areas()
        assert int(self.view[0]) == 0, "a wait timed out"
        return got[:, :out_words]

    def where(self, off):
        if off >= self.flag0:
            q, c = divmod(off - self.flag0, MAXC)
            return "flag (parity %d, src %d, chunk %d)" % (*divmod(q, self.W), c)
        q, i = divmod(off, self.slot)
        return "data (parity %d, src %d, word %d)" % (*divmod(q, self.W), i)

    def check_areas(self):
        got = torch.stack(self.areas).cpu().numpy()
        if not np.array_equal(got, self.model):
            r, off = (int(v[0]) for v in np.nonzero(got != self.model))
            raise AssertionError(f"area of rank {r}: {self.where(off)} is {got[r, off]:#x}, "
                                 f"the protocol says {self.model[r, off]:#x} "
                                 f"({int((got != self.model).sum())} words differ)")


# ---------------------------------------------------------------------------
# gather

WORLDS = [1, 2, 3, 8, 16]
P = 9216     # words of one model row: the round gathers whole rows


def _gather_cases(world):
    """(n_words, chunks, chunk_words, slot_words) at this world."""
    cases = [(4, 1, 4, 1024),            # one f32x4
             (256, 64, 4, 1024),         # 64 chunks of one f32x4: one live thread each
             (1024, 1, 1024, 1024),      # one load per thread; n_words == slot_words
             (1028, 1, 1028, 2048),      # thread 0 takes a second trip
             (4100, 5, 1024, 4112),      # last chunk of 4 words
             (8, 64, 4, 1024),           # 62 chunks wholly past n_words: nothing to move, flags still due
             (4096, 4, 1024, 4096),      # n_words == slot_words, several chunks
             (12, 1, 12, 4096),          # far below the slot: the source stride is the slot
             (12, 3, 4, 4096)]
    if world in (2, 3):
        cases.append((65536, 64, 1024, 65536))
    for cap in (64, 56):                 # one rank per GPU; 9 ranks on 8 GPUs
        for r in range(1, 8):
            # (a 7-row slot at the small worlds; at 8 and 16 the slot is the payload, which keeps
            # the sixteen 32-slot areas of world 16 at 132 MB for the longest call)
            cases.append((r * P, *chunk_plan(r * P, cap), 7 * P if world <= 3 else r * P))
    return cases


@pytest.mark.parametrize("world", WORLDS)
def test_gather_is_a_bitwise_copy_at_every_chunk_edge(world):
    """Every rank's gathered [world][n_words] is the stack of the ranks'
    contributions bit for bit (world 1: a copy of src, nothing pushed or
    waited for); fresh areas per case, the sequence number (hence the parity)
    changing from case to case."""
    cases = _gather_cases(world)
    assert len(cases) >= 23
    for k, (n, chunks, cw, slot) in enumerate(cases):
        w = _World(world, slot)
        x = _bits(world, n, 100 * world + k)
        got = w.exchange("gather", x, chunks, cw, seq=k + 1)
        for r in range(world):
            assert np.array_equal(got[r].reshape(world, n), x), (world, n, chunks, cw, r)


@pytest.mark.parametrize("world", [2, 3, 16])
def test_gather_call_sequence_on_one_set_of_areas(world):
    """Calls 1 .. 8 on the same areas, lengths long, short, long, 4 words,
    full slot, short, 4 words, long, fresh data each call: every call exact (no
    stale tail of a longer call, never the other parity's data), and after every
    call the whole of every area is what the protocol says -- the other parity's
    flags and data as the call before left them, own slot and own row zero."""
    slot = 8192
    w = _World(world, slot)
    plan = [(6144, 6, 1024), (260, 1, 260), (5000, 5, 1000), (4, 1, 4), (8192, 8, 1024), (516, 2, 260),
            (4, 64, 4), (7168, 64, 112)]
    for seq, (n, chunks, cw) in enumerate(plan, start=1):
        x = _bits(world, n, 1000 * world + seq)
        got = w.exchange("gather", x, chunks, cw, seq)
        for r in range(world):
            assert np.array_equal(got[r].reshape(world, n), x), (world, seq, r)
    for r in range(world):     # a rank's own slot and own flag row, both parities, were never written
        for p in (0, 1):
            assert not w.model[r, w.data_at(p, r):w.data_at(p, r) + slot].any()
            assert not w.model[r, w.flag_at(p, r):w.flag_at(p, r) + MAXC].any()


# ---------------------------------------------------------------------------
# reduce

def _rank_order_sum(x):
    """acc = 0.0; for s in range(W): acc += x[s] -- per entry, in float64."""
    acc = np.zeros(x.shape[1], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(x.shape[0]):
            acc = acc + x[s]
    return acc


def _reduce_values(world, m, seed):
    """float64 [world, m] in which every rank contributes to every entry, and
    the indices of the entries built to depend on the summation order."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((world, m)) * 10.0 ** g.uniform(-8, 8, size=(world, m))   # mixed magnitudes
    order_cols = []
    lo, mid, hi = 0, world // 2, world - 1
    triples = [dict(zip(pl, (1.0, 1e16, -1e16))) for pl in itertools.permutations((lo, mid, hi))] if world >= 3 else []
    tiny = 2.0 ** -40 * (1 + np.arange(world))

    def triple(col, t):
        x[:, col] = tiny
        for rank, v in t.items():
            x[rank, col] = v
        order_cols.append(col)

    if m >= 16:
        x[:, 0] = -0.0                         # -0.0 from every rank: 0.0 + -0.0 + ... = +0.0
        x[lo, 1] = np.nan                      # one NaN contributor, first / last rank
        x[hi, 2] = np.nan
        x[hi, 3] = np.inf
        x[lo, 4] = -np.inf
        x[lo, 5], x[hi, 5] = np.inf, (-np.inf if world > 1 else 1.0)   # inf - inf
        for j, t in enumerate(triples):
            triple(6 + j, t)
    elif triples:
        triple(m - 1, triples[0])
    return x, order_cols


def _assert_order_matters(x, order_cols):
    """The inputs can tell a wrong order from the right one: for every
    designated entry some other order of the ranks gives other bits, and the
    reverse order changes the vector."""
    W = x.shape[0]
    if W < 3:
        return 0     # a + b == b + a: nothing to tell apart
    g = np.random.default_rng(7)
    orders = (list(itertools.permutations(range(W))) if W == 3 else
              [list(range(W))[::-1]] + [list(np.roll(np.arange(W), k)) for k in (1, 2, 3)]
              + [list(g.permutation(W)) for _ in range(8)])
    fwd = _rank_order_sum(x).view(np.int64)
    other = np.stack([_rank_order_sum(x[list(o)]).view(np.int64) for o in orders])
    differs = (other != fwd).any(axis=0)
    assert order_cols and differs[order_cols].all(), (W, order_cols, differs[order_cols])
    rev = _rank_order_sum(x[::-1])
    finite = np.isfinite(rev)
    assert (rev.view(np.int64)[finite] != fwd[finite]).any(), W
    return int(differs.sum())


def _check_reduce(got, x, ctx):
    """got: int32 [W, 2 m] outputs of the W ranks against the rank-order oracle."""
    exp = _rank_order_sum(x)
    out = np.ascontiguousarray(got).view(np.float64)
    nan = np.isnan(exp)
    for r in range(x.shape[0]):
        assert np.isnan(out[r][nan]).all(), (ctx, r)
        assert np.array_equal(out[r][~nan].view(np.int64), exp[~nan].view(np.int64)), (ctx, r)
        assert np.array_equal(got[r], got[0]), (ctx, r)     # every rank: the same bits, NaNs too


@pytest.mark.parametrize("world", WORLDS)
def test_reduce_sums_in_rank_order_on_every_rank(world):
    """Ten calls on one set of areas (seq 1 .. 10: five lengths, each out of
    place and in place as ``reduce_f64`` does), every rank contributing to
    every entry with values whose sum depends on the order: each rank's
    output has the bits of the float64 loop over ranks 0 .. W-1 -- the own
    block, read from src, at position ``rank`` like any peer's."""
    slot = 1024
    w = _World(world, slot)
    seq = 0
    for m in (2, 256, 258, 512, 2 * 10 * world):      # doubles; 512 fills the slot
        for inplace in (False, True):
            seq += 1
            x, order_cols = _reduce_values(world, m, 50 * world + seq)
            _assert_order_matters(x, order_cols)
            xi = np.ascontiguousarray(x).view(np.int32)
            got = w.exchange("reduce", xi, 1, 2 * m, seq, inplace=inplace)
            _check_reduce(got, x, (world, m, inplace))
            if m >= 16:
                z = np.ascontiguousarray(got).view(np.float64)[:, 0]
                assert (z == 0.0).all() and not np.signbit(z).any()      # -0.0 from everyone: +0.0


def test_reduce_of_nothing_launches_nothing():
    """n_words == 0: the launcher returns 0 and nothing is written."""
    w = _World(2, 16)
    srcs, outs = w.buffers(np.zeros((2, 0), dtype=np.int32), 8)
    for r in range(2):
        a = w.args(r, srcs[r].data_ptr(), outs[r].data_ptr(), 0, 1, 0, 1)
        assert w.L.fedmx_ipc_wait_reduce_f64(ctypes.byref(a), w.stream) == 0
    _sync()
    assert (torch.stack(outs).cpu().numpy() == SENTINEL).all()
    w.check_areas()
    assert int(w.view[0]) == 0


# ---------------------------------------------------------------------------
# refusals

REFUSALS = [("world 0", dict(world=0)), ("world 17", dict(world=17)),
            ("rank -1", dict(rank=-1)), ("rank == world", dict(rank=2)),
            ("n_words < 0", dict(n_words=-4)), ("n_words > slot_words", dict(n_words=20, chunk_words=20)),
            ("n_words % 4", dict(n_words=6)), ("slot_words % 4", dict(slot_words=18)),
            ("chunks 0", dict(chunks=0)), ("chunks 65", dict(chunks=65)),
            ("chunk_words % 4", dict(chunk_words=10)), ("chunks * chunk_words < n_words", dict(chunk_words=4)),
            ("parity != seq & 1", dict(parity=0)), ("seq 0", dict(seq=0, parity=0)),
            ("null area of rank 0", dict(area0=0)), ("null area of rank 1", dict(area1=0))]


def test_refusals_return_minus_one_and_start_nothing():
    """ipc_check and the launchers' own conditions: every block that differs
    from an accepted one in ONE respect is refused with -1 by every launcher,
    and nothing ran -- outputs and areas at their start values, status 0.  The
    accepted block itself (area[2:] null, as for every world below 16) then
    runs and is exact, so each refusal is due to its one change."""
    w = _World(2, 16)
    x = _bits(2, 8, 3)
    srcs, outs = w.buffers(x, 16)
    L = w.L
    launchers = (L.fedmx_ipc_push, L.fedmx_ipc_wait_gather, L.fedmx_ipc_wait_reduce_f64)

    def block(**over):      # n_words 8 as one chunk of 8: what all three launchers accept
        return _with(w.args(0, srcs[0].data_ptr(), outs[0].data_ptr(), 8, 1, 8, 1), **over)

    for what, over in REFUSALS:
        for fn in launchers:
            assert fn(ctypes.byref(block(**over)), w.stream) == -1, what
    for fn in launchers[1:]:
        assert fn(ctypes.byref(block(out=None)), w.stream) == -1, "null out"
    # several chunks: the gather's business, refused by the reduce
    two = block(chunks=2, chunk_words=4)
    assert L.fedmx_ipc_wait_reduce_f64(ctypes.byref(two), w.stream) == -1
    _sync()
    assert (torch.stack(outs).cpu().numpy() == SENTINEL).all()
    w.check_areas()
    assert int(w.view[0]) == 0
    a = block()
    assert all(a.area[r] == 0 for r in range(2, _hip.IPC_MAX_WORLD))
    got = w.exchange("gather", x, 2, 4, seq=1)
    assert all(np.array_equal(got[r].reshape(2, 8), x) for r in range(2))
    xr, _ = _reduce_values(2, 4, 9)
    _check_reduce(w.exchange("reduce", np.ascontiguousarray(xr).view(np.int32), 1, 8, seq=2), xr, "accepted")


# ---------------------------------------------------------------------------
# the bounded wait

def test_a_missing_peer_times_out_and_a_later_flag_counts():
    """The documented drain path, once: rank 0 of 2 waits (2 chunks) for a
    peer that never pushed.  The launch returns after its ~5 ms bound with
    the status word at 1, rank 0's own row right and the peer's row the area's
    zeros; with a null status pointer it returns just the same and writes no
    status; flags of a LATER call of the parity, seq + 2, count as arrived
    (the test is ``(int)(flag - seq) < 0``) and the wait passes: status 0,
    which a wait that ran into its bound cannot leave.  One more 5 ms
    timeout than the gather's two: ``ipc_wait_reduce_f64_kernel`` has a wait
    loop of its own, not ``ipc_wait_flag``, and nothing else reaches its
    drain path."""
    w = _World(2, 16, timeout_ms=5)
    n, chunks, cw = 8, 2, 4
    x = _bits(2, n, 11)

    def wait(seq, fn=w.L.fedmx_ipc_wait_gather, out_words=2 * n, **over):
        srcs, outs = w.buffers(x, out_words)
        a = _with(w.args(0, srcs[0].data_ptr(), outs[0].data_ptr(), n, chunks, cw, seq), **over)
        w.view[0] = 0
        torch.cuda.synchronize()
        assert fn(ctypes.byref(a), w.stream) == 0
        _sync()                                   # the launch drains
        got = outs[0].cpu().numpy()
        assert (got[out_words:] == SENTINEL).all()
        w.check_areas()                           # a wait writes no area word
        return got[:out_words]

    zeros = np.zeros(n, dtype=np.int32)
    got = wait(seq=1)                                         # no push from rank 1
    assert int(w.view[0]) == 1
    assert np.array_equal(got[:n], x[0]) and np.array_equal(got[n:], zeros)
    got = wait(seq=1, status=None)                            # nowhere to report: still returns
    assert int(w.view[0]) == 0
    assert np.array_equal(got[:n], x[0]) and np.array_equal(got[n:], zeros)
    # the reduce's own wait loop: 0.0 + x0 + (the area's zeros)
    xr = np.array([[1.5, -2.25, 3e10, 7.0], [9.0, 9.0, 9.0, 9.0]])
    x = np.ascontiguousarray(xr).view(np.int32)
    chunks, cw = 1, 8
    got = wait(seq=1, fn=w.L.fedmx_ipc_wait_reduce_f64, out_words=n)
    assert int(w.view[0]) == 1
    assert np.array_equal(got.view(np.float64), xr[0])
    # flags and data as the host puts them: the peer's chunks 0 and 1 of parity 1
    x = _bits(2, n, 12)
    chunks, cw = 2, 4
    f, d = w.flag_at(1, 1), w.data_at(1, 1)

    def preset(flags):
        w.model[0, f:f + 2] = flags
        w.model[0, d:d + n] = x[1]
        w.areas[0].copy_(torch.from_numpy(w.model[0]))

    preset([5, 3])                                            # call 5's flag, and call 3's own: no wait at all
    got = wait(seq=3)
    assert int(w.view[0]) == 0
    assert np.array_equal(got[:n], x[0]) and np.array_equal(got[n:], x[1])
