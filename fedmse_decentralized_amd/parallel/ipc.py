"""One-shot peer-memory exchange: the round's collectives without RCCL.

SURVEY §5.8 / §2.4 (b) ("optional C++ one-shot IPC all-gather ... benchmarked
against RCCL and selected by ``--comm ipc|rccl``").  The reference has no
transport at all (peers are Python objects, `src/Trainer/client_trainer.py:136-151`);
the default multi-GPU path here is RCCL (``parallel.comm.TorchDistComm``).
On an 8x MI355X node every GPU has a direct xGMI link to each peer and the
per-round exchange is a few hundred KB, so a collective's cost is latency:
RCCL's launch plus the hand-off to and from ProcessGroupNCCL's stream.

``IpcComm`` keeps the torch.distributed group for bring-up, barriers and
object exchange, and replaces the two per-round collectives of the device
protocol (``engine/device_round.py``) with two kernel launches each on the
caller's stream (``ops/csrc/hip/fedmx_ipc.hip``):

* ``all_gather_into`` (f32 [world * rows, P], main stream): push this rank's
  rows into every rank's receive area, then wait for every peer's flags and
  copy the gathered block out;
* ``all_reduce_inplace`` (f64, evaluation stream): push, then wait and sum
  the ranks' vectors in rank order (bit-identical on every rank; each entry
  of the protocol's vectors has one non-zero contributor, so the result
  equals RCCL's sum exactly).

Every rank allocates one receive area per channel in uncached device memory
and exports it with ``hipIpcGetMemHandle``; the handles travel through
``all_gather_object``; every rank opens its peers' areas.  Bring-up is
collective and checked: allocation, opening and a self-test exchange must
succeed on every rank, else every rank falls back to the torch.distributed
collectives (``IpcComm.active`` False) — never a mix.  Waits are bounded
(``FEDMX_IPC_TIMEOUT_S``, default 60 s): a peer that never arrives sets a
host-visible status word and ``check()`` raises.
"""
from __future__ import annotations

import ctypes
import logging
import os
from collections import Counter
from typing import Dict, List, Optional

import numpy as np
import torch

from .comm import TorchDistComm

log = logging.getLogger(__name__)


class IpcUnavailable(RuntimeError):
    pass


# spinning wait workgroups all co-located ranks may put on one GPU together
# (half of a gfx950's ~2,048 resident 256-thread workgroups)
WAIT_WORKGROUP_BUDGET = 1024


def wait_chunk_cap(world: int, ranks_on_device: int, max_chunks: int) -> int:
    """Chunks per source of one wait kernel such that the (chunks x world)
    wait grids of every rank sharing this GPU stay within
    WAIT_WORKGROUP_BUDGET (see _Channel)."""
    return max(1, min(max_chunks, WAIT_WORKGROUP_BUDGET // (max(1, world) * max(1, ranks_on_device))))


def job_chunk_cap(world: int, peer_devices, max_chunks: int) -> int:
    """The ONE chunk cap of a job: ``wait_chunk_cap`` for the busiest physical
    device (``peer_devices``: every rank's device identity, the same list on
    every rank).  The pusher and the receiver of a chunk must cut a call
    alike -- the push publishes flag c after writing [c * chunk_words, ...)
    and the wait on flag c reads [c * chunk_words, ...) -- so the cap cannot
    depend on how many ranks share the asking rank's own device: with 9 ranks
    on 8 GPUs that gave the two co-located ranks 1024 // (9 * 2) = 56 chunks
    and the seven others 64.  The budget argument still holds: the busiest
    device carries max_share x world x cap <= WAIT_WORKGROUP_BUDGET waiting
    workgroups, and every other device, with fewer ranks under the same cap,
    fewer than that."""
    ids = [tuple(i) for i in peer_devices]
    max_share = max(Counter(ids).values()) if ids else 1
    return wait_chunk_cap(world, max_share, max_chunks)


def chunk_plan(n_words: int, max_chunks: int, chunk_target: int = 1024):
    """(chunks, chunk_words) of one gather of ``n_words`` 32-bit words: about
    ``chunk_target`` words per chunk, at most ``max_chunks`` chunks, whole
    f32x4 per chunk, and no chunk that starts at or past ``n_words``."""
    n = int(n_words)
    chunks = max(1, min(int(max_chunks), -(-n // int(chunk_target))))
    cw = ((-(-n // chunks)) + 3) & ~3
    # (rounding chunk_words up to 4 can leave the last chunks empty: drop them)
    chunks = max(1, -(-n // cw)) if cw else 1
    return chunks, cw


class _Channel:
    """One receive area per rank plus the sequence counter of its calls."""

    def __init__(self, comm: "IpcComm", slot_words: int, chunk_target: int = 1024):
        from ..ops import _hip

        self.L = _hip.lib()
        self.H = _hip
        self.comm = comm
        W, me = comm.world_size, comm.rank
        if W > _hip.IPC_MAX_WORLD:
            raise IpcUnavailable(f"world size {W} > {_hip.IPC_MAX_WORLD}")
        self.world, self.rank = W, me
        self.slot_words = (int(slot_words) + 3) & ~3
        self.chunk_target = chunk_target
        # Spinning wait workgroups must never fill the device: every rank's
        # wait kernel is a (chunks x world) grid whose workgroups poll until
        # the peers' push kernels have run, and ranks that SHARE one GPU
        # (one-box rehearsals) each put such a grid on it.  A gfx950 device
        # holds ~2,048 of these 256-thread workgroups at once (8 per CU); 8
        # ranks x 8 sources x 64 chunks = 4,096 spinning workgroups could
        # leave the peers' push kernels no CU to run on.  The chunk count is
        # capped so that all co-located ranks' wait grids together stay
        # within half of that (1,024 workgroups); a job with one rank per GPU
        # keeps up to IPC_MAX_CHUNKS.  The cap is the job's, from its busiest
        # device, so that every rank cuts a call alike (job_chunk_cap).  (Round
        # 6 suspected this of round 5's failed second bring-up; the cap alone
        # did not cure it -- IpcComm._teardown.)
        self.max_chunks = job_chunk_cap(W, comm.device_identities(), _hip.IPC_MAX_CHUNKS)
        nbytes = 4 * (2 * W * self.slot_words + 2 * W * _hip.IPC_MAX_CHUNKS)
        hsz = self.L.fedmx_ipc_handle_size()
        handle = (ctypes.c_uint8 * hsz)()
        p = ctypes.c_void_p()
        # (retried locally: with several processes sharing one GPU an export
        # has failed transiently, hipErrorInvalidValue on one rank of 8)
        for attempt in range(3):
            rc = self.L.fedmx_ipc_alloc(nbytes, ctypes.byref(p), ctypes.cast(handle, ctypes.c_void_p))
            if rc == 0:
                break
            log.warning(f"rank {me}: receive-area allocation / export failed (code {rc}), attempt {attempt + 1}")
            import time

            time.sleep(0.2 * (attempt + 1))
        self.own = p.value if rc == 0 else None
        allh = comm.base_all_gather_object((rc, bytes(handle)))
        bad = [r for r, (c, _) in enumerate(allh) if c != 0]
        if bad:
            self.close()
            raise IpcUnavailable(f"receive-area allocation / export failed on ranks {bad} (codes "
                                 f"{[allh[r][0] for r in bad]})")
        self.opened: List[int] = []
        areas = [0] * W
        err = 0
        # ranks on distinct GPUs: the receive areas are read and written over
        # xGMI, so peer access must be possible before any handle is opened
        # (ranks sharing a GPU, as in one-box rehearsals, need none)
        idx = comm.base_all_gather_object(int(comm.device.index))
        nvis = torch.cuda.device_count()
        for r in range(W):
            o = idx[r]
            if r != me and o != idx[me] and 0 <= o < nvis and not torch.cuda.can_device_access_peer(idx[me], o):
                err = -2    # no peer access between this GPU and rank r's
                break
        for r, (_, h) in enumerate(allh):
            if err:
                break
            if r == me:
                areas[r] = self.own
                continue
            hb = (ctypes.c_uint8 * hsz).from_buffer_copy(h)
            q = ctypes.c_void_p()
            rc = self.L.fedmx_ipc_open(ctypes.cast(hb, ctypes.c_void_p), ctypes.byref(q))
            if rc != 0 or not q.value:
                err = rc or -1
                break
            areas[r] = q.value
            self.opened.append(q.value)
        errs = comm.base_all_gather_object(err)
        if any(errs):
            self.close()
            raise IpcUnavailable(f"opening peers' receive areas failed (codes per rank {errs})")
        self.areas = areas
        self.seq = 0

    def _args(self, src: int, out: int, n_words: int, chunks: int, chunk_words: int) -> "ctypes.Structure":
        self.seq += 1
        a = self.H.IpcArgs()
        for r, v in enumerate(self.areas):
            a.area[r] = v
        a.src, a.out, a.status = src, out, self.comm.status_ptr
        a.timeout_ticks = self.comm.timeout_ticks
        a.world, a.rank, a.n_words, a.slot_words = self.world, self.rank, n_words, self.slot_words
        a.parity, a.seq, a.chunks, a.chunk_words = self.seq & 1, self.seq, chunks, chunk_words
        return a

    def gather(self, out: torch.Tensor, t: torch.Tensor, stream: int) -> None:
        n = t.numel()
        chunks, cw = chunk_plan(n, self.max_chunks, self.chunk_target)
        a = self._args(t.data_ptr(), out.data_ptr(), n, chunks, cw)
        self.H._check(self.L.fedmx_ipc_push(ctypes.byref(a), stream), "fedmx_ipc_push")
        self.H._check(self.L.fedmx_ipc_wait_gather(ctypes.byref(a), stream), "fedmx_ipc_wait_gather")

    def reduce_f64(self, t: torch.Tensor, stream: int) -> None:
        n = 2 * t.numel()
        a = self._args(t.data_ptr(), t.data_ptr(), n, 1, (n + 3) & ~3)
        self.H._check(self.L.fedmx_ipc_push(ctypes.byref(a), stream), "fedmx_ipc_push")
        self.H._check(self.L.fedmx_ipc_wait_reduce_f64(ctypes.byref(a), stream), "fedmx_ipc_wait_reduce_f64")

    def retire(self) -> list:
        """Detach this channel's memory without releasing it (see
        IpcComm._teardown): returns [(kind, ptr)] for the final close."""
        out = [("opened", q) for q in getattr(self, "opened", [])]
        if getattr(self, "own", None):
            out.append(("own", self.own))
        self.opened, self.own = [], None
        return out

    def close(self) -> None:
        from ..ops import _hiprt

        try:
            _hiprt.device_sync()
        except Exception:
            pass
        for q in getattr(self, "opened", []):
            self.L.fedmx_ipc_close(ctypes.c_void_p(q))
        self.opened = []
        if getattr(self, "own", None):
            self.L.fedmx_ipc_free(ctypes.c_void_p(self.own))
            self.own = None


class IpcComm(TorchDistComm):
    """torch.distributed group + peer-memory channels for the round's
    device-tensor collectives.  Inactive until ``setup_exchange`` succeeded
    on every rank; calls that do not fit a channel use the base collectives."""

    def __init__(self, device: Optional[torch.device] = None):
        super().__init__(device)
        from ..ops import _hip, _hiprt

        self.active = False
        self.ipc_calls = 0
        self._retired: list = []   # [(kind, ptr)] of channels replaced by a larger bring-up
        self._gather: Optional[_Channel] = None
        self._reduce: Optional[_Channel] = None
        self._status = _hiprt.MappedBuffer(64)
        self._status_view = self._status.view(0, np.int32, 1)
        self._status_view[0] = 0
        self.status_ptr = self._status.dev_ptr
        khz = _hip.lib().fedmx_ipc_wall_khz()
        self._timeout_s = float(os.environ.get("FEDMX_IPC_TIMEOUT_S", "60"))
        self.timeout_ticks = int(self._timeout_s * 1e3 * (khz if khz > 0 else 100_000))
        self._hip = _hip

    # the base (torch.distributed) object exchange, also used during bring-up
    def base_all_gather_object(self, obj):
        return TorchDistComm.all_gather_object(self, obj)

    def device_identities(self) -> list:
        """Every rank's (host, physical GPU), the same list on every rank (the
        collective self-test's, or asked now); collective when not known yet."""
        ids = getattr(self, "peer_devices", None)
        if ids is None:
            from .launch import _device_identity

            ids = self.base_all_gather_object(_device_identity(self.device))
            self.peer_devices = ids
        return ids

    def setup_exchange(self, gather_words: int, reduce_words: int) -> bool:
        """Create (or keep, when large enough) the two channels; collective.
        Returns whether the peer-memory path is active on every rank."""
        if (self.active and self._gather.slot_words >= gather_words
                and self._reduce.slot_words >= reduce_words):
            return True
        self._teardown()
        ok, why = True, ""
        try:
            self._gather = _Channel(self, gather_words)
            self._reduce = _Channel(self, reduce_words)
        except IpcUnavailable as e:   # raised collectively: every rank saw the same codes
            ok, why = False, str(e)
        if ok:
            # a rank whose self-test fails (a launch error, a mismatch or a peer
            # that never arrives: the waits are bounded by a short timeout here)
            # still reaches the agreement below
            full = self.timeout_ticks
            self.timeout_ticks = max(1, full * 10 // max(1, int(self._timeout_s)))
            try:
                ok = self._self_test()
                why = "self-test mismatch or timeout" if not ok else ""
            except Exception as e:   # noqa: BLE001 - any local failure means: not on this rank
                ok, why = False, f"self-test failed: {e}"
            finally:
                self.timeout_ticks = full
                self._status_view[0] = 0
        # every rank takes the same path
        oks = self.base_all_gather_object(bool(ok))
        self.active = all(oks)
        if not self.active:
            self._teardown()
            if self.is_root:
                log.warning("peer-memory exchange unavailable (%s; ranks ok: %s): using %s collectives",
                            why or "another rank failed", oks, self.backend)
        return self.active

    def _self_test(self) -> bool:
        """Three gathers and two reduces with rank-specific patterns (both
        parities, reused buffers), checked on the host."""
        dev = self.device
        W, me = self.world_size, self.rank
        stream = torch.cuda.current_stream(dev).cuda_stream
        n = min(self._gather.slot_words, 4 * 4096 + 12)
        n -= n % 4
        ok = True
        bad = []   # which checks failed on this rank (logged: the agreement only says who)
        for it in range(3):
            src = (torch.arange(n, device=dev, dtype=torch.float32) * (it + 1) + 1000.0 * me)
            out = torch.full((W, n), -1.0, device=dev, dtype=torch.float32)
            self._gather.gather(out, src, stream)
            exp = torch.stack([torch.arange(n, device=dev, dtype=torch.float32) * (it + 1) + 1000.0 * r
                               for r in range(W)])
            torch.cuda.synchronize(dev)
            if not torch.equal(out, exp):
                ok = False
                wrong = (out != exp).any(dim=1).nonzero().flatten().tolist()
                bad.append(f"gather {it}: rows from ranks {wrong}")
        m = min(64, self._reduce.slot_words // (2 * W))   # doubles per rank block
        for it in range(2 if m >= 1 else 0):
            t = torch.zeros(W * m, device=dev, dtype=torch.float64)
            t[me * m:(me + 1) * m] = torch.arange(m, device=dev, dtype=torch.float64) + 0.5 * it + me
            self._reduce.reduce_f64(t, stream)
            exp = torch.cat([torch.arange(m, device=dev, dtype=torch.float64) + 0.5 * it + r for r in range(W)])
            torch.cuda.synchronize(dev)
            if not torch.equal(t, exp):
                ok = False
                bad.append(f"reduce {it}")
        if not self.status_ok():
            ok = False
            bad.append("a wait timed out")
        if bad:
            log.warning("rank %d: peer-memory self-test (slot %d words, n %d): %s", self.rank,
                        self._gather.slot_words, n, "; ".join(bad))
        return ok

    def status_ok(self) -> bool:
        return int(self._status_view[0]) == 0

    def check(self) -> None:
        """Raise if a wait timed out (a peer never arrived)."""
        if not self.status_ok():
            raise RuntimeError("peer-memory exchange: a wait timed out (a rank stalled or died); "
                               "rerun with FEDMX_COMM=rccl")

    def _teardown(self, release: bool = False):
        """Drop the current channels.  A re-bring-up (a federation needing
        larger slots) RETIRES them instead of freeing: round 6 reproduced round
        5's failed second bring-up of an 8-process one-GPU rehearsal
        (gpurun_out/s6: every peer's pushes never reached ONE rank's new
        receive area, whose waits timed out) after freeing the first areas and
        allocating new ones in the same processes; keeping every area and
        peer mapping alive until the final close (a few MB) gives each
        bring-up fresh allocations and fresh mappings.  ``release``: the final
        close frees everything."""
        for ch in (self._gather, self._reduce):
            if ch is None:
                continue
            if release:
                ch.close()
            else:
                self._hip_sync()
                self._retired += ch.retire()
        self._gather = self._reduce = None
        self.active = False
        if release and self._retired:
            L = self._hip.lib()
            for kind, q in self._retired:
                (L.fedmx_ipc_close if kind == "opened" else L.fedmx_ipc_free)(ctypes.c_void_p(q))
            self._retired = []

    def _hip_sync(self):
        from ..ops import _hiprt

        try:
            _hiprt.device_sync()
        except Exception:
            pass

    # ---- the device protocol's two collectives ------------------------------------
    def all_gather_into(self, out, t):
        ch = self._gather
        if (self.active and ch is not None and t.dtype == torch.float32 and out.dtype == torch.float32
                and t.device == self.device and out.device == self.device and t.is_contiguous()
                and out.is_contiguous() and t.numel() % 4 == 0 and t.numel() <= ch.slot_words
                and out.numel() == self.world_size * t.numel()):
            ch.gather(out, t, self._hip._stream(self.device))
            self.ipc_calls += 1
            return
        super().all_gather_into(out, t)

    def all_reduce_inplace(self, t):
        ch = self._reduce
        if (self.active and ch is not None and t.dtype == torch.float64 and t.device == self.device
                and t.is_contiguous() and t.numel() % 2 == 0 and 2 * t.numel() <= ch.slot_words):
            ch.reduce_f64(t, self._hip._stream(self.device))
            self.ipc_calls += 1
            return
        super().all_reduce_inplace(t)

    def close(self):
        self._teardown(release=True)
