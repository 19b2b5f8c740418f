"""ctypes bindings of ``libfedmx_hip.so`` (hand-written gfx950 kernels).

The library has a plain C ABI (no torch headers); device memory is owned by
torch tensors and passed as raw pointers together with the stream.

Host<->device protocol traffic avoids the torch copy machinery entirely
(``_hiprt``): descriptor arrays for per-round work are written into a mapped
pinned ring that kernels read directly, static work lists (the per-round
evaluation of every hosted client) are cached in device memory, and small
results (scores, drifts, AUCs, training tracking) are written by the kernels
straight into mapped pinned memory, read after one stream synchronisation
per protocol phase.

Loading fails loudly: on a GPU box the HIP engine must run these kernels,
never a silent PyTorch fallback.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hiprt, build

_lock = threading.Lock()
# compact internal order of the 4-wave kernel (batch <= 12, hidden <= 27,
# latent <= 7: padded k-steps skipped); FEDMX_TRAIN_COMPACT=0 forces the
# identity order (A/B timing, cross-checks)
TRAIN_COMPACT = os.environ.get("FEDMX_TRAIN_COMPACT", "1") != "0"
TRAIN_FLAG_NO_COMPACT = 1
TRAIN_FLAG_HELPER = 2
TRAIN_FLAG_NO_HELPER = 4
TRAIN_FLAG_TEST_DROP_W4 = 8   # tests only: inject a flag-wait timeout (fedmx_train_hw.hip)
TRAIN_FLAG_TEST_MUTE_VALIDATOR = 32   # tests only: client slot 0's validator never answers (0.2 s timeout)
# extra TrainArgs.flags bits OR'd into every launch (tests/test_train_failure_gpu.py)
TRAIN_TEST_FLAGS = 0
# helper-wave training kernel (fedmx_train_hw.hip: 8 waves, W4's gradient and
# Adam on a second wave per SIMD) for the compact shapes: "1" on, "0" off,
# unset: the library's build default
_HELPER_ENV = os.environ.get("FEDMX_TRAIN_HELPER")
TRAIN_HELPER = None if _HELPER_ENV is None else _HELPER_ENV != "0"
# asynchronous validation of the helper-wave kernel (validator workgroups
# beside the trainers, fedmx_train_hw.hip): "0" turns it off
TRAIN_ASYNC_VALID = os.environ.get("FEDMX_TRAIN_ASYNC_VALID", "1") != "0"
_lib = None
_lib_path: Optional[Path] = None

FWD_DTYPE = np.dtype([
    ("params", "<u8"), ("x", "<u8"), ("sse", "<u8"), ("lat", "<u8"),
    ("nrows", "<i4"), ("lat_stride", "<i4"), ("d_in", "<i4"), ("latent", "<i4"),
    ("hidden", "<i4"), ("pad0", "<i4"), ("pad1", "<i8"),
])
CEN_DTYPE = np.dtype([
    ("train_lat", "<u8"), ("test_lat", "<u8"), ("out", "<u8"),
    ("n_train", "<i4"), ("n_test", "<i4"), ("latent", "<i4"), ("stride", "<i4"),
])
# fedmx_knn.hip KnnDesc
KNN_DTYPE = np.dtype([
    ("train_lat", "<u8"), ("query_lat", "<u8"), ("out", "<u8"),
    ("n_train", "<i4"), ("n_query", "<i4"), ("latent", "<i4"), ("k", "<i4"),
    ("train_stride", "<i4"), ("query_stride", "<i4"),
])
KNN_MAX_K = 16           # neighbours knn_score_kernel keeps in registers (fedmx_knn.hip)
KNN_MAX_Y = 1024         # workgroups per descriptor a kNN launch spreads the query rows over, at most
AUC_DTYPE = np.dtype([
    ("score", "<u8"), ("label", "<u8"), ("out", "<u8"),
    ("n", "<i4"), ("score_is_f64", "<i4"), ("score_scale", "<f4"), ("pad", "<i4"),
])
# fedmx_auc_large.hip AucLargeDesc
AUC_LARGE_DTYPE = np.dtype([
    ("score", "<u8"), ("label", "<u8"), ("out", "<u8"), ("ws", "<u8"), ("ctr", "<u8"),
    ("n", "<i4"), ("score_is_f64", "<i4"), ("score_scale", "<f4"), ("pad", "<i4"),
])
AUC_MAX_SORT = 8192              # keys auc_kernel sorts in LDS; a larger smaller class takes the large path
AUC_LARGE_CTR_WORDS = 8          # u64 counters per descriptor (one 64-byte line)
AUC_LARGE_SLICE_MIN_ROWS = 1024  # a descriptor takes at most ceil(probe rows / this) slices
AUC_LARGE_MAX_ROWS = 1 << 26     # rows per (scores, labels) pair the large path accepts
AUC_LARGE_RESIDENT = 2 * 256     # pairs workgroups resident at once (1024 threads, 64 KB of LDS: 2 per CU, 256 CUs)
SEG_DTYPE = np.dtype([("sse", "<u8"), ("n", "<i4"), ("batch", "<i4"), ("out", "<u8")])
# fedmx_detect.hip DetectDesc
DETECT_DTYPE = np.dtype([
    ("calib", "<u8"), ("calib_label", "<u8"), ("score", "<u8"), ("label", "<u8"), ("out", "<u8"),
    ("n_c", "<i4"), ("n", "<i4"), ("j", "<i4"), ("calib_is_f64", "<i4"), ("score_is_f64", "<i4"),
    ("score_scale", "<f4"), ("value_is_recall", "<i4"), ("out_stride", "<i4"),
])
# fedmx_score.hip ScoreDesc
SCORE_DTYPE = np.dtype([
    ("params", "<u8"), ("raw", "<u8"), ("sc_a", "<u8"), ("sc_b", "<u8"), ("z_mean", "<u8"), ("z_scale", "<u8"),
    ("score", "<u8"), ("flag", "<u8"), ("lat", "<u8"), ("alarms", "<u8"), ("threshold", "<f8"),
    ("nrows", "<i4"), ("d_in", "<i4"), ("hidden", "<i4"), ("latent", "<i4"), ("flags", "<i4"), ("score_scale", "<f4"),
])
SCORE_RAW_F64, SCORE_MINMAX, SCORE_KIND_AE, SCORE_KIND_CEN = 1, 2, 4, 8
SCORE_CHUNK_ROWS = 64    # rows a score_rows workgroup takes per pass: four waves, one 16-row tile each
# fedmx_explain.hip ExplainDesc
EXPLAIN_DTYPE = np.dtype([
    ("params", "<u8"), ("raw", "<u8"), ("sc_a", "<u8"), ("sc_b", "<u8"), ("z_mean", "<u8"), ("z_scale", "<u8"),
    ("which", "<u8"), ("idx", "<u8"), ("resid", "<u8"), ("sse", "<u8"), ("resid_full", "<u8"), ("latent_terms", "<u8"),
    ("nrows", "<i4"), ("d_in", "<i4"), ("hidden", "<i4"), ("latent", "<i4"), ("flags", "<i4"), ("top_k", "<i4"),
])
# fedmx_monitor.hip MonitorDesc / MonitorFoldDesc / MonitorPartial / MonitorTotal
MONITOR_DTYPE = np.dtype([
    ("params", "<u8"), ("raw", "<u8"), ("sc_a", "<u8"), ("sc_b", "<u8"), ("z_mean", "<u8"), ("z_scale", "<u8"),
    ("lo", "<u8"), ("hi", "<u8"), ("edges", "<u8"), ("hist", "<u8"), ("lat", "<u8"), ("alarms", "<u8"),
    ("part", "<u8"), ("threshold", "<f8"),
    ("nrows", "<i4"), ("d_in", "<i4"), ("hidden", "<i4"), ("latent", "<i4"), ("flags", "<i4"), ("score_scale", "<f4"),
    ("nedges", "<i4"), ("pad", "<i4"),
])
MONITOR_FOLD_DTYPE = np.dtype([("part", "<u8"), ("total", "<u8"), ("nblocks", "<i4"), ("pad", "<i4")])
MONITOR_COLS = 128       # padded columns: one partial each
MONITOR_PARTIAL_DTYPE = np.dtype([
    ("sum", "<f8", (MONITOR_COLS,)), ("sq", "<f8", (MONITOR_COLS,)), ("mn", "<f4", (MONITOR_COLS,)),
    ("mx", "<f4", (MONITOR_COLS,)), ("cnt", "<u4", (MONITOR_COLS,)), ("bad", "<u4", (MONITOR_COLS,)),
    ("out", "<u4", (MONITOR_COLS,)), ("pad", "<u4", (MONITOR_COLS,)),
])
MONITOR_TOTAL_DTYPE = np.dtype([
    ("sum", "<f8", (MONITOR_COLS,)), ("sq", "<f8", (MONITOR_COLS,)), ("cnt", "<i8", (MONITOR_COLS,)),
    ("bad", "<i8", (MONITOR_COLS,)), ("out", "<i8", (MONITOR_COLS,)), ("mn", "<f4", (MONITOR_COLS,)),
    ("mx", "<f4", (MONITOR_COLS,)),
])
# fedmx_incident.hip IncidentItem / IncidentSpanDesc
INCIDENT_ITEM_DTYPE = np.dtype([
    ("flags", "<u8"), ("scores", "<u8"), ("totals", "<u8"), ("offs", "<u8"), ("start", "<u8"), ("end", "<u8"),
    ("pa", "<u8"), ("pb", "<u8"), ("key", "<u8"), ("enc", "<u8"), ("summary", "<u8"),
    ("n", "<i4"), ("nspans", "<i4"), ("window", "<i4"), ("min_alarms", "<i4"), ("hold", "<i4"), ("kmax", "<i4"),
])
INCIDENT_SPAN_DTYPE = np.dtype([("item", "<i4"), ("span", "<i4")])
INCIDENT_PHASES = {"mark": 1, "scan": 2, "emit": 4, "peak": 8, "finish": 16}
INCIDENT_MAX_ITEMS = 65535   # the finish launch's grid.y
# fedmx_signature.hip SigDesc / SigFoldDesc / SigPartial
SIG_DTYPE = np.dtype([
    ("params", "<u8"), ("raw", "<u8"), ("sc_a", "<u8"), ("sc_b", "<u8"), ("which", "<u8"), ("seg", "<u8"),
    ("part", "<u8"),
    ("nrows", "<i4"), ("d_in", "<i4"), ("hidden", "<i4"), ("latent", "<i4"), ("flags", "<i4"), ("block", "<i4"),
    ("nslots", "<i4"), ("pad", "<i4"),
])
SIG_FOLD_DTYPE = np.dtype([
    ("part", "<u8"), ("err_sum", "<u8"), ("resid_sum", "<u8"), ("bad", "<u8"),
    ("seg", "<i4"), ("first", "<i4"), ("last", "<i4"), ("d_in", "<i4"),
])
SIG_WAVES = 4
SIG_PARTIAL_DTYPE = np.dtype([
    ("se", "<f8", (SIG_WAVES, MONITOR_COLS)), ("sr", "<f8", (SIG_WAVES, MONITOR_COLS)),
    ("bad", "<u4", (SIG_WAVES, MONITOR_COLS)),
])
from ..deploy.detector import (EXPLAIN_MAX_K, MONITOR_MAX_EDGES, check_incident_params, check_incident_rows,  # noqa: E402
                               check_top_k, check_which, incident_bound)   # (the rules' one definition)


class TrainArgs(ctypes.Structure):
    _fields_ = [
        ("params", ctypes.c_void_p), ("adam_m", ctypes.c_void_p), ("adam_v", ctypes.c_void_p),
        ("anchor", ctypes.c_void_p), ("best", ctypes.c_void_p), ("adam_step", ctypes.c_void_p),
        ("train_x", ctypes.c_void_p), ("train_off", ctypes.c_void_p),
        ("valid_x", ctypes.c_void_p), ("valid_off", ctypes.c_void_p),
        ("client_idx", ctypes.c_void_p), ("tracking", ctypes.c_void_p),
        ("epochs_run", ctypes.c_void_p), ("best_epoch", ctypes.c_void_p),
        ("epochs", ctypes.c_int32), ("batch", ctypes.c_int32), ("patience", ctypes.c_int32),
        ("d_in", ctypes.c_int32), ("hidden", ctypes.c_int32), ("latent", ctypes.c_int32),
        ("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
        ("eps", ctypes.c_float), ("lam", ctypes.c_float), ("mu", ctypes.c_float),
        ("stamps", ctypes.c_void_p), ("flags", ctypes.c_int32), ("pad0", ctypes.c_int32),
        ("err", ctypes.c_void_p), ("vws", ctypes.c_void_p), ("vseq", ctypes.c_uint32), ("pad1", ctypes.c_int32),
    ]


_vp, _i32 = ctypes.c_void_p, ctypes.c_int32


class ElectArgs(ctypes.Structure):
    _fields_ = [("sel", _vp), ("vec", _vp), ("noise", _vp), ("agg_counts", _vp), ("weights", _vp), ("state", _vp),
                ("report", _vp), ("k", _i32), ("cap", _i32), ("rule", _i32), ("mode", _i32), ("rec", _vp),
                ("hw", _vp), ("vote_cap", ctypes.c_double), ("fallback_u", ctypes.c_double),
                ("err", _vp), ("err_n", _i32), ("err_stride", _i32)]


ELECT_TRAIN_FAILED = -3   # report[0] of a round whose training launch failed (TrainArgs.err set)


class WsumArgs(ctypes.Structure):
    _fields_ = [("base", _vp), ("rows", _vp), ("weights", _vp), ("state", _vp), ("out", _vp), ("k", _i32), ("P", _i32)]


class DecideArgs(ctypes.Structure):
    _fields_ = [("params", _vp), ("anchor", _vp), ("hist", _vp), ("agg", _vp), ("state", _vp), ("sse", _vp),
                ("sse_off", _vp), ("sse_n", _vp), ("seg", _vp), ("agg_counts", _vp), ("has_hist", _vp),
                ("hist_perf", _vp), ("rejected", _vp), ("rej_out", _vp),
                ("thr", ctypes.c_double), ("pthr", ctypes.c_double), ("start", _i32), ("n_local", _i32),
                ("P", _i32), ("d_in", _i32), ("mode", _i32), ("pad", _i32)]


VERIFY_MAX_ROWS = 4096   # rows of one receiver's verification data the fused kernel keeps in LDS
ROBUST_MAX_K = 1024      # models one robust_agg_kernel tile ranks (elect_wsum's row table has the same bound)
KRUM_MAX_K = 1024        # models the krum kernels rank in LDS (fedmx_krum.hip)
GEOMED_MAX_K = 1024      # models whose weights geomed_step_kernel keeps in LDS (fedmx_geomed.hip)
GEOMED_MAX_ITERS = 64    # Weiszfeld iterations of one geomed_aggregate (T + 2 launches)

IPC_MAX_WORLD = 16
IPC_MAX_CHUNKS = 64


class IpcArgs(ctypes.Structure):
    """fedmx_ipc.hip: one push / wait launch of the peer-memory exchange."""
    _fields_ = [("area", ctypes.c_uint64 * IPC_MAX_WORLD), ("src", _vp), ("out", _vp), ("status", _vp),
                ("timeout_ticks", ctypes.c_int64), ("world", _i32), ("rank", _i32), ("n_words", _i32),
                ("slot_words", _i32), ("parity", _i32), ("seq", _i32), ("chunks", _i32), ("chunk_words", _i32)]


class VerifyArgs(ctypes.Structure):
    _fields_ = [("D", DecideArgs), ("vx", _vp), ("vn", _vp), ("eval_params", _vp), ("best_stage", _vp),
                ("best", _vp), ("latent", _i32), ("hidden", _i32)]


class VerifySplitArgs(ctypes.Structure):
    """fedmx_protocol.hip verify_split_kernel: per-receiver scratch (SSE rows,
    drift granule, arrival counter) and the forward workgroups per receiver."""
    _fields_ = [("sse", _vp), ("drift", _vp), ("count", _vp), ("splits", _i32), ("pad", _i32),
                ("done", _vp), ("seq", ctypes.c_uint32), ("pad2", _i32)]


# split verification (round 6): the verification forward over several
# workgroups per receiver, a drift workgroup beside them, the last arriver
# decides; "0" keeps the one-workgroup-per-receiver fused kernel
VERIFY_SPLIT = os.environ.get("FEDMX_VERIFY_SPLIT", "1") != "0"
# side-stream hand-off (round 6): with split verification, the round's
# evaluation waits on the verification kernel's hand-off word (side_wait)
# instead of an event recorded on the main stream; "0" keeps the event
SIDE_FLAG = os.environ.get("FEDMX_SIDE_FLAG", "1") != "0"


def lib():
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            override = os.environ.get("FEDMX_HIP_LIB")
            path = Path(override) if override else build.HIP_LIB
            if not path.exists() and not override:
                build.build_hip()   # hipcc cross-compiles for gfx950 in-tree
            L = ctypes.CDLL(str(path))
            global _lib_path
            _lib_path = path
            vp, i32 = ctypes.c_void_p, ctypes.c_int
            sig = {
                "fedmx_forward_rows": [vp, i32, vp],
                "fedmx_weighted_sum": [vp, vp, i32, i32, vp, vp],
                "fedmx_robust_agg": [vp, vp, vp, vp, i32, i32, i32, vp],
                "fedmx_robust_max_k": [],
                "fedmx_krum_agg": [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp],
                "fedmx_krum_max_k": [],
                "fedmx_krum_tile": [],
                "fedmx_geomed_agg": [vp, vp, vp, vp, i32, i32, i32, ctypes.c_double, vp, vp, vp, vp],
                "fedmx_geomed_max_k": [],
                "fedmx_param_drift": [vp, i32, vp, vp, vp, vp],
                "fedmx_standardize_lds": [vp, i32, i32, vp, vp],
                "fedmx_cen_score": [vp, i32, vp],
                "fedmx_knn_score": [vp, i32, i32, i32, vp],
                "fedmx_knn_tile_rows": [],
                "fedmx_knn_max_k": [],
                "fedmx_auc": [vp, i32, vp],
                "fedmx_auc_large": [vp, i32, i32, i32, i32, i32, vp],
                "fedmx_detect": [vp, i32, vp],
                "fedmx_score_rows": [vp, i32, vp],
                "fedmx_score_chunk_rows": [],
                "fedmx_explain_rows": [vp, i32, vp],
                "fedmx_explain_max_k": [],
                "fedmx_monitor_rows": [vp, i32, vp, i32, vp],
                "fedmx_monitor_fold": [vp, i32, vp],
                "fedmx_monitor_max_edges": [],
                "fedmx_incidents": [vp, i32, vp, i32, i32, i32, vp],
                "fedmx_incident_span_rows": [],
                "fedmx_incident_signatures": [vp, i32, vp, i32, vp],
                "fedmx_score_reduce": [vp, i32, i32, vp],
                "fedmx_score_reduce_copy": [vp, i32, i32, vp, i32, vp],
                "fedmx_broadcast_rows": [vp, vp, vp, i32, vp, i32, vp],
                "fedmx_train": [ctypes.POINTER(TrainArgs), i32, vp],
                "fedmx_probe_mfma": [vp, vp],
                "fedmx_elect_wsum": [ctypes.POINTER(ElectArgs), ctypes.POINTER(WsumArgs), vp],
                "fedmx_decide_adopt": [ctypes.POINTER(DecideArgs), vp],
                "fedmx_verify_decide": [ctypes.POINTER(VerifyArgs), vp],
                "fedmx_verify_split": [ctypes.POINTER(VerifyArgs), ctypes.POINTER(VerifySplitArgs), vp],
                "fedmx_side_wait": [vp, ctypes.c_uint32, vp, ctypes.c_longlong, vp],
                "fedmx_copy_f64": [vp, vp, i32, vp],
                "fedmx_copy2_f64": [vp, vp, i32, vp, vp, i32, vp],
                "fedmx_copy_rows": [vp, i32, vp, vp, i32, vp, i32, i32, vp],
                "fedmx_protocol_sizes": [vp],
                "fedmx_train_av_slot": [],
                "fedmx_train_hw_last_grid": [],
                # one-shot peer-memory exchange (fedmx_ipc.hip, parallel/ipc.py)
                "fedmx_ipc_alloc": [ctypes.c_size_t, ctypes.POINTER(vp), vp],
                "fedmx_ipc_open": [vp, ctypes.POINTER(vp)],
                "fedmx_ipc_close": [vp],
                "fedmx_ipc_free": [vp],
                "fedmx_ipc_push": [vp, vp],
                "fedmx_ipc_wait_gather": [vp, vp],
                "fedmx_ipc_wait_reduce_f64": [vp, vp],
            }
            for name, args in sig.items():
                f = getattr(L, name)
                f.argtypes = args
                f.restype = ctypes.c_int
            assert L.fedmx_fwd_desc_size() == FWD_DTYPE.itemsize
            assert L.fedmx_cen_desc_size() == CEN_DTYPE.itemsize
            assert L.fedmx_knn_desc_size() == KNN_DTYPE.itemsize
            assert L.fedmx_auc_desc_size() == AUC_DTYPE.itemsize
            assert L.fedmx_auc_large_desc_size() == AUC_LARGE_DTYPE.itemsize
            assert L.fedmx_auc_large_ctr_words() == AUC_LARGE_CTR_WORDS
            assert L.fedmx_auc_large_slice_min_rows() == AUC_LARGE_SLICE_MIN_ROWS
            assert L.fedmx_auc_large_max_rows() == AUC_LARGE_MAX_ROWS
            assert L.fedmx_detect_desc_size() == DETECT_DTYPE.itemsize
            assert L.fedmx_score_desc_size() == SCORE_DTYPE.itemsize
            assert L.fedmx_score_chunk_rows() == SCORE_CHUNK_ROWS
            assert L.fedmx_explain_desc_size() == EXPLAIN_DTYPE.itemsize
            assert L.fedmx_explain_max_k() == EXPLAIN_MAX_K
            assert L.fedmx_monitor_desc_size() == MONITOR_DTYPE.itemsize
            assert L.fedmx_monitor_fold_desc_size() == MONITOR_FOLD_DTYPE.itemsize
            assert L.fedmx_monitor_partial_size() == MONITOR_PARTIAL_DTYPE.itemsize
            assert L.fedmx_monitor_total_size() == MONITOR_TOTAL_DTYPE.itemsize
            assert L.fedmx_monitor_max_edges() == MONITOR_MAX_EDGES
            assert L.fedmx_incident_item_size() == INCIDENT_ITEM_DTYPE.itemsize
            assert L.fedmx_incident_span_desc_size() == INCIDENT_SPAN_DTYPE.itemsize
            assert L.fedmx_incident_span_rows() >= 8192 + 4098
            assert L.fedmx_sig_desc_size() == SIG_DTYPE.itemsize
            assert L.fedmx_sig_fold_desc_size() == SIG_FOLD_DTYPE.itemsize
            assert L.fedmx_sig_partial_size() == SIG_PARTIAL_DTYPE.itemsize
            assert L.fedmx_seg_desc_size() == SEG_DTYPE.itemsize
            assert L.fedmx_train_args_size() == ctypes.sizeof(TrainArgs)
            sz = (ctypes.c_int * 4)()
            L.fedmx_protocol_sizes(ctypes.cast(sz, ctypes.c_void_p))
            assert tuple(sz) == (ctypes.sizeof(ElectArgs), ctypes.sizeof(WsumArgs), ctypes.sizeof(DecideArgs),
                                 ctypes.sizeof(VerifyArgs)), tuple(sz)
            assert L.fedmx_ipc_args_size() == ctypes.sizeof(IpcArgs)
            assert L.fedmx_verify_split_args_size() == ctypes.sizeof(VerifySplitArgs)
            assert L.fedmx_ipc_max_world() == IPC_MAX_WORLD and L.fedmx_ipc_max_chunks() == IPC_MAX_CHUNKS
            assert L.fedmx_robust_max_k() == ROBUST_MAX_K
            assert L.fedmx_krum_max_k() == KRUM_MAX_K
            assert L.fedmx_geomed_max_k() == GEOMED_MAX_K
            assert L.fedmx_knn_max_k() == KNN_MAX_K
            _lib = L
    return _lib


def lib_path() -> str:
    """Path of the kernel library this process loaded (FEDMX_HIP_LIB variants)."""
    lib()
    return str(_lib_path)


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed with HIP error code {rc}")


class Runtime:
    """Per-device launch context: the stream plus the mapped descriptor / result rings.

    ``Runtime(device)`` is the process's default context (``runtime()``);
    ``Runtime(device, private=True)`` is an independent one with its own
    non-blocking stream and rings, made current with ``use_runtime`` — e.g.
    one per federation when several run concurrently on one GPU
    (``main.py --concurrent-combos``)."""

    def __init__(self, device: torch.device, private: bool = False):
        self.device = device
        if private:
            s = torch.cuda.Stream(device=device)
            self.torch_stream = s
            self.stream = s.cuda_stream
            self.desc = _hiprt.DescRing(1 << 20, self.stream)
            self.out = _hiprt.OutRing(1 << 20, self.stream)
            return
        cur = torch.cuda.current_stream(device)
        self.torch_stream = None
        if cur.cuda_stream == 0 and os.environ.get("FEDMX_NULL_STREAM", "0") != "1":
            # Never work on the legacy null stream: it implicitly serialises
            # with every blocking stream, and RCCL's bookkeeping on it made each
            # round's training wait for the previous round's side-stream
            # evaluation (+125 us per round with a one-rank RCCL group).  One
            # non-blocking stream becomes torch's current stream of this thread,
            # so torch ops, our launches and the collectives share one order.
            s = torch.cuda.Stream(device=device)
            s.wait_stream(cur)
            torch.cuda.set_stream(s)
            self.torch_stream = s
            _tls.rt_thread = self
            cur = s
        self.stream = cur.cuda_stream
        self.desc = _hiprt.DescRing(4 << 20, self.stream)
        self.out = _hiprt.OutRing(4 << 20, self.stream)

    def sync(self):
        _hiprt.stream_sync(self.stream)


_runtimes: Dict[Tuple[str, int], Runtime] = {}


_tls = threading.local()


def runtime(device: torch.device) -> Runtime:
    ov = getattr(_tls, "rt_override", None)
    if ov is not None and (device.index is None or device.index == ov.device.index):
        return ov
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    r = _runtimes.get(key)
    if r is None:
        r = _runtimes[key] = Runtime(torch.device("cuda", key[1]))
    if r.torch_stream is not None and getattr(_tls, "rt_thread", None) is not r:
        # torch's current stream is per thread: a thread that first touches the
        # runtime while still on the null stream joins the runtime's stream
        if torch.cuda.current_stream(r.device).cuda_stream == 0:
            r.torch_stream.wait_stream(torch.cuda.current_stream(r.device))
            torch.cuda.set_stream(r.torch_stream)
        _tls.rt_thread = r
    return r


def _stream(device: torch.device) -> int:
    s = getattr(_tls, "stream", None)
    return s if s is not None else runtime(device).stream


class use_runtime:
    """Make a private ``Runtime`` current for this thread: every launch, ring
    descriptor and torch op inside the block goes to its stream.  ``None``
    is a no-op (CPU engines)."""

    def __init__(self, rt: Optional[Runtime]):
        self.rt = rt
        self._ctx = torch.cuda.stream(rt.torch_stream) if rt is not None else None

    def __enter__(self):
        if self.rt is not None:
            self._prev = getattr(_tls, "rt_override", None)
            _tls.rt_override = self.rt
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.rt is not None:
            self._ctx.__exit__(*exc)
            _tls.rt_override = self._prev
        return False


class on_stream:
    """Route the cached-plan launches (FwdPlan.run, launch_cen / launch_auc /
    launch_auc_large / launch_score_reduce, copy kernels) to another HIP stream (a
    ``torch.cuda.Stream``), e.g. evaluation overlapping the next round's
    training; torch work inside the block follows the same stream."""

    def __init__(self, stream: "torch.cuda.Stream"):
        self.stream = stream
        self._ctx = torch.cuda.stream(stream)

    def __enter__(self):
        self._prev = getattr(_tls, "stream", None)
        _tls.stream = self.stream.cuda_stream
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self._ctx.__exit__(*exc)
        _tls.stream = self._prev
        return False


# ---------------------------------------------------------------------------
FWD_BLOCK_SLOTS = 4 * 256   # fwd_rows workgroups the LDS admits at once (40 KB each, 4 per CU, 256 CUs)
FWD_RESIDENT = 2 * 256      # ... and the VGPRs (~197 per lane: 2 waves per SIMD -> 2 workgroups per CU)


def fwd_rows_per_block(total_rows: int, n_items: int) -> int:
    """Rows per fwd_rows workgroup (multiple of 64): about one workgroup per
    LDS slot, then grown while the block count would leave only a sliver of
    workgroups for a last wave of residency (the headline's 33.8 K vote /
    dev rows: 535 blocks of 64 rows -> 265 of 128, the 23 blocks past the
    first 512 ran alone; -0.25 % round time).  Big scorings keep small
    blocks (8-rank dev set: 836 blocks of 320 rows beat 460 of 576)."""
    fixed = int(os.environ.get("FEDMX_FWD_ROWS_PER_BLOCK", "0"))   # A/B override
    if fixed > 0:
        return fixed
    slots = max(FWD_BLOCK_SLOTS - n_items, 1)
    per = -(-int(total_rows) // slots)
    per = max(64, -(-per // 64) * 64)

    def blocks(rpb):
        return -(-int(total_rows) // rpb) + n_items

    waves = blocks(per) / FWD_RESIDENT
    target = FWD_RESIDENT * int(waves)
    # every item keeps at least one block: growing the blocks can only help
    # while the items alone fit in the target (else the loop would never end)
    if waves > 1 and waves - int(waves) < 0.25 and n_items + 1 <= target:
        while blocks(per) > target and per < total_rows:
            per += 64
    return int(per)


_FWD_LAYOUTS: "OrderedDict" = None   # (x ptrs, row counts, rows per block) -> block layout (LRU)


def _fwd_layout(x_ptrs: np.ndarray, nrows: np.ndarray, rpb: int):
    """Block layout of a forward launch: item and first row of every block
    (filler blocks: item -1) in dispatch order.  Cached: the vote / dev-set
    scorings repeat the same shapes every round (building the XCD-grouped
    order took 0.1-0.5 ms of host time per round at 8 ranks)."""
    global _FWD_LAYOUTS
    from collections import OrderedDict

    if _FWD_LAYOUTS is None:
        _FWD_LAYOUTS = OrderedDict()
    # the layout depends on which items share their rows, not on the addresses
    # (the vote data changes with every round's voter): key on the sharing
    # pattern, items labelled by the first item with the same address
    _, first_of, label = np.unique(x_ptrs, return_index=True, return_inverse=True)
    key = (first_of[label].astype(np.int64).tobytes(), nrows.tobytes(), int(rpb))
    hit = _FWD_LAYOUTS.get(key)
    if hit is not None:
        _FWD_LAYOUTS.move_to_end(key)
        return hit
    nblk = (nrows + rpb - 1) // rpb
    item = np.repeat(np.arange(len(nrows)), nblk)
    first = np.repeat(np.cumsum(nblk) - nblk, nblk)
    r0 = (np.arange(int(nblk.sum())) - first) * rpb
    order = _xcd_order(x_ptrs[: len(nrows)], nrows, nblk)
    if order is not None:
        pad = order < 0
        sel = np.where(pad, 0, order)
        item = np.where(pad, -1, item[sel])
        r0 = np.where(pad, 0, r0[sel])
    layout = (item, r0)
    _FWD_LAYOUTS[key] = layout
    while len(_FWD_LAYOUTS) > 256:
        _FWD_LAYOUTS.popitem(last=False)
    return layout


def build_fwd_desc(param_ptrs: np.ndarray, x_ptrs: np.ndarray, nrows: np.ndarray, sse_ptrs: np.ndarray,
                   lat_ptrs: np.ndarray, dims, rows_per_block: Optional[int] = None) -> np.ndarray:
    """Vectorised FwdDesc construction: split items into row blocks (the
    kernel loops over any block length in 16-row tiles)."""
    nrows = np.asarray(nrows, dtype=np.int64)
    x_ptrs = np.asarray(x_ptrs, dtype=np.int64)
    rpb = rows_per_block or fwd_rows_per_block(int(nrows.sum()), len(nrows))
    item, r0 = _fwd_layout(x_ptrs, nrows, rpb)
    live = item >= 0
    it = np.where(live, item, 0)
    desc = np.zeros(len(item), dtype=FWD_DTYPE)
    desc["params"] = np.asarray(param_ptrs, dtype=np.int64)[it]
    desc["x"] = x_ptrs[it] + (4 * 128) * r0
    sp = np.asarray(sse_ptrs, dtype=np.int64)[it]
    lp = np.asarray(lat_ptrs, dtype=np.int64)[it]
    desc["sse"] = np.where(sp != 0, sp + 4 * r0, 0)
    desc["lat"] = np.where(lp != 0, lp + 4 * dims.latent * r0, 0)
    desc["nrows"] = np.where(live, np.minimum(rpb, nrows[it] - r0), 0)   # filler: no rows, exits at once
    desc["lat_stride"] = dims.latent
    desc["d_in"] = dims.d_in
    desc["latent"] = dims.latent
    desc["hidden"] = dims.hidden
    return desc


XCDS = 8   # blocks b and b + 8 share an XCD (and its 4 MB L2) on the MI355X dispatcher


def _xcd_order(x_ptrs: np.ndarray, nrows: np.ndarray, nblk: np.ndarray) -> Optional[np.ndarray]:
    """Block order that puts every model's blocks of the same row range on
    one XCD.  Items that score several models on the same rows (the FedMSE
    dev set: every selected model over N x 6.6 K shared rows) are laid out
    in chunks of 8 row ranges, model after model, each chunk starting at a
    multiple of 8 (filler blocks keep the alignment), so block b and the
    other models' blocks of its rows share b % 8: the rows come from HBM
    once per XCD L2 instead of once per model.  None: nothing to group."""
    first = np.cumsum(nblk) - nblk
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, (xp, n) in enumerate(zip(x_ptrs.tolist(), nrows.tolist())):
        groups.setdefault((int(xp), int(n)), []).append(i)
    shared = [g for g in groups.values() if len(g) > 1 and nblk[g[0]] >= XCDS]
    if not shared:
        return None
    order: List[int] = []
    done = np.zeros(len(nrows), dtype=bool)
    for g in shared:
        nb = int(nblk[g[0]])
        for c0 in range(0, nb, XCDS):
            cnt = min(XCDS, nb - c0)
            for it in g:
                order.extend(range(int(first[it]) + c0, int(first[it]) + c0 + cnt))
                order.extend([-1] * ((-len(order)) % XCDS))
        done[g] = True
    for i in np.flatnonzero(~done):
        order.extend(range(int(first[i]), int(first[i]) + int(nblk[i])))
    return np.asarray(order, dtype=np.int64)


def _check_rows(items, dev):
    for _, x in items:
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 128 or not x.is_contiguous() or x.device != dev:
            raise ValueError("forward_rows expects contiguous float32 [n, 128] inputs on the params device")


def forward_rows(params: torch.Tensor, items, dims, want_sse=True, want_latent=False):
    """items: sequence of (param_row, x[n, DP]).  Returns (sse list, latent list) on device."""
    dev = params.device
    _check_rows(items, dev)
    rt = runtime(dev)
    sizes = np.array([int(x.shape[0]) for _, x in items], dtype=np.int64)
    tot = int(sizes.sum())
    sse_all = torch.empty(tot, dtype=torch.float32, device=dev) if want_sse else None
    lat_all = torch.empty(tot, dims.latent, dtype=torch.float32, device=dev) if want_latent else None
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    P = params.shape[1]
    pptr = params.data_ptr() + 4 * P * np.array([int(r) for r, _ in items], dtype=np.int64)
    xptr = np.array([x.data_ptr() for _, x in items], dtype=np.int64)
    sptr = (sse_all.data_ptr() + 4 * offs) if want_sse else np.zeros(len(items), np.int64)
    lptr = (lat_all.data_ptr() + 4 * dims.latent * offs) if want_latent else np.zeros(len(items), np.int64)
    desc = build_fwd_desc(pptr, xptr, sizes, sptr, lptr, dims)
    if len(desc):
        (dptr,) = rt.desc.put(desc)
        _check(lib().fedmx_forward_rows(dptr, len(desc), rt.stream), "fedmx_forward_rows")
    sse_l = [sse_all[o:o + n] for o, n in zip(offs, sizes)] if want_sse else []
    lat_l = [lat_all[o:o + n] for o, n in zip(offs, sizes)] if want_latent else []
    return sse_l, lat_l


class FwdPlan:
    """A cached forward launch over fixed (param row, buffer) items."""

    def __init__(self, params: torch.Tensor, items, dims, want_sse: bool, want_latent: bool):
        dev = params.device
        _check_rows(items, dev)
        self.params = params
        self.device = dev
        self.sizes = np.array([int(x.shape[0]) for _, x in items], dtype=np.int64)
        tot = int(self.sizes.sum())
        self.sse = torch.empty(tot, dtype=torch.float32, device=dev) if want_sse else None
        self.lat = torch.empty(tot, dims.latent, dtype=torch.float32, device=dev) if want_latent else None
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)[:-1]]).astype(np.int64)
        P = params.shape[1]
        pptr = params.data_ptr() + 4 * P * np.array([int(r) for r, _ in items], dtype=np.int64)
        xptr = np.array([x.data_ptr() for _, x in items], dtype=np.int64)
        sptr = (self.sse.data_ptr() + 4 * self.offs) if want_sse else np.zeros(len(items), np.int64)
        lptr = (self.lat.data_ptr() + 4 * dims.latent * self.offs) if want_latent else np.zeros(len(items), np.int64)
        desc = build_fwd_desc(pptr, xptr, self.sizes, sptr, lptr, dims)
        self.nblocks = len(desc)
        self.desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        self._keep = [x for _, x in items]

    def run(self):
        if self.nblocks:
            _check(lib().fedmx_forward_rows(self.desc.data_ptr(), self.nblocks, _stream(self.device)),
                   "fedmx_forward_rows")

    def sse_views(self):
        return [self.sse[o:o + n] for o, n in zip(self.offs, self.sizes)]

    def lat_views(self):
        return [self.lat[o:o + n] for o, n in zip(self.offs, self.sizes)]


def _cen_rows(t: torch.Tensor, latent: int, what: str):
    # (the strides of a dimension of one element, or of a tensor without rows, are never applied)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < latent or (
            t.shape[0] > 0 and t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"cen: {what} must be float32 [n, >= {latent}] with unit column stride")


def cen_desc(train_lat, test_lat, out: torch.Tensor, latent: int) -> Tuple[np.ndarray, List[torch.Tensor]]:
    """CenDesc array (fedmx_eval.hip): item i scores every row of
    ``test_lat[i]`` against the scaler fitted on ``train_lat[i]`` into
    consecutive float64 slots of ``out``.  The kernel reads both tensors of
    an item with one row stride, so they must share it (equal-stride views of
    wider buffers are fine; the stride of a tensor of at most one row is
    never applied and not compared).  Raises ValueError otherwise, for a tensor with
    fewer than ``latent`` columns or a column stride other than 1; nothing is
    launched.  Returns (descriptors, per-item views of ``out``)."""
    if len(train_lat) != len(test_lat):
        raise ValueError("cen: one test set per train set")
    n = len(train_lat)
    desc = np.zeros(n, dtype=CEN_DTYPE)
    views, off = [], 0
    for i, (tr, te) in enumerate(zip(train_lat, test_lat)):
        _cen_rows(tr, latent, "train latents")
        _cen_rows(te, latent, "test latents")
        # a tensor of at most one row is read at its first row only: its row stride is immaterial
        strides = {int(t.stride(0)) for t in (tr, te) if t.shape[0] > 1}
        if len(strides) > 1:
            raise ValueError(f"cen: train and test latents of item {i} have row strides {tr.stride(0)} and "
                             f"{te.stride(0)}; the kernel reads both with one")
        desc[i]["train_lat"] = tr.data_ptr()
        desc[i]["test_lat"] = te.data_ptr()
        desc[i]["out"] = out.data_ptr() + 8 * off
        desc[i]["n_train"] = tr.shape[0]
        desc[i]["n_test"] = te.shape[0]
        desc[i]["latent"] = latent
        desc[i]["stride"] = strides.pop() if strides else tr.stride(0)
        views.append(out[off:off + te.shape[0]])
        off += te.shape[0]
    return desc, views


def cen_scores(train_lat: Sequence[torch.Tensor], test_lat: Sequence[torch.Tensor], latent: int):
    dev = train_lat[0].device
    rt = runtime(dev)
    out_all = torch.empty(sum(int(t.shape[0]) for t in test_lat), dtype=torch.float64, device=dev)
    desc, views = cen_desc(train_lat, test_lat, out_all, latent)
    (dptr,) = rt.desc.put(desc)
    _check(lib().fedmx_cen_score(dptr, len(desc), rt.stream), "fedmx_cen_score")
    return views


def knn_tile_rows() -> int:
    """Train rows one LDS tile of knn_score_kernel holds."""
    return int(lib().fedmx_knn_tile_rows())


def knn_grid_y(query_lat) -> int:
    """Workgroups per descriptor of a kNN launch: one 256-row pass over the
    largest query set, capped (more rows take more passes)."""
    nq = max((int(q.shape[0]) for q in query_lat), default=0)
    return max(1, min((nq + 255) // 256, KNN_MAX_Y))


def _lat_rows(t: torch.Tensor, latent: int, what: str):
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < latent or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"knn: {what} must be float32 [n, >= {latent}] with unit column stride")


def knn_desc(train_lat, query_lat, out: torch.Tensor, latent: int, k: int) -> Tuple[np.ndarray, List[torch.Tensor]]:
    """KnnDesc array (fedmx_knn.hip): item i scores every row of
    ``query_lat[i]`` against ``train_lat[i]`` into consecutive float64 slots
    of ``out``.  Returns (descriptors, per-item views of ``out``)."""
    if not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError(f"knn: k must lie in 1..{KNN_MAX_K}, got {k!r}")
    if not 1 <= int(latent) <= 16:
        raise ValueError(f"knn: latent must lie in 1..16, got {latent!r}")
    if len(train_lat) != len(query_lat):
        raise ValueError("knn: one query set per train set")
    n = len(train_lat)
    desc = np.zeros(n, dtype=KNN_DTYPE)
    views, off = [], 0
    for i, (tr, qu) in enumerate(zip(train_lat, query_lat)):
        _lat_rows(tr, latent, "train latents")
        _lat_rows(qu, latent, "query latents")
        if tr.shape[0] == 0:
            raise ValueError("knn: a train set has no rows")
        desc[i]["train_lat"] = tr.data_ptr()
        desc[i]["query_lat"] = qu.data_ptr()
        desc[i]["out"] = out.data_ptr() + 8 * off
        desc[i]["n_train"] = tr.shape[0]
        desc[i]["n_query"] = qu.shape[0]
        desc[i]["latent"] = latent
        desc[i]["k"] = k
        desc[i]["train_stride"] = tr.stride(0)
        desc[i]["query_stride"] = qu.stride(0)
        views.append(out[off:off + qu.shape[0]])
        off += qu.shape[0]
    if off > out.shape[0]:
        raise ValueError(f"knn: {off} query rows do not fit the {out.shape[0]} output slots")
    return desc, views


def knn_scores(train_lat: Sequence[torch.Tensor], query_lat: Sequence[torch.Tensor], latent: int, k: int):
    """float64 distance of every query row to the k-th nearest (scaled) train
    row of its item (README "Latent scorers"); one launch for all items."""
    dev = train_lat[0].device
    rt = runtime(dev)
    out_all = torch.empty(sum(int(t.shape[0]) for t in query_lat), dtype=torch.float64, device=dev)
    desc, views = knn_desc(train_lat, query_lat, out_all, latent, k)
    (dptr,) = rt.desc.put(desc)
    _check(lib().fedmx_knn_score(dptr, len(desc), int(k), knn_grid_y(query_lat), rt.stream), "fedmx_knn_score")
    return views


def auc_desc(scores, labels, out_ptr: int, f32_scale: float = 1.0) -> np.ndarray:
    """AucDesc array (fedmx_eval.hip): item i's result goes to float64 slot i
    of ``out_ptr``.  The kernel reads raw pointers, so anything but a
    contiguous float32 / float64 vector with one contiguous int32 label per
    score is refused here."""
    n = len(scores)
    if len(labels) != n:
        raise ValueError(f"auc: {n} score vectors but {len(labels)} label vectors")
    desc = np.zeros(n, dtype=AUC_DTYPE)
    for i, (s, l) in enumerate(zip(scores, labels)):
        f64 = _score_vec(s, "scores", "auc")
        if l.dtype != torch.int32 or l.dim() != 1 or not l.is_contiguous() or l.shape[0] != s.shape[0]:
            raise ValueError("auc: labels must be contiguous int32, one per score")
        desc[i]["score"] = s.data_ptr()
        desc[i]["label"] = l.data_ptr()
        desc[i]["out"] = out_ptr + 8 * i
        desc[i]["n"] = s.shape[0]
        desc[i]["score_is_f64"] = f64
        desc[i]["score_scale"] = f32_scale
    return desc


def auc(scores: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], f32_scale: float = 1.0) -> np.ndarray:
    """Exact tie-aware ROC-AUC per (scores, labels) pair.  Returns a float64
    host view written by the kernel (valid after ``runtime(dev).sync()``);
    -1 marks classes too large for the LDS sort (caller uses the host path)."""
    dev = scores[0].device
    rt = runtime(dev)
    optr, view = rt.out.take(np.float64, len(scores))
    desc = auc_desc(scores, labels, optr, f32_scale)
    (dptr,) = rt.desc.put(desc)
    _check(lib().fedmx_auc(dptr, len(desc), rt.stream), "fedmx_auc")
    return view


def _check_chunk_keys(chunk_keys: int) -> int:
    ck = int(chunk_keys)
    if ck < 64 or ck > AUC_MAX_SORT or ck & (ck - 1):
        raise ValueError(f"auc_large: chunk_keys must be a power of two from 64 to {AUC_MAX_SORT}, got {chunk_keys!r}")
    return ck


def auc_large_grid(sort_rows, probe_rows, chunk_keys: int = AUC_MAX_SORT,
                   resident: int = AUC_LARGE_RESIDENT) -> Tuple[int, int]:
    """(chunks, slices) of one pairs launch (fedmx_auc_large.hip) over
    descriptors whose sort class has ``sort_rows[i]`` rows and whose probe
    class ``probe_rows[i]``: the chunk count of the largest sort class, and
    as many probe slices as fill the chip's resident workgroups once, but no
    more than the largest probe class gives 1024 rows each.  Upper bounds of
    the class sizes do as well: workgroups beyond a descriptor's own chunk
    and slice counts leave at once."""
    ck = _check_chunk_keys(chunk_keys)
    sort_rows = np.atleast_1d(np.asarray(sort_rows, dtype=np.int64))
    probe_rows = np.atleast_1d(np.asarray(probe_rows, dtype=np.int64))
    if sort_rows.shape != probe_rows.shape:
        raise ValueError("auc_large: one sort and one probe size per descriptor")
    live = (sort_rows > 0) & (probe_rows > 0)
    if not live.any():
        return 0, 1
    nch = -(-sort_rows[live] // ck)
    chunks = int(nch.max())
    want = -(-int(resident) // int(nch.sum()))
    cap = -(-int(probe_rows[live].max()) // AUC_LARGE_SLICE_MIN_ROWS)
    return chunks, int(max(1, min(want, cap, 65535)))


def auc_large_cover(sort_rows: int, probe_rows: int, chunk_keys: int, slices: int):
    """The work of every pairs workgroup that stays, as the kernel cuts it for
    one descriptor inside a launch with ``slices`` slices: a list of
    ((first key, end key), (first probe row, end probe row))."""
    ck = _check_chunk_keys(chunk_keys)
    m, npr = int(sort_rows), int(probe_rows)
    if m <= 0 or npr <= 0:
        return []
    nchunks = -(-m // ck)
    nsl = min(max(-(-npr // AUC_LARGE_SLICE_MIN_ROWS), 1), int(slices))
    return [((c * ck, min(m, (c + 1) * ck)), ((npr * s) // nsl, (npr * (s + 1)) // nsl))
            for c in range(nchunks) for s in range(nsl)]


def auc_large_desc(scores, labels, out_ptr: int, ws_ptr: int, ctr_ptr: int, f32_scale: float = 1.0,
                   out_index: Optional[Sequence[int]] = None) -> np.ndarray:
    """AucLargeDesc array (fedmx_auc_large.hip): item i's result goes to
    float64 slot ``out_index[i]`` (default i) of ``out_ptr``; its workspace is
    the next ``n`` doubles of ``ws_ptr`` (sum of all n in total) and its
    counters the i-th 64 bytes of ``ctr_ptr``, zero before the first launch."""
    n = len(scores)
    desc = np.zeros(n, dtype=AUC_LARGE_DTYPE)
    off = 0
    for i, (s, l) in enumerate(zip(scores, labels)):
        if l.dtype != torch.int32 or l.dim() != 1 or not l.is_contiguous() or l.shape[0] != s.shape[0]:
            raise ValueError("auc_large: labels must be contiguous int32, one per score")
        f64 = _score_vec(s, "scores", "auc_large")
        rows = int(s.shape[0])
        if rows > AUC_LARGE_MAX_ROWS:
            raise ValueError(f"auc_large: {rows} rows are beyond the {AUC_LARGE_MAX_ROWS} a pair may have")
        desc[i]["score"] = s.data_ptr()
        desc[i]["label"] = l.data_ptr()
        desc[i]["out"] = out_ptr + 8 * (i if out_index is None else int(out_index[i]))
        desc[i]["ws"] = ws_ptr + 8 * off
        desc[i]["ctr"] = ctr_ptr + 8 * AUC_LARGE_CTR_WORDS * i
        desc[i]["n"] = rows
        desc[i]["score_is_f64"] = f64
        desc[i]["score_scale"] = f32_scale
        off += rows
    return desc


def auc_large(scores: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], f32_scale: float = 1.0,
              chunk_keys: int = AUC_MAX_SORT) -> np.ndarray:
    """Exact tie-aware ROC-AUC per (scores, labels) pair by the
    multi-workgroup path, whatever the class sizes (up to 2^26 rows a pair;
    more raise ValueError).  Returns a float64 host view written by the
    kernels (valid after ``runtime(dev).sync()``); NaN where a class is empty."""
    ck = _check_chunk_keys(chunk_keys)
    dev = scores[0].device
    rt = runtime(dev)
    k = len(scores)
    rows = np.array([int(s.shape[0]) for s in scores], dtype=np.int64)
    # workspace and counters from torch's pool: freed on return, reused in stream order
    ws = torch.empty(max(int(rows.sum()), 1), dtype=torch.float64, device=dev)
    ctr = torch.zeros(AUC_LARGE_CTR_WORDS * k, dtype=torch.int64, device=dev)
    optr, view = rt.out.take(np.float64, k)
    desc = auc_large_desc(scores, labels, optr, ws.data_ptr(), ctr.data_ptr(), f32_scale)
    # the class sizes are known on the device only: the smaller class has at most half the rows
    chunks, slices = auc_large_grid(rows // 2, rows, ck)
    (dptr,) = rt.desc.put(desc)
    _check(lib().fedmx_auc_large(dptr, k, int(rows.max()), chunks, slices, ck, rt.stream), "fedmx_auc_large")
    return view


def launch_auc_large(desc_dev: torch.Tensor, n: int, max_rows: int, chunks: int, slices: int, device,
                     chunk_keys: int = AUC_MAX_SORT):
    _check(lib().fedmx_auc_large(desc_dev.data_ptr(), n, int(max_rows), int(chunks), int(slices),
                                 _check_chunk_keys(chunk_keys), _stream(device)), "fedmx_auc_large")


def _score_vec(t: torch.Tensor, what: str, who: str = "detect") -> int:
    if t.dtype not in (torch.float32, torch.float64) or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be a contiguous float32 or float64 vector")
    return 1 if t.dtype == torch.float64 else 0


def detect_desc(calib, scores, labels, ranks, out_ptr: int, out_stride: int, calib_labels=None,
                f32_scale: float = 1.0, value_is_recall: bool = False) -> np.ndarray:
    """DetectDesc array (fedmx_detect.hip): item i thresholds at the
    ``ranks[i]``-th smallest cleaned value of ``calib[i]`` (of its rows whose
    ``calib_labels[i]`` entry is 0, when given) and writes its 8 results to
    ``out_ptr + 8 * i``, ``out_stride`` doubles apart."""
    n = len(scores)
    if not (len(calib) == len(labels) == len(ranks) == n) or (calib_labels is not None and len(calib_labels) != n):
        raise ValueError("detect: calib, scores, labels, ranks (and calib_labels) must have one entry per item")
    if out_stride < n:
        raise ValueError(f"detect: output stride {out_stride} is below the {n} items")
    desc = np.zeros(n, dtype=DETECT_DTYPE)
    for i, (c, s, l, j) in enumerate(zip(calib, scores, labels, ranks)):
        if l.dtype != torch.int32 or l.shape[0] != s.shape[0] or not l.is_contiguous():
            raise ValueError("detect: labels must be contiguous int32, one per score")
        desc[i]["calib_is_f64"] = _score_vec(c, "calib")
        desc[i]["score_is_f64"] = _score_vec(s, "scores")
        if c.dtype != s.dtype:
            raise ValueError("detect: calib and scores must share a dtype (one score_scale reads both)")
        cl = None if calib_labels is None else calib_labels[i]
        if cl is not None and (cl.dtype != torch.int32 or cl.shape[0] != c.shape[0] or not cl.is_contiguous()):
            raise ValueError("detect: calib_labels must be contiguous int32, one per calibration value")
        if int(j) >= int(c.shape[0]):
            raise ValueError(f"detect: rank {int(j)} is beyond the {int(c.shape[0])} calibration values")
        desc[i]["calib"] = c.data_ptr()
        desc[i]["calib_label"] = 0 if cl is None else cl.data_ptr()
        desc[i]["score"] = s.data_ptr()
        desc[i]["label"] = l.data_ptr()
        desc[i]["out"] = out_ptr + 8 * i
        desc[i]["n_c"] = c.shape[0]
        desc[i]["n"] = s.shape[0]
        desc[i]["j"] = max(int(j), -1)
        desc[i]["score_scale"] = f32_scale
        desc[i]["value_is_recall"] = 1 if value_is_recall else 0
        desc[i]["out_stride"] = out_stride
    return desc


def detect(calib, scores, labels, ranks, calib_labels=None, f32_scale: float = 1.0,
           value_is_recall: bool = False) -> np.ndarray:
    """Threshold + operating-point metrics per item.  Returns a float64 host
    view [8, k] written by the kernel (valid after ``runtime(dev).sync()``)."""
    dev = scores[0].device
    rt = runtime(dev)
    k = len(scores)
    optr, view = rt.out.take(np.float64, 8 * k)
    desc = detect_desc(calib, scores, labels, ranks, optr, k, calib_labels, f32_scale, value_is_recall)
    (dptr,) = rt.desc.put(desc)
    _check(lib().fedmx_detect(dptr, k, rt.stream), "fedmx_detect")
    return view.reshape(8, k)


def launch_detect(desc_dev: torch.Tensor, n: int, device):
    _check(lib().fedmx_detect(desc_dev.data_ptr(), n, _stream(device)), "fedmx_detect")


# ---------------------------------------------------------------------------
# deployed detectors (fedmx_score.hip)
SCORE_RESIDENT = 2 * 256   # score_rows workgroups resident at once (77 KB of LDS each: 2 per CU, 256 CUs)


def score_rows_per_block(total_rows: int) -> int:
    """Rows per score_rows workgroup (a multiple of the 64-row pass): about
    two rounds of residency over the chip, so the grid fills it and the 37 KB
    weight staging of a workgroup is spread over many passes on big inputs."""
    fixed = int(os.environ.get("FEDMX_SCORE_ROWS_PER_BLOCK", "0"))   # A/B override
    if fixed > 0:
        return -(-fixed // SCORE_CHUNK_ROWS) * SCORE_CHUNK_ROWS
    per = -(-int(total_rows) // (2 * SCORE_RESIDENT))
    return max(SCORE_CHUNK_ROWS, -(-per // SCORE_CHUNK_ROWS) * SCORE_CHUNK_ROWS)


class ScoreState:
    """One detector's constants in device memory: the padded parameter
    vector, the feature scaler's two float64 vectors and, for CEN, the latent
    scaler's.  ``kind``: SCORE_KIND_AE, SCORE_KIND_CEN or 0 (latents only)."""

    def __init__(self, params_padded: torch.Tensor, dims, sc_a: np.ndarray, sc_b: np.ndarray, minmax: bool,
                 kind: int, threshold: float, z_mean: Optional[np.ndarray] = None,
                 z_scale: Optional[np.ndarray] = None):
        dev = params_padded.device
        if params_padded.dtype != torch.float32 or params_padded.numel() != 9216 or not params_padded.is_contiguous():
            raise ValueError("score_rows: params must be one contiguous padded float32 vector")
        sc_a = np.ascontiguousarray(sc_a, dtype=np.float64)
        sc_b = np.ascontiguousarray(sc_b, dtype=np.float64)
        if sc_a.shape != (dims.d_in,) or sc_b.shape != (dims.d_in,):
            raise ValueError(f"score_rows: the feature scaler must hold {dims.d_in} values per vector")
        if kind not in (0, SCORE_KIND_AE, SCORE_KIND_CEN):
            raise ValueError(f"score_rows: unknown score kind {kind!r}")
        self.params, self.dims, self.device = params_padded, dims, dev
        self.minmax, self.kind, self.threshold = bool(minmax), int(kind), float(threshold)
        self.scaler = torch.from_numpy(np.stack([sc_a, sc_b])).to(dev)
        self.zscaler = None
        if kind == SCORE_KIND_CEN:
            z_mean = np.ascontiguousarray(z_mean, dtype=np.float64)
            z_scale = np.ascontiguousarray(z_scale, dtype=np.float64)
            if z_mean.shape != (dims.latent,) or z_scale.shape != (dims.latent,):
                raise ValueError(f"score_rows: the latent scaler must hold {dims.latent} values per vector")
            self.zscaler = torch.from_numpy(np.stack([z_mean, z_scale])).to(dev)
        self.band = self.edges = None   # the monitoring baseline (set_baseline)
        self.nedges = -1

    def set_baseline(self, feat_lo: np.ndarray, feat_hi: np.ndarray, score_edges: np.ndarray) -> None:
        """Upload a monitoring baseline: the band (float32 [d_in] each) and the
        score edges (float64, at most MONITOR_MAX_EDGES, non-decreasing)."""
        lo = np.ascontiguousarray(feat_lo, dtype=np.float32)
        hi = np.ascontiguousarray(feat_hi, dtype=np.float32)
        e = np.ascontiguousarray(score_edges, dtype=np.float64)
        if lo.shape != (self.dims.d_in,) or hi.shape != (self.dims.d_in,):
            raise ValueError(f"monitor_rows: the band must hold {self.dims.d_in} values per vector")
        if e.ndim != 1 or e.shape[0] > MONITOR_MAX_EDGES or np.isnan(e).any() or np.any(np.diff(e) < 0):
            raise ValueError(f"monitor_rows: at most {MONITOR_MAX_EDGES} non-decreasing score edges")
        self.band = torch.from_numpy(np.stack([lo, hi])).to(self.device)
        self.edges = torch.from_numpy(np.concatenate([e, np.zeros(1)])).to(self.device)   # (never empty)
        self.nedges = int(e.shape[0])


def score_desc(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], scores, flags, lats, alarms: torch.Tensor,
               rows_per_block: Optional[int] = None) -> np.ndarray:
    """ScoreDesc array (fedmx_score.hip): item i scores the raw rows
    ``rows[i]`` ([n, d_in], float64 or float32, contiguous) with detector
    ``states[i]`` into ``scores[i]`` (float64 [n]) and ``flags[i]`` (uint8 [n];
    both None for a latents-only item), its latents into ``lats[i]`` (float32
    [n, latent] or None), and adds its alarm count to ``alarms[i]`` (int32).
    Every item is cut into blocks of ``rows_per_block`` rows, one workgroup each."""
    n_items = len(states)
    if not (len(rows) == len(scores) == len(flags) == len(lats) == n_items) or alarms.numel() < n_items:
        raise ValueError("score_rows: one rows / scores / flags / latents / alarm slot per detector")
    if alarms.dtype != torch.int32 or not alarms.is_contiguous():
        raise ValueError("score_rows: the alarm counters must be contiguous int32")
    sizes = np.array([int(x.shape[0]) for x in rows], dtype=np.int64)
    rpb = rows_per_block or score_rows_per_block(int(sizes.sum()))
    if rpb % SCORE_CHUNK_ROWS:
        raise ValueError(f"score_rows: rows per block must be a multiple of {SCORE_CHUNK_ROWS}")
    parts = []
    for i, (st, x, sc, fl, la) in enumerate(zip(states, rows, scores, flags, lats)):
        n, dims = int(sizes[i]), st.dims
        if x.dim() != 2 or x.shape[1] != dims.d_in or x.dtype not in (torch.float32, torch.float64) \
                or not x.is_contiguous() or x.device != st.device:
            raise ValueError(f"score_rows: rows must be contiguous float32 / float64 [n, {dims.d_in}] on the "
                             "detector's device")
        if (sc is None) != (fl is None) or (sc is None and la is None) or (sc is None) != (st.kind == 0):
            raise ValueError("score_rows: a scoring item needs scores and flags, a latents-only item neither")
        if sc is not None and (sc.dtype != torch.float64 or sc.numel() != n or not sc.is_contiguous()
                               or fl.dtype != torch.uint8 or fl.numel() != n or not fl.is_contiguous()):
            raise ValueError("score_rows: scores must be float64 [n] and flags uint8 [n], contiguous")
        if la is not None and (la.dtype != torch.float32 or tuple(la.shape) != (n, dims.latent)
                               or not la.is_contiguous()):
            raise ValueError(f"score_rows: latents must be contiguous float32 [n, {dims.latent}]")
        if n == 0:
            continue
        r0 = np.arange(0, n, rpb, dtype=np.int64)
        d = np.zeros(len(r0), dtype=SCORE_DTYPE)
        esz = 8 if x.dtype == torch.float64 else 4
        d["params"] = st.params.data_ptr()
        d["raw"] = x.data_ptr() + esz * dims.d_in * r0
        d["sc_a"] = st.scaler.data_ptr()
        d["sc_b"] = st.scaler.data_ptr() + 8 * dims.d_in
        if st.zscaler is not None:
            d["z_mean"] = st.zscaler.data_ptr()
            d["z_scale"] = st.zscaler.data_ptr() + 8 * dims.latent
        if sc is not None:
            d["score"] = sc.data_ptr() + 8 * r0
            d["flag"] = fl.data_ptr() + r0
        if la is not None:
            d["lat"] = la.data_ptr() + 4 * dims.latent * r0
        d["alarms"] = alarms.data_ptr() + 4 * i
        d["threshold"] = st.threshold
        d["nrows"] = np.minimum(rpb, n - r0)
        d["d_in"], d["hidden"], d["latent"] = dims.d_in, dims.hidden, dims.latent
        d["flags"] = (SCORE_RAW_F64 if esz == 8 else 0) | (SCORE_MINMAX if st.minmax else 0) | st.kind
        d["score_scale"] = np.float32(1.0 / dims.d_in)
        parts.append(d)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=SCORE_DTYPE)


def score_rows(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], want_latents: bool = False,
               rows_per_block: Optional[int] = None):
    """Score raw rows with deployed detectors in one launch.  Returns per item
    (scores float64 [n] or None, flags uint8 [n] or None, latents float32
    [n, latent] or None) on the device and the int32 alarm counters (one per
    item; valid after the stream is synchronised).  A latents-only state
    (kind 0) always returns its latents."""
    dev = states[0].device
    rt = runtime(dev)
    alarms = torch.zeros(len(states), dtype=torch.int32, device=dev)
    scores, flags, lats = [], [], []
    for st, x in zip(states, rows):
        n = int(x.shape[0])
        scoring = st.kind != 0
        scores.append(torch.empty(n, dtype=torch.float64, device=dev) if scoring else None)
        flags.append(torch.empty(n, dtype=torch.uint8, device=dev) if scoring else None)
        lats.append(torch.empty(n, st.dims.latent, dtype=torch.float32, device=dev)
                    if (want_latents or not scoring) else None)
    desc = score_desc(states, rows, scores, flags, lats, alarms, rows_per_block)
    if len(desc):
        (dptr,) = rt.desc.put(desc)
        _check(lib().fedmx_score_rows(dptr, len(desc), rt.stream), "fedmx_score_rows")
    return list(zip(scores, flags, lats)), alarms


def explain_desc(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], which, outs: Sequence[dict], top_k: int,
                 rows_per_block: Optional[int] = None) -> np.ndarray:
    """ExplainDesc array (fedmx_explain.hip): item i explains rows
    ``which[i]`` (int32 [m] on the device, every entry in ``[0, n)``; None:
    all ``m = n`` rows in order) of the raw rows ``rows[i]`` ([n, d_in], float64
    or float32, contiguous) with detector ``states[i]`` into ``outs[i]``:
    ``idx`` int32 [m, top_k], ``resid`` float32 [m, top_k], ``sse`` float32
    [m], ``resid_full`` float32 [m, d_in] or None, ``latent_terms`` float64
    [m, latent] or None (CEN states only).  Every item is cut into blocks of
    ``rows_per_block`` explained rows, one workgroup each."""
    k = check_top_k(top_k)
    if not (len(rows) == len(which) == len(outs) == len(states)):
        raise ValueError("explain_rows: one rows / which / outputs entry per detector")
    sizes = np.array([int(x.shape[0]) if w is None else int(w.numel()) for x, w in zip(rows, which)], dtype=np.int64)
    rpb = rows_per_block or score_rows_per_block(int(sizes.sum()))
    if rpb % SCORE_CHUNK_ROWS:
        raise ValueError(f"explain_rows: rows per block must be a multiple of {SCORE_CHUNK_ROWS}")
    parts = []
    for i, (st, x, w, o) in enumerate(zip(states, rows, which, outs)):
        m, dims = int(sizes[i]), st.dims
        if x.dim() != 2 or x.shape[1] != dims.d_in or x.dtype not in (torch.float32, torch.float64) \
                or not x.is_contiguous() or x.device != st.device:
            raise ValueError(f"explain_rows: rows must be contiguous float32 / float64 [n, {dims.d_in}] on the "
                             "detector's device")
        if dims.d_in > 127:   # column 127 carries the forward's bias input, not a residual (fedmx_explain.hip)
            raise ValueError(f"explain_rows: d_in {dims.d_in} reaches the padded layout's bias column")
        if w is not None and (w.dtype != torch.int32 or w.dim() != 1 or not w.is_contiguous()
                              or w.device != st.device):
            raise ValueError("explain_rows: which must be a contiguous int32 vector on the detector's device")
        want = {"idx": (torch.int32, (m, k)), "resid": (torch.float32, (m, k)), "sse": (torch.float32, (m,)),
                "resid_full": (torch.float32, (m, dims.d_in)), "latent_terms": (torch.float64, (m, dims.latent))}
        for name, (dt, shape) in want.items():
            t = o.get(name)
            if t is None and name in ("resid_full", "latent_terms"):
                continue
            if t is None or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != st.device:
                raise ValueError(f"explain_rows: {name} must be contiguous {dt} {list(shape)} on the detector's device")
        if o.get("latent_terms") is not None and st.zscaler is None:
            raise ValueError("explain_rows: latent terms need a CEN detector's latent scaler")
        if m == 0:
            continue
        r0 = np.arange(0, m, rpb, dtype=np.int64)
        d = np.zeros(len(r0), dtype=EXPLAIN_DTYPE)
        esz = 8 if x.dtype == torch.float64 else 4
        d["params"] = st.params.data_ptr()
        if w is None:
            d["raw"] = x.data_ptr() + esz * dims.d_in * r0
        else:
            d["raw"] = x.data_ptr()
            d["which"] = w.data_ptr() + 4 * r0
        d["sc_a"] = st.scaler.data_ptr()
        d["sc_b"] = st.scaler.data_ptr() + 8 * dims.d_in
        d["idx"] = o["idx"].data_ptr() + 4 * k * r0
        d["resid"] = o["resid"].data_ptr() + 4 * k * r0
        d["sse"] = o["sse"].data_ptr() + 4 * r0
        if o.get("resid_full") is not None:
            d["resid_full"] = o["resid_full"].data_ptr() + 4 * dims.d_in * r0
        if o.get("latent_terms") is not None:
            d["z_mean"] = st.zscaler.data_ptr()
            d["z_scale"] = st.zscaler.data_ptr() + 8 * dims.latent
            d["latent_terms"] = o["latent_terms"].data_ptr() + 8 * dims.latent * r0
        d["nrows"] = np.minimum(rpb, m - r0)
        d["d_in"], d["hidden"], d["latent"] = dims.d_in, dims.hidden, dims.latent
        d["flags"] = (SCORE_RAW_F64 if esz == 8 else 0) | (SCORE_MINMAX if st.minmax else 0)
        d["top_k"] = k
        parts.append(d)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=EXPLAIN_DTYPE)


def explain_rows(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], top_k: int, which=None,
                 dense: bool = False, rows_per_block: Optional[int] = None) -> List[dict]:
    """Explain raw rows with deployed detectors in one ``explain_rows_kernel``
    launch (README "Explaining an alarm").  ``which[i]``: the indices into
    ``rows[i]`` to explain (a host integer array, any order, repeats allowed;
    checked here to lie in ``[0, n)``), or None for every row.  Returns per
    item a dict of device tensors, valid after the stream is synchronised:
    ``idx`` int32 [m, top_k], ``resid`` float32 [m, top_k], ``sse`` float32
    [m], ``resid_full`` float32 [m, d_in] (``dense``, else None),
    ``latent_terms`` float64 [m, latent] (CEN states, else None), ``rows``
    (the checked indices, host int64 [m]; None for every row) and ``which`` (the uploaded
    indices or None; kept alive until then).  An item with nothing to
    explain gets empty tensors and no workgroup."""
    dev = states[0].device
    rt = runtime(dev)
    k = check_top_k(top_k)
    which = list(which) if which is not None else [None] * len(states)
    if len(which) != len(states) or len(rows) != len(states):
        raise ValueError("explain_rows: one rows / which entry per detector")
    wdev, outs, picked = [], [], []
    for st, x, w in zip(states, rows, which):
        n = int(x.shape[0])
        picked.append(None if w is None else check_which(w, n))
        if w is not None:
            if n > np.iinfo(np.int32).max:
                raise ValueError("explain_rows: which indexes at most 2^31 - 1 rows")
            w = torch.from_numpy(picked[-1].astype(np.int32)).to(dev)
        m = n if w is None else int(picked[-1].shape[0])
        wdev.append(w)
        outs.append({
            "idx": torch.empty(m, k, dtype=torch.int32, device=dev),
            "resid": torch.empty(m, k, dtype=torch.float32, device=dev),
            "sse": torch.empty(m, dtype=torch.float32, device=dev),
            "resid_full": torch.empty(m, st.dims.d_in, dtype=torch.float32, device=dev) if dense else None,
            "latent_terms": (torch.empty(m, st.dims.latent, dtype=torch.float64, device=dev)
                             if st.kind == SCORE_KIND_CEN else None),
        })
    desc = explain_desc(states, rows, wdev, outs, k, rows_per_block)
    if len(desc):
        (dptr,) = rt.desc.put(desc)
        _check(lib().fedmx_explain_rows(dptr, len(desc), rt.stream), "fedmx_explain_rows")
    for o, w, p in zip(outs, wdev, picked):
        o["which"], o["rows"] = w, p
    return outs


def monitor_desc(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], lats, alarms: torch.Tensor,
                 hist: torch.Tensor, part: torch.Tensor, total: torch.Tensor, rows_per_block: Optional[int] = None):
    """MonitorDesc and MonitorFoldDesc arrays (fedmx_monitor.hip): item i folds
    the raw rows ``rows[i]`` ([n, d_in], float64 or float32, contiguous) under
    detector ``states[i]`` into ``total[i]`` (MONITOR_TOTAL_DTYPE, uint8 view),
    through one block partial each in ``part`` (MONITOR_PARTIAL_DTYPE, one per
    descriptor in descriptor order); adds its alarm count to ``alarms[i]``
    (int32) and, for a state with a baseline, its score histogram to
    ``hist[16 * i:]`` (int64); a latents-only state (kind 0) writes its latents
    to ``lats[i]`` (float32 [n, latent]) and counts neither.  Every item is cut
    into blocks of ``rows_per_block`` rows, one workgroup each; an item without
    rows gets no descriptor of either kind."""
    n_items = len(states)
    if not (len(rows) == len(lats) == n_items) or alarms.numel() < n_items or hist.numel() < 16 * n_items:
        raise ValueError("monitor_rows: one rows / latents / alarm slot / 16 histogram slots per detector")
    if alarms.dtype != torch.int32 or not alarms.is_contiguous() or hist.dtype != torch.int64 \
            or not hist.is_contiguous():
        raise ValueError("monitor_rows: the alarm counters must be contiguous int32, the histograms int64")
    sizes = np.array([int(x.shape[0]) for x in rows], dtype=np.int64)
    rpb = rows_per_block or score_rows_per_block(int(sizes.sum()))
    if rpb % SCORE_CHUNK_ROWS:
        raise ValueError(f"monitor_rows: rows per block must be a multiple of {SCORE_CHUNK_ROWS}")
    nblocks = int(sum(-(-int(n) // rpb) for n in sizes))
    if part.dtype != torch.uint8 or part.numel() < nblocks * MONITOR_PARTIAL_DTYPE.itemsize \
            or not part.is_contiguous() or total.dtype != torch.uint8 \
            or total.numel() < n_items * MONITOR_TOTAL_DTYPE.itemsize or not total.is_contiguous():
        raise ValueError("monitor_rows: the workspace holds one partial per block and one total per detector")
    parts, folds, b0 = [], [], 0
    for i, (st, x, la) in enumerate(zip(states, rows, lats)):
        n, dims = int(sizes[i]), st.dims
        if x.dim() != 2 or x.shape[1] != dims.d_in or x.dtype not in (torch.float32, torch.float64) \
                or not x.is_contiguous() or x.device != st.device:
            raise ValueError(f"monitor_rows: rows must be contiguous float32 / float64 [n, {dims.d_in}] on the "
                             "detector's device")
        if (la is not None) != (st.kind == 0):
            raise ValueError("monitor_rows: a latents-only item needs latents, a scoring item none")
        if la is not None and (la.dtype != torch.float32 or tuple(la.shape) != (n, dims.latent)
                               or not la.is_contiguous() or la.device != st.device):
            raise ValueError(f"monitor_rows: latents must be contiguous float32 [n, {dims.latent}]")
        if n == 0:
            continue
        r0 = np.arange(0, n, rpb, dtype=np.int64)
        d = np.zeros(len(r0), dtype=MONITOR_DTYPE)
        esz = 8 if x.dtype == torch.float64 else 4
        d["params"] = st.params.data_ptr()
        d["raw"] = x.data_ptr() + esz * dims.d_in * r0
        d["sc_a"] = st.scaler.data_ptr()
        d["sc_b"] = st.scaler.data_ptr() + 8 * dims.d_in
        if st.zscaler is not None:
            d["z_mean"] = st.zscaler.data_ptr()
            d["z_scale"] = st.zscaler.data_ptr() + 8 * dims.latent
        if st.band is not None:
            d["lo"] = st.band.data_ptr()
            d["hi"] = st.band.data_ptr() + 4 * dims.d_in
            d["edges"] = st.edges.data_ptr()
            d["nedges"] = st.nedges
            if st.kind != 0:
                d["hist"] = hist.data_ptr() + 8 * 16 * i
        if la is not None:
            d["lat"] = la.data_ptr() + 4 * dims.latent * r0
        d["alarms"] = alarms.data_ptr() + 4 * i
        d["part"] = part.data_ptr() + MONITOR_PARTIAL_DTYPE.itemsize * (b0 + np.arange(len(r0), dtype=np.int64))
        d["threshold"] = st.threshold
        d["nrows"] = np.minimum(rpb, n - r0)
        d["d_in"], d["hidden"], d["latent"] = dims.d_in, dims.hidden, dims.latent
        d["flags"] = (SCORE_RAW_F64 if esz == 8 else 0) | (SCORE_MINMAX if st.minmax else 0) | st.kind
        d["score_scale"] = np.float32(1.0 / dims.d_in)
        parts.append(d)
        f = np.zeros(1, dtype=MONITOR_FOLD_DTYPE)
        f["part"] = part.data_ptr() + MONITOR_PARTIAL_DTYPE.itemsize * b0
        f["total"] = total.data_ptr() + MONITOR_TOTAL_DTYPE.itemsize * i
        f["nblocks"] = len(r0)
        folds.append(f)
        b0 += len(r0)
    if not parts:
        return np.zeros(0, dtype=MONITOR_DTYPE), np.zeros(0, dtype=MONITOR_FOLD_DTYPE)
    return np.concatenate(parts), np.concatenate(folds)


def monitor_rows(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], rows_per_block: Optional[int] = None):
    """Monitor raw rows with deployed detectors (README "Monitoring a
    deployed detector"): one ``monitor_rows_kernel`` launch over all items and
    one ``monitor_fold_kernel`` launch behind it.  Returns, valid after the
    stream is synchronised: ``total`` (uint8 device tensor; view it as
    MONITOR_TOTAL_DTYPE, one record per item; an item without rows keeps
    zeros), the int32 alarm counters, the int64 histograms ``[items, 16]``, the
    per-item latents (latents-only states, else None), the rows per block
    used and the block-partial workspace (keep it until then).  Nothing
    launches when no item has rows."""
    dev = states[0].device
    rt = runtime(dev)
    n_items = len(states)
    sizes = [int(x.shape[0]) for x in rows]
    rpb = rows_per_block or score_rows_per_block(sum(sizes))
    if rpb % SCORE_CHUNK_ROWS:
        raise ValueError(f"monitor_rows: rows per block must be a multiple of {SCORE_CHUNK_ROWS}")
    nblocks = sum(-(-n // rpb) for n in sizes)
    alarms = torch.zeros(n_items, dtype=torch.int32, device=dev)
    hist = torch.zeros(n_items, 16, dtype=torch.int64, device=dev)
    part = torch.empty(max(nblocks, 1) * MONITOR_PARTIAL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    total = torch.zeros(n_items * MONITOR_TOTAL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    lats = [torch.empty(n, st.dims.latent, dtype=torch.float32, device=dev) if st.kind == 0 else None
            for st, n in zip(states, sizes)]
    desc, fold = monitor_desc(states, rows, lats, alarms, hist, part, total, rpb)
    if len(desc):
        dptr, fptr = rt.desc.put(desc, fold)
        _check(lib().fedmx_monitor_rows(dptr, len(desc), fptr, len(fold), rt.stream), "fedmx_monitor_rows")
    return total, alarms, hist, lats, rpb, part


# ---------------------------------------------------------------------------
# incidents (fedmx_incident.hip)
def incident_span_rows() -> int:
    """Rows one incident workgroup owns (its halo comes on top)."""
    return int(lib().fedmx_incident_span_rows())


def incident_desc(flags: Sequence[torch.Tensor], scores: Sequence[torch.Tensor], window: int, min_alarms: int,
                  hold: int, outs: Sequence[dict]):
    """IncidentItem and IncidentSpanDesc arrays (fedmx_incident.hip): item i
    groups ``flags[i]`` (uint8 [n], contiguous) with ``scores[i]`` (float64 [n])
    into ``outs[i]``: ``out`` int64 [4, kmax] (start, end, and the two prefix
    values; row 3 holds alarms after the finish pass), ``peak`` int64 [2, kmax]
    zeroed (keys and coded rows; peak_score's bits and peak_row after it),
    ``summary`` int64 [4] zeroed, ``ws`` int32 [2, nspans, 4], with ``kmax =
    incident_bound(n, hold)``.  An item without rows gets no descriptor."""
    w, m, h = check_incident_params(window, min_alarms, hold)
    if not (len(flags) == len(scores) == len(outs)):
        raise ValueError("incidents: one flags / scores / outputs entry per item")
    S = incident_span_rows()
    items, spans = [], []
    for f, s, o in zip(flags, scores, outs):
        n = check_incident_rows(f.shape, s.shape)
        if f.dtype != torch.uint8 or s.dtype != torch.float64 or not f.is_contiguous() or not s.is_contiguous() \
                or f.device != s.device:
            raise ValueError("incidents: flags must be contiguous uint8 [n] and scores float64 [n] on one device")
        if n == 0:
            continue
        kmax, nsp = incident_bound(n, h), -(-n // S)
        out, peak, summary, ws = o["out"], o["peak"], o["summary"], o["ws"]
        if out.dtype != torch.int64 or tuple(out.shape) != (4, kmax) or not out.is_contiguous() \
                or peak.dtype != torch.int64 or tuple(peak.shape) != (2, kmax) or not peak.is_contiguous() \
                or summary.dtype != torch.int64 or summary.numel() != 4 or not summary.is_contiguous() \
                or ws.dtype != torch.int32 or tuple(ws.shape) != (2, nsp, 4) or not ws.is_contiguous() \
                or ws.data_ptr() % 16 or any(t.device != f.device for t in (out, peak, summary, ws)):
            raise ValueError(f"incidents: outputs must be int64 [4, {kmax}], [2, {kmax}] and [4] and a 16-byte "
                             f"aligned int32 [2, {nsp}, 4] workspace on the flags' device")
        d = np.zeros(1, dtype=INCIDENT_ITEM_DTYPE)
        d["flags"], d["scores"] = f.data_ptr(), s.data_ptr()
        d["totals"], d["offs"] = ws.data_ptr(), ws.data_ptr() + 16 * nsp
        for j, name in enumerate(("start", "end", "pa", "pb")):
            d[name] = out.data_ptr() + 8 * kmax * j
        d["key"], d["enc"] = peak.data_ptr(), peak.data_ptr() + 8 * kmax
        d["summary"] = summary.data_ptr()
        d["n"], d["nspans"], d["window"], d["min_alarms"], d["hold"], d["kmax"] = n, nsp, w, m, h, kmax
        sp = np.zeros(nsp, dtype=INCIDENT_SPAN_DTYPE)
        sp["item"], sp["span"] = len(items), np.arange(nsp, dtype=np.int32)
        items.append(d)
        spans.append(sp)
    if not items:
        return np.zeros(0, dtype=INCIDENT_ITEM_DTYPE), np.zeros(0, dtype=INCIDENT_SPAN_DTYPE)
    if len(items) > INCIDENT_MAX_ITEMS:
        raise ValueError(f"incidents: at most {INCIDENT_MAX_ITEMS} items with rows per call")
    return np.concatenate(items), np.concatenate(spans)


def incidents(flags: Sequence[torch.Tensor], scores: Sequence[torch.Tensor], window: int, min_alarms: int,
              hold: int = 0, phases: int = 31) -> List[Optional[dict]]:
    """Group alarms into incidents (README "Incidents"): the mark, scan, emit,
    peak and finish launches of fedmx_incident.hip over all items, on the
    runtime's stream behind whatever produced ``flags`` and ``scores`` there.
    Returns per item the ``incident_desc`` output tensors (None for an item
    without rows), valid after the stream is synchronised: ``summary`` = (hot
    rows, count, rows covered, longest); of ``out`` rows 0, 1, 3 and of
    ``peak`` row 1 (peak_row) and row 0 (peak_score's bits) the first ``count``
    entries.  Nothing launches when no item has rows."""
    w, m, h = check_incident_params(window, min_alarms, hold)
    S = incident_span_rows()
    outs = []
    for f, s in zip(flags, scores):
        n = check_incident_rows(f.shape, s.shape)
        if n == 0:
            outs.append(None)
            continue
        dev, kmax = f.device, incident_bound(n, h)
        outs.append({"out": torch.empty(4, kmax, dtype=torch.int64, device=dev),
                     "peak": torch.zeros(2, kmax, dtype=torch.int64, device=dev),
                     "summary": torch.zeros(4, dtype=torch.int64, device=dev),
                     "ws": torch.empty(2, -(-n // S), 4, dtype=torch.int32, device=dev)})
    live = [i for i, o in enumerate(outs) if o is not None]
    if not live:
        return outs
    items, spans = incident_desc([flags[i] for i in live], [scores[i] for i in live], w, m, h,
                                 [outs[i] for i in live])
    rt = runtime(flags[live[0]].device)
    iptr, sptr = rt.desc.put(items, spans)
    _check(lib().fedmx_incidents(iptr, len(items), sptr, len(spans), int(items["kmax"].max()), int(phases),
                                 rt.stream), "fedmx_incidents")
    return outs


# ---------------------------------------------------------------------------
# incident signatures (fedmx_signature.hip)
def signature_desc(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], which, seg, offsets, part: torch.Tensor,
                   outs: Sequence[dict], rows_per_block: int):
    """SigDesc and SigFoldDesc arrays (fedmx_signature.hip): item i reduces the
    residuals of the list ``which[i]`` (int32 [m] on the device: row indices
    into ``rows[i]``, every entry in ``[0, n)``) per incident, ``seg[i]`` (int32
    [m] on the device, non-decreasing, in ``[0, s)``) naming each position's;
    ``offsets[i]`` (host int64 [s + 1]) are the incidents' first list positions
    and ``m``.  ``outs[i]``: ``err_sum`` / ``resid_sum`` float64 [s, d_in] and
    ``bad`` int64 [s, d_in].  ``part`` (uint8) holds ``blocks + s`` zeroed
    SIG_PARTIAL_DTYPE slots per item with list positions, in item order.  Every
    list is cut into blocks of ``rows_per_block`` positions, one workgroup
    each; an item with ``m = 0`` gets no descriptor of either kind."""
    if not (len(rows) == len(which) == len(seg) == len(offsets) == len(outs) == len(states)):
        raise ValueError("incident_signatures: one rows / list / offsets / outputs entry per detector")
    rpb = int(rows_per_block)
    if rpb < 1 or rpb % SCORE_CHUNK_ROWS:
        raise ValueError(f"incident_signatures: rows per block must be a positive multiple of {SCORE_CHUNK_ROWS}")
    psz = SIG_PARTIAL_DTYPE.itemsize
    parts, folds, slot0 = [], [], 0
    for st, x, w, sg, off, o in zip(states, rows, which, seg, offsets, outs):
        dims = st.dims
        off = np.asarray(off, dtype=np.int64)
        s, m = int(off.shape[0]) - 1, int(off[-1])
        if x.dim() != 2 or x.shape[1] != dims.d_in or x.dtype not in (torch.float32, torch.float64) \
                or not x.is_contiguous() or x.device != st.device:
            raise ValueError(f"incident_signatures: rows must be contiguous float32 / float64 [n, {dims.d_in}] on "
                             "the detector's device")
        if dims.d_in > 127:   # column 127 carries the forward's bias input, not a residual (fedmx_explain.hip)
            raise ValueError(f"incident_signatures: d_in {dims.d_in} reaches the padded layout's bias column")
        if int(x.shape[0]) > np.iinfo(np.int32).max:
            raise ValueError("incident_signatures: the list indexes at most 2^31 - 1 rows")
        for t, name in ((w, "the list"), (sg, "its incidents")):
            if t.dtype != torch.int32 or tuple(t.shape) != (m,) or not t.is_contiguous() or t.device != st.device:
                raise ValueError(f"incident_signatures: {name} must be contiguous int32 [{m}] on the detector's device")
        if s < 0 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError("incident_signatures: the incidents' list offsets must start at 0 and not fall")
        for name, dt in (("err_sum", torch.float64), ("resid_sum", torch.float64), ("bad", torch.int64)):
            t = o.get(name)
            if t is None or t.dtype != dt or tuple(t.shape) != (s, dims.d_in) or not t.is_contiguous() \
                    or t.device != st.device:
                raise ValueError(f"incident_signatures: {name} must be contiguous {dt} [{s}, {dims.d_in}] on the "
                                 "detector's device")
        if m == 0:
            continue
        r0 = np.arange(0, m, rpb, dtype=np.int64)
        nslots = len(r0) + s
        if part.dtype != torch.uint8 or not part.is_contiguous() or part.numel() < (slot0 + nslots) * psz:
            raise ValueError("incident_signatures: the workspace holds blocks + incidents partial slots per item")
        base = part.data_ptr() + psz * slot0
        d = np.zeros(len(r0), dtype=SIG_DTYPE)
        esz = 8 if x.dtype == torch.float64 else 4
        d["params"] = st.params.data_ptr()
        d["raw"] = x.data_ptr()
        d["sc_a"] = st.scaler.data_ptr()
        d["sc_b"] = st.scaler.data_ptr() + 8 * dims.d_in
        d["which"] = w.data_ptr() + 4 * r0
        d["seg"] = sg.data_ptr() + 4 * r0
        d["part"] = base
        d["nrows"] = np.minimum(rpb, m - r0)
        d["d_in"], d["hidden"], d["latent"] = dims.d_in, dims.hidden, dims.latent
        d["flags"] = (SCORE_RAW_F64 if esz == 8 else 0) | (SCORE_MINMAX if st.minmax else 0)
        d["block"] = np.arange(len(r0))
        d["nslots"] = nslots
        parts.append(d)
        j = np.arange(s, dtype=np.int64)
        f = np.zeros(s, dtype=SIG_FOLD_DTYPE)
        f["part"] = base
        for name in ("err_sum", "resid_sum", "bad"):
            f[name] = o[name].data_ptr() + 8 * dims.d_in * j
        f["seg"] = j
        f["first"] = off[:-1] // rpb
        f["last"] = np.where(off[1:] > off[:-1], (off[1:] - 1) // rpb, off[:-1] // rpb - 1)   # (none: last < first)
        f["d_in"] = dims.d_in
        folds.append(f)
        slot0 += nslots
    if not parts:
        return np.zeros(0, dtype=SIG_DTYPE), np.zeros(0, dtype=SIG_FOLD_DTYPE)
    return np.concatenate(parts), np.concatenate(folds)


def incident_signatures(states: Sequence[ScoreState], rows: Sequence[torch.Tensor], lists, segs, offsets,
                        rows_per_block: int) -> List[dict]:
    """Per-incident residual sums of deployed detectors (README "Incident
    signatures"): one ``incident_sig_kernel`` launch over all items' lists and
    one ``incident_sig_fold_kernel`` launch behind it.  ``lists[i]`` / ``segs[i]``:
    host integer arrays [m] (``deploy.detector.signature_list``); ``offsets[i]``:
    host int64 [s + 1].  Returns per item a dict of device tensors, valid after
    the stream is synchronised: ``err_sum`` / ``resid_sum`` float64 [s, d_in],
    ``bad`` int64 [s, d_in] (zeros for an incident or an item without list
    positions), and what must stay alive until then.  Nothing launches when no
    item has a list position."""
    dev = states[0].device
    rt = runtime(dev)
    wdev, sdev, outs, nslots = [], [], [], 0
    for st, x, w, sg, off in zip(states, rows, lists, segs, offsets):
        w = np.asarray(w, dtype=np.int64)
        n, m, s = int(x.shape[0]), int(w.shape[0]), int(len(off)) - 1
        sg = np.asarray(sg, dtype=np.int32)
        if sg.shape != (m,) or (m and (int(w.min()) < 0 or int(w.max()) >= n or int(sg.min()) < 0
                                       or int(sg.max()) >= s or np.any(np.diff(sg) < 0))):
            raise ValueError(f"incident_signatures: the list must index [0, {n}) and its incidents rise within "
                             f"[0, {s})")
        wdev.append(torch.from_numpy(w.astype(np.int32)).to(dev))
        sdev.append(torch.from_numpy(np.ascontiguousarray(sg)).to(dev))
        outs.append({"err_sum": torch.zeros(s, st.dims.d_in, dtype=torch.float64, device=dev),
                     "resid_sum": torch.zeros(s, st.dims.d_in, dtype=torch.float64, device=dev),
                     "bad": torch.zeros(s, st.dims.d_in, dtype=torch.int64, device=dev)})
        if m:
            nslots += -(-m // int(rows_per_block)) + s
    part = torch.zeros(max(nslots, 1) * SIG_PARTIAL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    desc, fold = signature_desc(states, rows, wdev, sdev, offsets, part, outs, rows_per_block)
    if len(desc) and len(fold):
        dptr, fptr = rt.desc.put(desc, fold)
        _check(lib().fedmx_incident_signatures(dptr, len(desc), fptr, len(fold), rt.stream),
               "fedmx_incident_signatures")
    for o, w, sg in zip(outs, wdev, sdev):
        o["keep"] = (w, sg, part)
    return outs


def launch_score_rows(desc_dev: torch.Tensor, n: int, device):
    _check(lib().fedmx_score_rows(desc_dev.data_ptr(), n, _stream(device)), "fedmx_score_rows")


def launch_cen(desc_dev: torch.Tensor, n: int, device):
    _check(lib().fedmx_cen_score(desc_dev.data_ptr(), n, _stream(device)), "fedmx_cen_score")


def launch_knn(desc_dev: torch.Tensor, n: int, device, k: int = KNN_MAX_K, y: int = 8):
    """``k``: the launch's neighbour-list capacity, at least every
    descriptor's k (the default holds any); ``y``: workgroups per descriptor."""
    _check(lib().fedmx_knn_score(desc_dev.data_ptr(), n, int(k), int(y), _stream(device)), "fedmx_knn_score")


def launch_auc(desc_dev: torch.Tensor, n: int, device):
    _check(lib().fedmx_auc(desc_dev.data_ptr(), n, _stream(device)), "fedmx_auc")


def score_reduce(sse_list: Sequence[torch.Tensor], batch: Sequence[int], d_in: int) -> np.ndarray:
    """Host view [len, 2] float64: (mean over batches of batch-MSE, overall MSE)
    per SSE segment; valid after the next stream sync."""
    dev = sse_list[0].device
    rt = runtime(dev)
    optr, view = rt.out.take(np.float64, 2 * len(sse_list))
    desc = np.zeros(len(sse_list), dtype=SEG_DTYPE)
    desc["sse"] = [s.data_ptr() for s in sse_list]
    desc["n"] = [int(s.shape[0]) for s in sse_list]
    desc["batch"] = list(batch)
    desc["out"] = optr + 16 * np.arange(len(sse_list), dtype=np.int64)
    (dptr,) = rt.desc.put(desc)
    _check(lib().fedmx_score_reduce(dptr, len(desc), d_in, rt.stream), "fedmx_score_reduce")
    return view.reshape(len(sse_list), 2)


COPY_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("nfloats", "<i4"), ("pad", "<i4")])


def score_reduce_to(sse_list: Sequence[torch.Tensor], batch: Sequence[int], d_in: int, out_ptrs: Sequence[int],
                    copies: Sequence[Tuple[int, int, int]] = ()):
    """score_reduce writing each segment's (vote score, MSE) pair to the given
    device addresses (16 bytes each) instead of the result ring.  ``copies``
    (src, dst, nfloats): row copies that run in the same launch, beside the
    reductions (the multi-rank exchange's pack)."""
    dev = sse_list[0].device
    rt = runtime(dev)
    desc = np.zeros(len(sse_list), dtype=SEG_DTYPE)
    desc["sse"] = [s.data_ptr() for s in sse_list]
    desc["n"] = [int(s.shape[0]) for s in sse_list]
    desc["batch"] = list(batch)
    desc["out"] = np.asarray(out_ptrs, dtype=np.int64)
    if not copies:
        (dptr,) = rt.desc.put(desc)
        _check(lib().fedmx_score_reduce(dptr, len(desc), d_in, rt.stream), "fedmx_score_reduce")
        return
    cd = np.zeros(len(copies), dtype=COPY_DTYPE)
    cd["src"] = [c[0] for c in copies]
    cd["dst"] = [c[1] for c in copies]
    cd["nfloats"] = [c[2] for c in copies]
    if bool(np.any(cd["nfloats"] % 4)):
        raise ValueError("score_reduce_to: copies must move whole float4 words")
    dptr, cptr = rt.desc.put(desc, cd)
    _check(lib().fedmx_score_reduce_copy(dptr, len(desc), d_in, cptr, len(cd), rt.stream), "fedmx_score_reduce_copy")


def seg_desc_device(sse_list: Sequence[torch.Tensor], batch: Sequence[int], out_ptrs: Sequence[int], dev) -> torch.Tensor:
    """A persistent score_reduce descriptor array in device memory (cached launch plans)."""
    desc = np.zeros(len(sse_list), dtype=SEG_DTYPE)
    desc["sse"] = [s.data_ptr() for s in sse_list]
    desc["n"] = [int(s.shape[0]) for s in sse_list]
    desc["batch"] = list(batch)
    desc["out"] = np.asarray(out_ptrs, dtype=np.int64)
    return torch.from_numpy(desc.view(np.uint8).copy()).to(dev)


def launch_score_reduce(desc_dev: torch.Tensor, n: int, d_in: int, device):
    _check(lib().fedmx_score_reduce(desc_dev.data_ptr(), n, d_in, _stream(device)), "fedmx_score_reduce")


def elect_wsum(eargs: ElectArgs, wargs: WsumArgs, device):
    _check(lib().fedmx_elect_wsum(ctypes.byref(eargs), ctypes.byref(wargs), _stream(device)), "fedmx_elect_wsum")


def decide_adopt(args: DecideArgs, device):
    _check(lib().fedmx_decide_adopt(ctypes.byref(args), _stream(device)), "fedmx_decide_adopt")


def verify_decide(args: VerifyArgs, device):
    """Verification forward + decide_adopt + evaluation snapshot, one launch."""
    _check(lib().fedmx_verify_decide(ctypes.byref(args), _stream(device)), "fedmx_verify_decide")


def verify_split(args: VerifyArgs, sargs: VerifySplitArgs, device):
    """verify_decide's decisions, adoption and snapshots with each receiver's
    forward spread over ``sargs.splits`` workgroups and its drift over one
    more (modes 0 / 1 / 3; the thesis rule keeps verify_decide)."""
    _check(lib().fedmx_verify_split(ctypes.byref(args), ctypes.byref(sargs), _stream(device)), "fedmx_verify_split")


def side_wait(word_ptr: int, seq: int, status_ptr: int, timeout_ticks: int, stream: int):
    """Enqueue on ``stream`` a one-lane wait until the 32-bit word at
    ``word_ptr`` reaches ``seq`` (verify_split_kernel's hand-off word);
    past ``timeout_ticks`` (wall_clock64 ticks) it sets the int32 at
    ``status_ptr`` (host-visible) and lets the stream go on."""
    _check(lib().fedmx_side_wait(ctypes.c_void_p(word_ptr), ctypes.c_uint32(seq & 0xFFFFFFFF),
                                 ctypes.c_void_p(status_ptr), ctypes.c_longlong(timeout_ticks),
                                 ctypes.c_void_p(stream)), "fedmx_side_wait")


def copy_f64(dst_ptr: int, src_ptr: int, n: int, device):
    _check(lib().fedmx_copy_f64(dst_ptr, src_ptr, n, _stream(device)), "fedmx_copy_f64")


def copy2_f64(d0: int, s0: int, n0: int, d1: int, s1: int, n1: int, device):
    _check(lib().fedmx_copy2_f64(d0, s0, n0, d1, s1, n1, _stream(device)), "fedmx_copy2_f64")


def copy_rows(dst_ptr: int, dstride: int, didx_ptr: int, src_ptr: int, sstride: int, sidx_ptr: int, n: int,
              length: int, device):
    """dst[didx[i]] = src[sidx[i]] for n rows of ``length`` floats (index
    pointers may be 0 = identity; strides in floats)."""
    _check(lib().fedmx_copy_rows(dst_ptr, dstride, didx_ptr, src_ptr, sstride, sidx_ptr, n, length,
                                 _stream(device)), "fedmx_copy_rows")


def broadcast_rows(dst0: torch.Tensor, dst1: Optional[torch.Tensor], rows: Sequence[int], src: torch.Tensor):
    if not len(rows):
        return
    rt = runtime(dst0.device)
    (iptr,) = rt.desc.put(np.asarray(rows, dtype=np.int32))
    _check(lib().fedmx_broadcast_rows(dst0.data_ptr(), 0 if dst1 is None else dst1.data_ptr(), iptr, len(rows),
                                      src.data_ptr(), dst0.shape[1], rt.stream), "fedmx_broadcast_rows")


def weighted_sum(stack: torch.Tensor, weights: Sequence[float], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dev = stack.device
    rt = runtime(dev)
    K, P = stack.shape
    (wptr,) = rt.desc.put(np.asarray(weights, dtype=np.float32))
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=dev)
    st = stack.contiguous()
    _check(lib().fedmx_weighted_sum(st.data_ptr(), wptr, K, P, out.data_ptr(), rt.stream), "fedmx_weighted_sum")
    return out


def robust_aggregate(base: torch.Tensor, rows_ptr: Optional[int], k: int, t: int, out: torch.Tensor,
                     state_ptr: int = 0) -> torch.Tensor:
    """``out[i]`` = trimmed mean (``t`` models trimmed at each end of the
    per-coordinate order, ties by position; ``t = (k - 1) // 2``: the median)
    of ``base[rows[j], i]``, j < k, summed in row-table order
    (fedmx_robust.hip).  ``rows_ptr``: device-visible ``int64[k]`` (e.g. in the
    mapped descriptor ring), or None for rows 0..k-1.  With ``state_ptr`` the
    launch writes nothing when the int32 there is negative (no aggregator
    elected).  Raises ValueError for k or t out of range; nothing is launched."""
    if base.dim() != 2 or base.dtype != torch.float32 or not base.is_contiguous():
        raise ValueError("robust_aggregate: base must be a contiguous float32 [rows, P] tensor")
    P = int(base.shape[1])
    if not 1 <= k <= ROBUST_MAX_K:
        raise ValueError(f"robust_aggregate: k = {k} models (1..{ROBUST_MAX_K} supported)")
    if t < 0 or 2 * t >= k:
        raise ValueError(f"robust_aggregate: trim count {t} leaves no model of {k}")
    if rows_ptr is None and k > base.shape[0]:
        raise ValueError(f"robust_aggregate: k = {k} exceeds the stack's {base.shape[0]} rows")
    if out.dtype != torch.float32 or out.numel() != P or not out.is_contiguous() or out.device != base.device:
        raise ValueError("robust_aggregate: out must be a contiguous float32 [P] tensor on base's device")
    _check(lib().fedmx_robust_agg(base.data_ptr(), rows_ptr or 0, state_ptr, out.data_ptr(), k, P, t,
                                  _stream(base.device)), "fedmx_robust_agg")
    return out


def robust_aggregate_stack(stack: torch.Tensor, t: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``robust_aggregate`` over a ``[k, P]`` stack in row order."""
    st = stack.contiguous()
    if out is None:
        out = torch.empty(st.shape[1], dtype=torch.float32, device=st.device)
    return robust_aggregate(st, None, int(st.shape[0]), t, out)


def krum_workspace_size(k: int) -> int:
    """float64 elements of the krum kernels' workspace for ``k`` models:
    ``D[k][k]``, ``score[k]``, then the compacted kept positions (``int32[k]``
    in the last ``k`` elements' bytes)."""
    return k * k + 2 * k


def krum_aggregate(base: torch.Tensor, rows_ptr: Optional[int], k: int, f: int, m: int, out: torch.Tensor,
                   state_ptr: int = 0, workspace: Optional[torch.Tensor] = None, kept_out=None,
                   score_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out`` = mean of the ``m`` models with the lowest Krum scores among
    ``base[rows[j]]``, j < k (score: the sum of a model's ``max(k - f - 2, 0)``
    smallest squared distances; ``protocol/aggregation.py``), added in
    row-table order (fedmx_krum.hip, three launches).  ``rows_ptr``:
    device-visible ``int64[k]``, or None for rows 0..k-1.  ``workspace``:
    float64, at least ``krum_workspace_size(k)`` elements on ``base``'s device
    (``[:k*k]`` the distances, then the scores unless ``score_out`` takes them,
    then the kept positions as int32); allocated when None.  ``kept_out``: an
    int32 ``[k]`` tensor on ``base``'s device, or a device-visible address,
    that receives the kept mask.  With ``state_ptr`` the launches write nothing
    when the int32 there is negative (no aggregator elected).  Raises
    ValueError for k, f or m out of range; nothing is launched."""
    if base.dim() != 2 or base.dtype != torch.float32 or not base.is_contiguous():
        raise ValueError("krum_aggregate: base must be a contiguous float32 [rows, P] tensor")
    P = int(base.shape[1])
    if not 1 <= k <= KRUM_MAX_K:
        raise ValueError(f"krum_aggregate: k = {k} models (1..{KRUM_MAX_K} supported)")
    if not 1 <= m <= k:
        raise ValueError(f"krum_aggregate: m = {m} kept models of {k}")
    if f < 0:
        raise ValueError(f"krum_aggregate: f = {f} poisoned models")
    if rows_ptr is None and k > base.shape[0]:
        raise ValueError(f"krum_aggregate: k = {k} exceeds the stack's {base.shape[0]} rows")
    if out.dtype != torch.float32 or out.numel() != P or not out.is_contiguous() or out.device != base.device:
        raise ValueError("krum_aggregate: out must be a contiguous float32 [P] tensor on base's device")
    need = krum_workspace_size(k)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=base.device)
    elif (workspace.dtype != torch.float64 or workspace.numel() < need or not workspace.is_contiguous()
          or workspace.device != base.device):
        raise ValueError(f"krum_aggregate: workspace must be a contiguous float64 tensor of >= {need} elements "
                         "on base's device")
    score_ptr = workspace.data_ptr() + 8 * k * k
    if score_out is not None:
        if (score_out.dtype != torch.float64 or score_out.numel() < k or not score_out.is_contiguous()
                or score_out.device != base.device):
            raise ValueError("krum_aggregate: score_out must be a contiguous float64 [k] tensor on base's device")
        score_ptr = score_out.data_ptr()
    kept_ptr = 0
    if isinstance(kept_out, torch.Tensor):
        if (kept_out.dtype != torch.int32 or kept_out.numel() < k or not kept_out.is_contiguous()
                or kept_out.device != base.device):
            raise ValueError("krum_aggregate: kept_out must be a contiguous int32 [k] tensor on base's device")
        kept_ptr = kept_out.data_ptr()
    elif kept_out is not None:
        kept_ptr = int(kept_out)
    _check(lib().fedmx_krum_agg(base.data_ptr(), rows_ptr or 0, state_ptr, out.data_ptr(), k, P, f, m,
                                workspace.data_ptr(), score_ptr, kept_ptr,
                                workspace.data_ptr() + 8 * (k * k + k), _stream(base.device)), "fedmx_krum_agg")
    return out


def krum_aggregate_stack(stack: torch.Tensor, f: int, m: int, out: Optional[torch.Tensor] = None,
                         **kw) -> torch.Tensor:
    """``krum_aggregate`` over a ``[k, P]`` stack in row order."""
    st = stack.contiguous()
    if out is None:
        out = torch.empty(st.shape[1], dtype=torch.float32, device=st.device)
    return krum_aggregate(st, None, int(st.shape[0]), f, m, out, **kw)


def geomed_workspace_size(k: int, P: int) -> int:
    """float64 elements of the geomed kernel's workspace for ``k`` models of
    ``P`` values: two halves of block partials ``part[ceil(P / 256)][k]``
    (successive launches read one and write the other)."""
    return 2 * (-(-int(P) // 256)) * int(k)


def _geomed_f64_out(name: str, t, k: int, device) -> int:
    """Address of a float64 ``[k]`` result: a tensor on ``device``, a
    device-visible address, or None."""
    if isinstance(t, torch.Tensor):
        if t.dtype != torch.float64 or t.numel() < k or not t.is_contiguous() or t.device != device:
            raise ValueError(f"geomed_aggregate: {name} must be a contiguous float64 [k] tensor on base's device")
        return t.data_ptr()
    return 0 if t is None else int(t)


def geomed_aggregate(base: torch.Tensor, rows_ptr: Optional[int], k: int, iters: int, nu: float, out: torch.Tensor,
                     state_ptr: int = 0, workspace: Optional[torch.Tensor] = None, weights_out=None,
                     dist_out=None) -> torch.Tensor:
    """``out`` = the smoothed geometric median of ``base[rows[j]]``, j < k,
    after ``iters`` Weiszfeld iterations with smoothing ``nu``
    (``protocol/aggregation.py``; fedmx_geomed.hip, ``iters + 2`` launches).
    ``rows_ptr``: device-visible ``int64[k]``, or None for rows 0..k-1.
    ``workspace``: float64, at least ``geomed_workspace_size(k, P)`` elements
    on ``base``'s device; allocated when None.  ``weights_out`` / ``dist_out``:
    float64 ``[k]`` tensors on ``base``'s device, or device-visible addresses,
    that receive the final weights and the squared distances they came from.
    With ``state_ptr`` the launches write nothing when the int32 there is
    negative (no aggregator elected).  Raises ValueError for k, iters or nu out
    of range; nothing is launched."""
    if base.dim() != 2 or base.dtype != torch.float32 or not base.is_contiguous():
        raise ValueError("geomed_aggregate: base must be a contiguous float32 [rows, P] tensor")
    if base.device.type != "cuda":
        raise ValueError("geomed_aggregate: base must be on a GPU device")
    P = int(base.shape[1])
    if P < 1:
        raise ValueError("geomed_aggregate: base has no columns")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= GEOMED_MAX_K:
        raise ValueError(f"geomed_aggregate: k = {k} models (1..{GEOMED_MAX_K} supported)")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= GEOMED_MAX_ITERS:
        raise ValueError(f"geomed_aggregate: iters = {iters} (an integer in 0..{GEOMED_MAX_ITERS})")
    if isinstance(nu, bool) or not isinstance(nu, (int, float, np.floating, np.integer)) \
            or not (float(nu) > 0.0 and math.isfinite(float(nu))):
        raise ValueError(f"geomed_aggregate: nu = {nu} (finite and > 0)")
    k, iters, nu = int(k), int(iters), float(nu)
    if rows_ptr is None and k > base.shape[0]:
        raise ValueError(f"geomed_aggregate: k = {k} exceeds the stack's {base.shape[0]} rows")
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.numel() != P
            or not out.is_contiguous() or out.device != base.device):
        raise ValueError("geomed_aggregate: out must be a contiguous float32 [P] tensor on base's device")
    need = geomed_workspace_size(k, P)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=base.device)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float64 or workspace.numel() < need
          or not workspace.is_contiguous() or workspace.device != base.device):
        raise ValueError(f"geomed_aggregate: workspace must be a contiguous float64 tensor of >= {need} elements "
                         "on base's device")
    w_ptr = _geomed_f64_out("weights_out", weights_out, k, base.device)
    d_ptr = _geomed_f64_out("dist_out", dist_out, k, base.device)
    _check(lib().fedmx_geomed_agg(base.data_ptr(), rows_ptr or 0, state_ptr, out.data_ptr(), k, P, iters, nu,
                                  workspace.data_ptr(), w_ptr, d_ptr, _stream(base.device)), "fedmx_geomed_agg")
    return out


def geomed_aggregate_stack(stack: torch.Tensor, iters: int, nu: float, out: Optional[torch.Tensor] = None,
                           **kw) -> torch.Tensor:
    """``geomed_aggregate`` over a ``[k, P]`` stack in row order."""
    st = stack.contiguous()
    if out is None:
        out = torch.empty(st.shape[1], dtype=torch.float32, device=st.device)
    return geomed_aggregate(st, None, int(st.shape[0]), iters, nu, out, **kw)


def param_drift(hist: torch.Tensor, new: torch.Tensor, seg: torch.Tensor, to_host: bool = False):
    """Per-row drift; a device tensor, or (``to_host``) a host view valid after the next sync."""
    dev = hist.device
    rt = runtime(dev)
    M = hist.shape[0]
    h = hist.contiguous()
    nw = new.contiguous()
    if to_host:
        optr, out = rt.out.take(np.float32, M)
    else:
        out = torch.empty(M, dtype=torch.float32, device=dev)
        optr = out.data_ptr()
    _check(lib().fedmx_param_drift(h.data_ptr(), M, nw.data_ptr(), seg.data_ptr(), optr, rt.stream),
           "fedmx_param_drift")
    return out


def standardize_ddof1(x: torch.Tensor, d_in: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dev = x.device
    y = torch.empty_like(x) if out is None else out
    _check(lib().fedmx_standardize_lds(x.data_ptr(), x.shape[0], d_in, y.data_ptr(), _stream(dev)),
           "fedmx_standardize_lds")
    return y


def ranks_share_device(environ=None, device_count=None) -> bool:
    """True when several ranks of this job run on one GPU (one-box
    rehearsals: ``FEDMX_DEVICE_INDEX`` pins every rank to one device, or
    torchrun started more local ranks than there are devices).  Their
    training launches then compete for the CUs, so a trainer's validator
    workgroup is no longer guaranteed to be resident beside it: those launches
    keep the synchronous epoch tail."""
    env = os.environ if environ is None else environ
    world = int(env.get("LOCAL_WORLD_SIZE", env.get("WORLD_SIZE", "1")))
    if world <= 1:
        return False
    if "FEDMX_DEVICE_INDEX" in env:
        return True
    n = torch.cuda.device_count() if device_count is None else device_count
    return world > n


class TrainBuffers:
    """Persistent per-store device buffers for the training launch."""

    def __init__(self, store):
        dev = store.params.device
        # the helper-wave kernel's data contract (engine/base.ClientStore):
        # whole 12- or 16-row chunks are read past the last client's end, and
        # X's padded column DP-1 is read as the bias input 1
        tail = int(store.train.shape[0]) - int(store.train_off[-1])
        if tail < 15:
            raise ValueError(f"training buffer needs >= 15 rows after the last client (has {tail}); "
                             "build it with ClientStore.load_data")
        if tuple(getattr(store, "bias_column_rows", ())) != ("train", "valid"):
            raise ValueError("training / validation buffers must hold 1 in column DP-1 (ClientStore._concat)")
        self.train_off = torch.from_numpy(store.train_off).to(dev)
        self.valid_off = torch.from_numpy(store.valid_off).to(dev)
        self.dev = dev
        self.vws: Optional[torch.Tensor] = None   # validator workspace [k][fedmx_train_av_slot()] (zeroed once)
        self.vseq = 0                            # launch number stamped into its flags

    def validator_workspace(self, k: int, n_rows: int):
        """(pointer, launch number) of the asynchronous-validation workspace
        for a k-client launch, or (None, 0) when k validators would not fit
        beside their trainers.  Allocated once (one slot per client the
        device can host a validator for, at most one per store row; never
        freed, so no in-flight launch loses it) and never cleared again:
        every launch stamps its flags with a new number, so stale flags of
        earlier launches never match."""
        if self.vws is None:
            cus = torch.cuda.get_device_properties(self.dev).multi_processor_count
            # one trainer + one validator CU per client, and this process alone
            # on the device (no validator when ranks share it)
            self.vslots = 0 if ranks_share_device() else max(0, min(int(n_rows), cus // 2))
            self.vws = torch.zeros(max(self.vslots, 1) * int(lib().fedmx_train_av_slot()), dtype=torch.float32,
                                   device=self.dev)
        if k > self.vslots:
            return None, 0
        self.vseq = self.vseq % 0xFFFFFFFF + 1
        return self.vws.data_ptr(), self.vseq


def train(store, local_ids: Sequence[int], hp, dims, stamps: Optional[torch.Tensor] = None,
          compact: Optional[bool] = None, helper: Optional[bool] = None, err: int = 0,
          async_valid: bool = True):
    """Launch the fused training kernel for store rows ``local_ids`` (async).
    Returns host views (tracking[k, E, 2], epochs_run[k], best_epoch[k])
    written by the kernel, valid after the next stream sync."""
    dev = store.params.device
    rt = runtime(dev)
    k = len(local_ids)
    bufs = getattr(store, "_train_bufs", None)
    if bufs is None:
        bufs = store._train_bufs = TrainBuffers(store)
    (iptr,) = rt.desc.put(np.asarray(local_ids, dtype=np.int32))
    tptr, trk = rt.out.take(np.float64, k * hp.epochs * 2)
    trk[:] = np.nan
    eptr, er = rt.out.take(np.int32, k)
    bptr, be = rt.out.take(np.int32, k)
    a = TrainArgs()
    a.params = store.params.data_ptr()
    a.adam_m = store.adam_m.data_ptr()
    a.adam_v = store.adam_v.data_ptr()
    a.anchor = store.anchor.data_ptr()
    a.best = store.best.data_ptr()
    a.adam_step = store.adam_step.data_ptr()
    a.train_x = store.train.data_ptr()
    a.train_off = bufs.train_off.data_ptr()
    a.valid_x = store.valid.data_ptr()
    a.valid_off = bufs.valid_off.data_ptr()
    a.client_idx = iptr
    a.tracking = tptr
    a.epochs_run = eptr
    a.best_epoch = bptr
    a.epochs = hp.epochs
    a.batch = hp.batch_size
    a.patience = hp.patience
    a.d_in, a.hidden, a.latent = dims.d_in, dims.hidden, dims.latent
    a.lr, a.beta1, a.beta2, a.eps = hp.lr, hp.beta1, hp.beta2, hp.eps
    a.lam, a.mu = hp.shrink_lambda, hp.fedprox_mu
    a.stamps = stamps.data_ptr() if stamps is not None else None
    a.err = err or None
    if TRAIN_ASYNC_VALID and async_valid:
        a.vws, a.vseq = bufs.validator_workspace(k, store.params.shape[0])
    a.flags = 0 if (TRAIN_COMPACT if compact is None else compact) else TRAIN_FLAG_NO_COMPACT
    helper_on = TRAIN_HELPER if helper is None else helper
    if helper_on is not None:
        a.flags |= TRAIN_FLAG_HELPER if helper_on else TRAIN_FLAG_NO_HELPER
    a.flags |= TRAIN_TEST_FLAGS
    rc = lib().fedmx_train(ctypes.byref(a), k, rt.stream)
    if rc == -2:
        raise ValueError(f"fused training kernel needs batch_size >= 1, got {hp.batch_size}")
    if rc == -3:
        raise ValueError(f"fused training kernel takes d_in 1..127, hidden 1..31 and latent 1..15, got "
                         f"{dims.d_in} / {dims.hidden} / {dims.latent}")
    _check(rc, "fedmx_train")
    return trk.reshape(k, hp.epochs, 2), er, be


def probe_mfma(device) -> np.ndarray:
    """One v_mfma_f32_16x16x4_f32 on A[i][k] = i + 100k, B[k][j] = 1000k + j."""
    out = torch.zeros(16 * 16, dtype=torch.float32, device=device)
    _check(lib().fedmx_probe_mfma(out.data_ptr(), _stream(device)), "fedmx_probe_mfma")
    return out.view(16, 16).cpu().numpy()
