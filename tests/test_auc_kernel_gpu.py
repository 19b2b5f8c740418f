"""The single-workgroup AUC kernel (``auc_kernel``, fedmx_eval.hip) on the GPU
over ``test_auc_kernel.kernel_cases()``: equal to the integer-count AUC of the
read scores to the bit (no tolerance anywhere in this file), in both score
types, from offset views, in any row order, alone or among many unequal
descriptors, and equal to the multi-workgroup path's bits."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in multiply")]

from fedmse_decentralized_amd.models.layout import ModelDims
from fedmse_decentralized_amd.ops import _hip, _host

from test_auc_kernel import KERNEL_CASES, WANT, count_auc

DEV = torch.device("cuda")
_TORCH = {np.float32: torch.float32, np.float64: torch.float64}
SENTINEL = -7.0
EXTRA = 3


def _runs():
    """(name, scores, labels, scale, want) of every launch item: each case as
    it is, and each float64 case also rounded to float32 (read with the
    case's scale; its reference is the count over those float32 scores)."""
    out = []
    for name, s, y, scale in KERNEL_CASES:
        out.append((name, s, y, scale, WANT[name]))
        if s.dtype == np.float64:
            s32 = s.astype(np.float32)
            out.append((name + "/f32", s32, y, scale, count_auc(s32, y, scale)))
    return out


RUNS = _runs()
SCALES = sorted({r[3] for r in RUNS})


def _same(got, want):
    return (np.isnan(got) and np.isnan(want)) or got == want


def _dev(s, y, offset=1):
    """Scores and labels on the device as views ``base[offset : offset + n]``,
    the way the plans' SSE and score slices reach the kernel."""
    n = len(y)
    sb = torch.zeros(n + offset + 1, dtype=_TORCH[s.dtype.type])
    sb[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(s))
    yb = torch.full((n + offset + 1,), 1, dtype=torch.int32)
    yb[offset:offset + n] = torch.from_numpy(np.asarray(y).astype(np.int32))
    return sb.to(DEV)[offset:offset + n], yb.to(DEV)[offset:offset + n]


def _launch(pairs, scale, times=1):
    """``auc_desc`` + ``launch_auc`` into a device tensor holding a sentinel,
    ``EXTRA`` slots longer than the items: the results of every launch."""
    out = torch.full((len(pairs) + EXTRA,), SENTINEL, dtype=torch.float64, device=DEV)
    desc = _hip.auc_desc([p[0] for p in pairs], [p[1] for p in pairs], out.data_ptr(), scale)
    blob = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    torch.cuda.synchronize()
    got = []
    for _ in range(times):
        out.fill_(SENTINEL)
        _hip.launch_auc(blob, len(pairs), DEV)
        _hip.runtime(DEV).sync()
        torch.cuda.synchronize()
        got.append(out.cpu().numpy())
    return got


@pytest.fixture(scope="module")
def on_device():
    """Every run's offset views, uploaded once and left unchanged."""
    _hip.runtime(DEV)
    return {r[0]: _dev(r[1], r[2]) for r in RUNS}


def test_grid_in_one_launch_per_scale(on_device):
    seen = 0
    for scale in SCALES:
        sub = [r for r in RUNS if r[3] == scale]
        (got,) = _launch([on_device[r[0]] for r in sub], scale)
        assert (got[len(sub):] == SENTINEL).all()
        for (name, _, _, _, want), g in zip(sub, got):
            assert g != SENTINEL and _same(g, want), (name, g, want)
        seen += len(sub)
    assert seen == len(RUNS) > 2 * 100


def test_one_descriptor_per_launch(on_device):
    for name, s, y, scale, want in RUNS[::7]:
        (got,) = _launch([on_device[name]], scale)
        assert _same(got[0], want) and (got[1:] == SENTINEL).all(), (name, got, want)


def test_offsets_do_not_matter():
    """The same rows at offset 0 and at offset 3 of their buffers (a float32
    view then starts off an 8-byte boundary, a float64 one off a 16-byte one)."""
    names = ("net65-pos", "net65-pos/f32", "pad65-neg", "pad65-neg/f32", "fp32-collide")
    for name, s, y, scale, want in [r for r in RUNS if r[0] in names]:
        (got,) = _launch([_dev(s, y, 0), _dev(s, y, 3)], scale)
        assert got[0] == got[1] == want, (name, got, want)


def _tied(small, other, small_is_positive, seed):
    rng = np.random.default_rng(seed)
    y = np.r_[np.full(small, int(small_is_positive)), np.full(other, int(not small_is_positive))].astype(np.int64)
    rng.shuffle(y)
    return np.round(rng.normal(size=len(y)) + 0.3 * y, 2), y


def test_mixed_launch_and_relaunch(on_device):
    """Descriptors of very unequal work in one launch: no rows, single-class
    vectors, classes one beyond the LDS sort (-1: the caller's other path) and
    ordinary ones of both score types; launched twice, the same bytes."""
    rng = np.random.default_rng(70)
    special = [("no-rows", np.zeros(0), np.zeros(0, np.int64), float("nan")),
               ("no-rows/f32", np.zeros(0, np.float32), np.zeros(0, np.int64), float("nan")),
               ("all-positive", rng.normal(size=40), np.full(40, 3, np.int64), float("nan")),
               ("all-negative", rng.normal(size=1500).astype(np.float32), np.zeros(1500, np.int64), float("nan"))]
    for small_is_positive in (True, False):
        s, y = _tied(8193, 8193 + 9, small_is_positive, 8193)
        special.append((f"beyond-{small_is_positive}", s, y, -1.0))
    s, y = _tied(8193, 8193, True, 8194)
    special.append(("beyond-equal", s.astype(np.float32), y, -1.0))
    ordinary = [r for r in RUNS if r[3] == 1.0][::3]
    names = [sp[0] for sp in special] + [r[0] for r in ordinary]
    want = [sp[3] for sp in special] + [r[4] for r in ordinary]
    pairs = [_dev(s, y) for _, s, y, _ in special] + [on_device[r[0]] for r in ordinary]
    # the special ones spread among the others
    order = rng.permutation(len(pairs))
    assert len(pairs) >= 70 and {p[0].dtype for p in pairs} == {torch.float32, torch.float64}
    first, second = _launch([pairs[i] for i in order], 1.0, times=2)
    for slot, i in enumerate(order):
        assert _same(first[slot], want[i]), (names[i], first[slot], want[i])
    assert (first[len(pairs):] == SENTINEL).all()
    assert first.tobytes() == second.tobytes()


def test_row_order_does_not_matter():
    """The slot a key gets in LDS comes from an atomic counter: any order of
    the rows gives the same bits."""
    names = ("pad1025-pos", "net1025-far-neg", "equal4096", "net7-pos/f32", "fp32-collide", "labels")
    picked = [r for r in RUNS if r[0] in names]
    assert len(picked) == len(names)
    for name, s, y, scale, want in picked:
        perm = np.random.default_rng(len(y)).permutation(len(y))
        (got,) = _launch([_dev(s[perm], y[perm]), _dev(s[::-1], y[::-1])], scale)
        assert _same(got[0], want) and _same(got[1], want), (name, got, want)


def test_both_device_paths_agree(on_device):
    """``auc_large`` at 8192 and at 64 keys a chunk returns ``auc``'s bits."""
    rt = _hip.runtime(DEV)
    for scale in SCALES:
        sub = [r for r in RUNS if r[3] == scale]
        sc, lb = [on_device[r[0]][0] for r in sub], [on_device[r[0]][1] for r in sub]
        small = _hip.auc(sc, lb, scale)
        rt.sync()
        small = np.array(small)
        for chunk_keys in (8192, 64):
            large = _hip.auc_large(sc, lb, scale, chunk_keys=chunk_keys)
            rt.sync()
            large = np.array(large)
            for r, a, b in zip(sub, small, large):
                assert _same(a, r[4]) and _same(b, a), (r[0], chunk_keys, a, b, r[4])


def _raise(*a, **k):
    raise AssertionError("the host AUC must not be called")


def test_engine_takes_strided_views(monkeypatch):
    """A column of a 2-D tensor (row stride 3) gives the bits of its
    contiguous copy, in both score types, below and beyond the LDS sort."""
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine

    eng = HipEngine(ModelDims(115, 27, 7), DEV)
    monkeypatch.setattr(_host, "roc_auc", _raise)
    by_name = {r[0]: r for r in RUNS}
    big = _tied(8193, 8193 + 9, True, 8193)
    for dtype in (np.float64, np.float32):
        data = [by_name[n][1:3] for n in ("net65-neg", "pad1025-pos", "net8192-pos")] + [big]
        data = [(s.astype(dtype), y) for s, y in data]
        want = [count_auc(s, y) for s, y in data]
        wide, labels = [], []
        for k, (s, y) in enumerate(data):
            t = torch.full((len(y), 3), 1e3 * (k + 1), dtype=_TORCH[s.dtype.type])
            t[:, 1] = torch.from_numpy(s)
            wide.append(t.to(DEV))
            labels.append(torch.from_numpy(y.astype(np.int32)).to(DEV))
        views = [t[:, 1] for t in wide]
        assert not any(v.is_contiguous() for v in views)
        got = eng.auc(views, labels)
        copy = eng.auc([v.contiguous() for v in views], labels)
        assert got.tobytes() == copy.tobytes() and list(got) == want, (got, copy, want)
        with pytest.raises(ValueError):   # the raw binding refuses what the engine copies
            _hip.auc(views, labels)
    for bad in (torch.float16, torch.bfloat16, torch.int64):
        with pytest.raises(ValueError):
            eng.auc([views[0].to(bad)], labels[:1])
