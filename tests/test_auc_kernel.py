"""The inputs the single-workgroup AUC kernel (``auc_kernel``, fedmx_eval.hip)
is run over on the GPU (tests/test_auc_kernel_gpu.py), their reference
computed three independent ways that must agree to the bit, and the checks
``_hip.auc_desc`` makes before it hands raw pointers to the kernel.  CPU only."""
import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.eval.metrics import auc_chunked_numpy, read_scores
from fedmse_decentralized_amd.ops import _host, build

from test_auc_large import CASES

# (the fp32-overflow case overflows in numpy as it does in the kernel)
pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered in multiply")

DBL_MAX = np.finfo(np.float64).max
AUC_MAX_SORT = 8192
NETWORK_ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)
FAR_PROBE_ROWS = (3, 64, 1025)     # also against m + 20000 probe rows
EQUAL_ROWS = (1, 64, 4096)         # P == N
PADDING_ROWS = (5, 65, 1025)       # next power of two above m: the sort pads


def _tied(small, other, small_is_positive, seed):
    """``_tied`` of test_auc_large_gpu.py: two-decimal scores, dense ties."""
    rng = np.random.default_rng(seed)
    y = np.r_[np.full(small, int(small_is_positive)), np.full(other, int(not small_is_positive))].astype(np.int64)
    rng.shuffle(y)
    return np.round(rng.normal(size=len(y)) + 0.3 * y, 2), y


def _padding_edge(m, sorted_is_positive):
    """A sorted class of ``m`` rows and a probe class of ``3 m + 7``: a quarter
    of each +inf (read as DBL_MAX: ties at the last keys before the padding),
    an eighth -inf and an eighth NaN, the rest two-decimal scores."""
    rng = np.random.default_rng(31 * m + int(sorted_is_positive))
    other = 3 * m + 7
    y = np.r_[np.full(m, int(sorted_is_positive)), np.full(other, int(not sorted_is_positive))].astype(np.int64)
    s = np.round(rng.normal(size=m + other), 2)
    for first, rows in ((0, m), (m, other)):
        order = first + rng.permutation(rows)
        q, e = -(-rows // 4), -(-rows // 8)
        s[order[:q]] = np.inf
        s[order[q:q + e]] = -np.inf
        s[order[q + e:q + 2 * e]] = np.nan
    perm = rng.permutation(m + other)
    return s[perm], y[perm]


def _fp32_cases():
    rng = np.random.default_rng(115)
    out = []
    # neighbouring float32 values with a mantissa of 1.8 .. 2: their products with
    # 1/115 land in a binade whose float32 spacing is wider than the products',
    # so neighbours collide; the float64 product keeps every one of them apart.
    # Each positive's upper neighbour is a negative: a tie or not decides the AUC.
    base = (rng.uniform(1.8, 2.0, size=600) * 2.0 ** rng.integers(4, 12, size=600)).astype(np.float32)
    base = np.unique(base)
    up = np.nextafter(base, np.float32(np.inf))
    s = np.r_[base, up, up[::3]].astype(np.float32)
    y = np.r_[np.ones(len(base)), np.zeros(len(up)), np.ones(len(up[::3]))].astype(np.int64)
    perm = rng.permutation(len(s))
    out.append(("fp32-collide", s[perm], y[perm], 1.0 / 115))
    # products beyond float32: +-inf in float32, finite (and distinct) in float64
    s = np.round(rng.normal(size=400), 1).astype(np.float32)
    big = rng.choice(400, 120, replace=False)
    s[big[:80]] = rng.uniform(2.0e38, 3.3e38, size=80).astype(np.float32)
    s[big[80:]] = -rng.uniform(2.0e38, 3.3e38, size=40).astype(np.float32)
    out.append(("fp32-overflow", s, (rng.random(400) < 0.4).astype(np.int64), 2.0))
    # products below the smallest normal float32: subnormals and zeros
    s = rng.uniform(1e-39, 5e-38, size=500).astype(np.float32)
    s[::5] = -s[::5]
    out.append(("fp32-underflow", s, (rng.random(500) < 0.5).astype(np.int64), 1e-7))
    return out


def kernel_cases():
    """(name, scores, labels, f32_scale) of every input the GPU tests give
    ``auc_kernel``: the multi-workgroup path's grid, then every size at which
    the bitonic network, its padding and the thread stride change, +inf keys
    at the padding edge, signed zeros, the float32 read and other labels."""
    cases = list(CASES)
    for m in NETWORK_ROWS:
        for small_is_positive in (True, False):
            tag = "pos" if small_is_positive else "neg"
            cases.append((f"net{m}-{tag}", *_tied(m, m + 9, small_is_positive, m), 1.0))
            if m in FAR_PROBE_ROWS:
                cases.append((f"net{m}-far-{tag}", *_tied(m, m + 20000, small_is_positive, m + 1), 1.0))
    for m in EQUAL_ROWS:
        cases.append((f"equal{m}", *_tied(m, m, True, m + 2), 1.0))
    for m in PADDING_ROWS:
        for sorted_is_positive in (True, False):
            cases.append((f"pad{m}-{'pos' if sorted_is_positive else 'neg'}", *_padding_edge(m, sorted_is_positive), 1.0))
    rng = np.random.default_rng(11)
    cases.append(("zeros", rng.choice([-0.0, 0.0, np.nan], size=301), (rng.random(301) < 0.45).astype(np.int64), 1.0))
    cases += _fp32_cases()
    y = np.zeros(333, np.int64)
    marked = rng.choice(333, 120, replace=False)
    y[marked] = np.resize([-1, 2, np.iinfo(np.int32).min, 1], 120)
    cases.append(("labels", np.round(rng.normal(size=333) + 0.3 * (y != 0), 2), y, 1.0))
    return cases


KERNEL_CASES = kernel_cases()
# the cases whose larger class is beyond the LDS sort (the smaller never is)
LARGE_PROBE = {f"net{m}-{t}" for m in (8191, 8192) for t in ("pos", "neg")} | \
              {f"net{m}-far-{t}" for m in FAR_PROBE_ROWS for t in ("pos", "neg")}


def count_auc(scores, labels, f32_scale=1.0):
    """The AUC from the definition, in integers: over all (probe, key) pairs,
    L = keys below the probe value and E = keys equal to it, counted in the
    fully sorted smaller class (the positives when P = N); then the one
    division the kernel makes.  Twice the numerator stays an integer."""
    s = read_scores(scores, f32_scale)
    pos = np.asarray(labels) != 0
    P, N = int(pos.sum()), int((~pos).sum())
    if P == 0 or N == 0:
        return float("nan")
    keys, probe = (s[pos], s[~pos]) if P <= N else (s[~pos], s[pos])
    keys = np.sort(keys)
    lb = np.searchsorted(keys, probe, side="left")
    ub = np.searchsorted(keys, probe, side="right")
    L, E = int(lb.sum(dtype=np.int64)), int((ub - lb).sum(dtype=np.int64))
    twice = 2 * P * N - 2 * L - E if P <= N else 2 * L + E
    assert twice < 1 << 53
    return (0.5 * float(twice)) / float(P * N)


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


with np.errstate(over="ignore"):
    WANT = {name: count_auc(s, y, scale) for name, s, y, scale in KERNEL_CASES}


def test_names_are_unique_and_the_grid_is_included():
    names = [c[0] for c in KERNEL_CASES]
    assert len(set(names)) == len(names)
    assert names[:len(CASES)] == [c[0] for c in CASES]
    assert LARGE_PROBE <= set(names)


def test_three_references_agree_to_the_bit():
    for name, s, y, scale in KERNEL_CASES:
        chunked = auc_chunked_numpy(s, y, AUC_MAX_SORT, scale)
        host = _host.roc_auc(read_scores(s, scale), y)
        assert _same(chunked, WANT[name]) and _same(host, WANT[name]), (name, chunked, host, WANT[name])
        assert 0.0 <= WANT[name] <= 1.0
        if s.dtype == np.float64:   # the float32 copy the GPU grid also runs
            s32 = s.astype(np.float32)
            want = count_auc(s32, y, scale)
            assert auc_chunked_numpy(s32, y, AUC_MAX_SORT, scale) == want == _host.roc_auc(read_scores(s32, scale), y)


def test_cases_are_what_they_claim():
    by_name = {c[0]: c for c in KERNEL_CASES}
    for name, s, y, scale in KERNEL_CASES:
        P = int((y != 0).sum())
        N = len(y) - P
        assert 1 <= min(P, N) <= AUC_MAX_SORT, name
        assert (max(P, N) > AUC_MAX_SORT) == (name in LARGE_PROBE), name
        assert len(y) <= 22100, name
    for m in NETWORK_ROWS:
        for tag, positive in (("pos", 1), ("neg", 0)):
            y = by_name[f"net{m}-{tag}"][2]
            assert int((y == positive).sum()) == m and len(y) == 2 * m + 9
    for m in EQUAL_ROWS:
        y = by_name[f"equal{m}"][2]
        assert int(y.sum()) == m == len(y) - m
    for m in PADDING_ROWS:
        assert m & (m - 1)   # the sort pads
        for tag, positive in (("pos", 1), ("neg", 0)):
            _, s, y, _ = by_name[f"pad{m}-{tag}"]
            assert int((y == positive).sum()) == m < len(y) - m
            for dtype in (np.float64, np.float32):
                r = read_scores(s.astype(dtype))
                for cls in (y != 0, y == 0):
                    assert (r[cls] == DBL_MAX).sum() >= 2
                    assert (r[cls] == -DBL_MAX).any() and np.isnan(s[cls]).any()
    _, s, y, _ = by_name["zeros"]
    for cls in (y != 0, y == 0):
        assert np.isnan(s[cls]).any() and (np.signbit(s[cls]) & (s[cls] == 0)).any() \
            and (~np.signbit(s[cls]) & (s[cls] == 0)).any()
    assert WANT["zeros"] == 0.5
    _, s, y, scale = by_name["fp32-collide"]
    assert s.dtype == np.float32 and scale == 1.0 / 115
    read = read_scores(s, scale)
    assert len(np.unique(read)) < len(np.unique(s))
    assert len(np.unique(s.astype(np.float64) * scale)) == len(np.unique(s))   # the float64 product keeps them apart
    wide = s.astype(np.float64) * np.float64(np.float32(scale))
    assert _host.roc_auc(wide, y) != WANT["fp32-collide"]   # and gives another AUC
    _, s, y, scale = by_name["fp32-overflow"]
    assert s.dtype == np.float32 and scale == 2.0 and np.isfinite(s).all()
    read = read_scores(s, scale)
    for cls in (y != 0, y == 0):
        assert (read[cls] == DBL_MAX).sum() >= 2 and (read[cls] == -DBL_MAX).sum() >= 2
    assert _host.roc_auc(s.astype(np.float64) * 2.0, y) != WANT["fp32-overflow"]
    _, s, y, scale = by_name["fp32-underflow"]
    read = read_scores(s, scale)
    tiny = float(np.finfo(np.float32).tiny)
    assert s.dtype == np.float32 and (read == 0).any() and ((read != 0) & (np.abs(read) < tiny)).any()
    assert (np.abs(read) < tiny).all() and len(np.unique(read)) < 12
    _, s, y, _ = by_name["labels"]
    assert {-1, 2, np.iinfo(np.int32).min, 1, 0} == set(y.tolist())
    assert WANT["labels"] != count_auc(s, y == 1)


# ---------------------------------------------------------------------------
def _hip():
    from fedmse_decentralized_amd.ops import _hip

    return _hip


def test_auc_desc_fills_the_descriptor():
    _hip_ = _hip()
    s64, s32 = torch.zeros(7, dtype=torch.float64), torch.zeros(12, dtype=torch.float32)[1:10]
    y7, y9 = torch.zeros(7, dtype=torch.int32), torch.zeros(11, dtype=torch.int32)[2:]
    d = _hip_.auc_desc([s64, s32, s64[:0]], [y7, y9, y7[:0]], 4096, 0.25)
    assert d.dtype == _hip_.AUC_DTYPE and d.shape == (3,)
    assert d["score"].tolist()[:2] == [s64.data_ptr(), s32.data_ptr()]
    assert d["label"].tolist()[:2] == [y7.data_ptr(), y9.data_ptr()]
    assert d["out"].tolist() == [4096, 4104, 4112] and d["n"].tolist() == [7, 9, 0]
    assert d["score_is_f64"].tolist() == [1, 0, 1] and (d["score_scale"] == np.float32(0.25)).all()


@pytest.mark.parametrize("what", ["strided", "float16", "bfloat16", "int64 scores", "2-D", "2-D column", "0-D",
                                  "short labels", "long labels", "strided labels", "int64 labels", "2-D labels",
                                  "fewer label vectors", "more label vectors"])
def test_auc_desc_refuses(what):
    """Everything ``auc_kernel`` would read as if it were a contiguous float32
    / float64 vector with one contiguous int32 label per score."""
    _hip_ = _hip()
    s = torch.arange(8, dtype=torch.float64)
    y = torch.zeros(8, dtype=torch.int32)
    scores, labels = [s], [y]
    if what == "strided":
        scores, labels = [torch.arange(16, dtype=torch.float64)[::2]], [y]
    elif what == "float16":
        scores = [s.to(torch.float16)]
    elif what == "bfloat16":
        scores = [s.to(torch.bfloat16)]
    elif what == "int64 scores":
        scores = [s.to(torch.int64)]
    elif what == "2-D":
        scores = [s.reshape(8, 1)]
    elif what == "2-D column":
        scores = [torch.zeros(8, 3, dtype=torch.float32)[:, 1]]
    elif what == "0-D":
        scores, labels = [torch.zeros((), dtype=torch.float64)], [y[:1]]
    elif what == "short labels":
        labels = [y[:7]]
    elif what == "long labels":
        labels = [torch.zeros(9, dtype=torch.int32)]
    elif what == "strided labels":
        labels = [torch.zeros(16, dtype=torch.int32)[::2]]
    elif what == "int64 labels":
        labels = [y.to(torch.int64)]
    elif what == "2-D labels":
        labels = [y.reshape(8, 1)]
    elif what == "fewer label vectors":
        scores, labels = [s, s], [y]
    elif what == "more label vectors":
        scores, labels = [s], [y, y]
    with pytest.raises(ValueError):
        _hip_.auc_desc(scores, labels, 4096)
    # a good pair before the bad one does not let it through
    with pytest.raises(ValueError):
        _hip_.auc_desc([s] + scores, [y] + labels, 4096)


def test_descriptor_dtype_matches_the_library():
    if not build.HIP_LIB.exists():
        pytest.skip("kernel library not built")
    _hip_ = _hip()
    assert _hip_.lib().fedmx_auc_desc_size() == _hip_.AUC_DTYPE.itemsize == 40
    assert _hip_.AUC_MAX_SORT == AUC_MAX_SORT
