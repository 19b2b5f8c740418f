"""The chunked AUC rule of the multi-workgroup device path (README "Exact AUC
at any size"), stated in numpy (``eval.metrics.auc_chunked_numpy``), against
the host library's rank-sum AUC, to the bit; and the host-side grid sizing of
its pairs kernel.  CPU only."""
import numpy as np
import pytest

from fedmse_decentralized_amd.eval.metrics import auc_chunked_numpy, read_scores
from fedmse_decentralized_amd.ops import _host, build

SORT_ROWS = (1, 63, 64, 65, 128, 129, 1000)
PROBE_ROWS = (1, 5, 129, 3000)


def grid_cases():
    """(name, scores, labels, f32_scale) of the grid the CPU and the GPU tests
    share: a class of every size in SORT_ROWS against one of every size in
    PROBE_ROWS (the smaller of the two is the one the rule sorts), the first
    as the positives and then as the negatives, scores rounded to two
    decimals so ties span chunk boundaries; then the special score sets."""
    cases = []
    for m in SORT_ROWS:
        for other in PROBE_ROWS:
            for first_is_positive in (True, False):
                rng = np.random.default_rng(1000 * m + other)
                y = np.r_[np.full(m, int(first_is_positive)), np.full(other, int(not first_is_positive))]
                rng.shuffle(y)
                s = np.round(rng.normal(size=len(y)) + 0.3 * y, 2)
                cases.append((f"m{m}-p{other}-{'pos' if first_is_positive else 'neg'}", s, y, 1.0))
    rng = np.random.default_rng(7)
    y = np.r_[np.ones(129, np.int64), np.zeros(129, np.int64)]   # P = N: the positives are sorted
    rng.shuffle(y)
    cases.append(("P=N", np.round(rng.normal(size=258) + 0.3 * y, 2), y, 1.0))
    y = (rng.random(700) < 0.3).astype(np.int64)
    cases.append(("all-equal", np.full(700, 0.25), y, 1.0))
    cases.append(("separated-up", y + 0.25 * rng.random(700), y, 1.0))
    cases.append(("separated-down", -y - 0.25 * rng.random(700), y, 1.0))
    s = np.round(rng.normal(size=700), 1)
    s[rng.choice(700, 60, replace=False)] = np.nan
    s[rng.choice(700, 40, replace=False)] = np.inf
    s[rng.choice(700, 40, replace=False)] = -np.inf
    cases.append(("non-finite", s, y, 1.0))
    sse = (rng.gamma(2.0, 40.0, size=900) * 115).astype(np.float32)
    sse[::7] = sse[3]   # ties
    cases.append(("fp32-scaled", sse, (rng.random(900) < 0.6).astype(np.int64), 1.0 / 115))
    return cases


CASES = grid_cases()
WANT = {name: _host.roc_auc(read_scores(s, scale), y) for name, s, y, scale in CASES}


@pytest.mark.parametrize("chunk_keys", [64, 8192])
def test_chunked_rule_equals_the_host_auc_to_the_bit(chunk_keys):
    for name, s, y, scale in CASES:
        got = auc_chunked_numpy(s, y, chunk_keys, scale)
        assert got == WANT[name], (name, chunk_keys, got, WANT[name])
    assert WANT["all-equal"] == 0.5 and WANT["separated-up"] == 1.0 and WANT["separated-down"] == 0.0


def test_read_scores_follows_the_kernel():
    s = np.array([1.0, np.nan, np.inf, -np.inf, 230.0], dtype=np.float32)
    got = read_scores(s, 1.0 / 115)
    want = (s * np.float32(1.0 / 115)).astype(np.float64)
    assert got[0] == want[0] and got[4] == want[4] and got[1] == 0.0
    assert got[2] == np.finfo(np.float64).max and got[3] == -np.finfo(np.float64).max
    assert read_scores(np.array([0.1]), 1.0 / 115)[0] == 0.1   # f64: as is


@pytest.mark.parametrize("chunk_keys", [64, 8192])
def test_single_class_and_no_rows_are_nan(chunk_keys):
    assert np.isnan(auc_chunked_numpy(np.zeros(0), np.zeros(0, np.int64), chunk_keys))
    for lab in (0, 1):
        assert np.isnan(auc_chunked_numpy(np.arange(9.0), np.full(9, lab), chunk_keys))


def _hip():
    from fedmse_decentralized_amd.ops import _hip

    return _hip


@pytest.mark.parametrize("chunk_keys", [64, 8192])
def test_grid_covers_every_chunk_and_slice_once(chunk_keys):
    _hip_ = _hip()
    ck = chunk_keys
    sort_sizes = [1, ck - 1, ck, ck + 1, 2 * ck - 1, 2 * ck, 2 * ck + 1, 5 * ck + 3]
    probe_sizes = [1, 3, 1023, 1024, 1025, ck - 1, ck, ck + 1, 3 * ck + 1, 200_000]
    for m in sort_sizes:
        for npr in probe_sizes:
            chunks, slices = _hip_.auc_large_grid([m], [npr], ck)
            assert chunks == -(-m // ck) and 1 <= slices <= 65535
            for sl in {slices, 1, 7, npr + 5}:   # also more slices than probe rows
                hits = np.zeros((m, npr), dtype=np.uint8) if m * npr <= 4_000_000 else None
                keys = np.zeros(m, dtype=np.int64)
                rows = np.zeros(npr, dtype=np.int64)
                work = _hip_.auc_large_cover(m, npr, ck, sl)
                assert len(work) <= chunks * sl
                for (k0, k1), (p0, p1) in work:
                    assert 0 <= k0 < k1 <= m and k1 - k0 <= ck and 0 <= p0 <= p1 <= npr
                    if hits is not None:
                        hits[k0:k1, p0:p1] += 1
                    keys[k0:k1] += p1 - p0
                    rows[p0:p1] += k1 - k0
                if hits is not None:
                    assert (hits == 1).all(), (m, npr, sl)
                assert (keys == npr).all() and (rows == m).all(), (m, npr, sl)


def test_grid_fills_the_chip_and_takes_bounds():
    _hip_ = _hip()
    # one client, a 10,000-row class inside 100,000 rows: 2 chunks, one slice per 1024 probe rows
    assert _hip_.auc_large_grid([10_000], [90_000]) == (2, 88)
    # 1 M / 1 M: 123 chunks already fill the 512 resident workgroups with 5 slices
    chunks, slices = _hip_.auc_large_grid([1_000_000], [1_000_000])
    assert chunks == 123 and chunks * slices >= _hip_.AUC_LARGE_RESIDENT > chunks * (slices - 1)
    # several descriptors: the largest chunk count, slices from the sum of the chunks
    assert _hip_.auc_large_grid([9_000] * 10, [10_000] * 10) == (2, 10)
    # nothing to do: no chunk, and a valid grid all the same
    assert _hip_.auc_large_grid([0, 5], [7, 0]) == (0, 1)
    assert _hip_.auc_large_cover(0, 7, 64, 3) == [] and _hip_.auc_large_cover(5, 0, 64, 3) == []
    for bad in (32, 100, 16384):
        with pytest.raises(ValueError):
            _hip_.auc_large_grid([5], [7], bad)


def test_descriptor_dtype_matches_the_library():
    if not build.HIP_LIB.exists():
        pytest.skip("kernel library not built")
    _hip_ = _hip()
    L = _hip_.lib()
    assert L.fedmx_auc_large_desc_size() == _hip_.AUC_LARGE_DTYPE.itemsize == 56
    assert L.fedmx_auc_large_ctr_words() == _hip_.AUC_LARGE_CTR_WORDS
    assert L.fedmx_auc_large_max_rows() == _hip_.AUC_LARGE_MAX_ROWS == 1 << 26
