"""The inputs and the exact oracle that tests/test_knn_kernel_gpu.py holds
``knn_score_kernel`` to (tests/knn_oracle.py), checked on the CPU: the
construction gives ``StandardScaler`` the oracle's fit to the bit, the oracle
agrees with ``knn_score_numpy`` within the project's tolerance, every arrival
order is what it claims, and the case lists cover every value of every axis."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_oracle as O  # noqa: E402
from fedmse_decentralized_amd.data.scaler import StandardScaler  # noqa: E402
from fedmse_decentralized_amd.engine.torch_engine import knn_score_numpy  # noqa: E402
from test_knn_scorer import GPU_TOL, tile_rows  # noqa: E402


def every_case():
    """(name, train, query, k, exact scores or None) of every launch item of the GPU file."""
    T = tile_rows()
    out = []
    train, query, s = O.list_case()
    out += [(f"list k{k}", train, query, k, O.kth_score(s, k)) for k in O.ALL_K]
    train, query, s = O.three_row_case()
    out.append(("three rows", train, query, 16, O.kth_score(s, 16)))
    train, query, scores = O.column_case()
    out += [(f"Z{z}", np.ascontiguousarray(train[:, :z]), np.ascontiguousarray(query[:, :z]), O.COL_K, scores[z - 1])
            for z in O.ALL_Z]
    for nq, nt in O.pass_cells(T):
        train, query, want = O.pass_case(nq, nt)
        out.append((f"pass q{nq} n{nt}", train, query, O.PASS_K, want))
    for order in O.ORDERS:
        for k in O.ORDER_K:
            train, query, d2 = O.order_case(order, k)
            out.append((f"{order} k{k}", train, query, k, O.kth_score(O.sorted_d2(d2), k)))
    return out


@pytest.fixture(scope="module")
def cases():
    return every_case()


# -- the oracle's own arithmetic --------------------------------------------------------
def test_fma_sq_rounds_once():
    rng = np.random.default_rng(1)
    d = (rng.normal(size=4000) * 2.0 ** rng.integers(-20, 8, size=4000)).tolist()
    acc = np.abs(rng.normal(size=4000) * 2.0 ** rng.integers(-30, 12, size=4000)).tolist()
    acc[:50] = [0.0] * 50
    two_roundings = 0
    for x, a in zip(d, acc):
        got = O.fma_sq(x, a)
        assert got == O.fma_sq_fraction(x, a)
        two_roundings += got != x * x + a
    assert two_roundings > 100       # the inputs tell a fused multiply-add from a multiply and an add
    # a case worked by hand: (1 + 2^-30)^2 - 1 = 2^-29 + 2^-60 exactly; the product alone rounds to 1 + 2^-29
    x = 1.0 + 2.0 ** -30
    assert O.fma_sq(x, 0.0) == 1.0 + 2.0 ** -29
    assert Fraction(O.fma_sq(x, 2.0 ** 30)) == Fraction(2 ** 30 + 1)
    assert x * x - (1.0 + 2.0 ** -29) == 0.0 and O.fma_sq(x, -(1.0 + 2.0 ** -29)) == 2.0 ** -60
    assert O.fma_sq(float("inf"), 1.0) == float("inf") and np.isnan(O.fma_sq(float("nan"), 1.0))


def test_selection_counts_nan_as_inf_and_duplicates_with_multiplicity():
    d2 = np.array([[4.0, np.nan, 1.0, 1.0, 9.0], [np.nan, np.nan, np.inf, 0.0, 0.0]])
    s = O.sorted_d2(d2)
    np.testing.assert_array_equal(s, [[1.0, 1.0, 4.0, 9.0, np.inf], [0.0, 0.0, np.inf, np.inf, np.inf]])
    np.testing.assert_array_equal(O.kth_score(s, 2), [1.0, 0.0])
    np.testing.assert_array_equal(O.kth_score(s, 3), [2.0, np.inf])
    np.testing.assert_array_equal(O.kth_score(s, 16), [np.inf, np.inf])      # min(k, n_train)


def test_fit_refuses_inputs_whose_sums_depend_on_the_order():
    rng = np.random.default_rng(2)
    good = O.train_set(rng, 41, 3)
    O.exact_fit(good)
    off_grid = good.copy()
    off_grid[0, 0] += np.float32(2.0 ** -12)
    with pytest.raises(AssertionError):
        O.exact_fit(off_grid)
    lopsided = good.copy()
    lopsided[0, 1] = np.float32(1.0) if lopsided[0, 1] != 1.0 else np.float32(2.0)   # mean k / (256 * 41): no float64
    with pytest.raises(AssertionError):
        O.exact_fit(lopsided)


# -- the three checks of the inputs -------------------------------------------------------
def test_standard_scaler_gives_the_exact_fit_to_the_bit(cases):
    """Proves the construction (an order-independent fit), not the kernel."""
    seen_unit_scale = False
    for name, train, query, k, _ in cases:
        O.check_grid(train)
        O.check_grid(query)
        mean, scale = O.exact_fit(train)
        sc = StandardScaler().fit(train)
        O.assert_bits(sc.mean_, mean, f"{name}: mean")
        O.assert_bits(sc.scale_, scale, f"{name}: scale")
        assert np.all(O.bits(mean) == 0), name                 # +0.0
        # any row order gives the same bits
        O.assert_bits(StandardScaler().fit(train[::-1]).scale_, scale, f"{name}: scale of the reversed rows")
        seen_unit_scale |= bool(np.any(scale == 1.0) and np.all(train == 0))
    assert seen_unit_scale       # the var <= upper branch (the identical-rows order)


def test_exact_oracle_agrees_with_knn_score_numpy(cases):
    exact = 0
    for name, train, query, k, want in cases:
        if want is None:
            continue
        exact += 1
        ref = knn_score_numpy(train, query, k)
        err = np.max(np.abs(want - ref) / (1.0 + np.abs(ref)))
        print(f"{name}: max |exact - numpy| / (1 + |numpy|) = {err:.3e}")
        np.testing.assert_allclose(want, ref, rtol=GPU_TOL, atol=GPU_TOL, err_msg=name)
        assert np.all(np.isfinite(want))
    assert exact >= len(cases) - 1


@pytest.mark.parametrize("k", O.ORDER_K)
def test_arrival_orders_are_what_they_claim(k):
    n = O.ORDER_TRAIN
    for order in O.ORDERS:
        train, query, d2 = O.order_case(order, k)
        assert train.shape == (n, 1) and query.shape == (O.ORDER_QUERY, 1) and d2.shape == (O.ORDER_QUERY, n)
        assert query.min() > np.abs(train).max()            # outside the train range
        s = np.sort(d2, axis=1)
        b = O.bits(s)
        if order == "descending":
            assert np.all(d2[:, 1:] < d2[:, :-1])           # every row goes to the front of the list
        elif order == "ascending":
            assert np.all(d2[:, 1:] > d2[:, :-1])           # nothing is inserted after the first K rows
        elif order == "identical":
            assert np.all(O.bits(d2) == O.bits(d2)[:, :1]) and np.all(d2 > 0)
        elif order == "tie3":
            assert np.all(b[:, k - 1] == b[:, k]) and np.all(b[:, k] == b[:, k + 1])
            assert np.all(s[:, k + 2] > s[:, k + 1])
            assert k == 1 or np.all(s[:, k - 2] < s[:, k - 1])
        else:
            assert np.all(b[:, k] == b[:, k + 1])
            assert np.all(s[:, k - 1] < s[:, k]) and np.all(s[:, k + 2] > s[:, k + 1])
        if order in ("tie3", "tie2"):
            # the same order for every query row, and not a sorted one
            arrival = np.argsort(d2, axis=1, kind="stable")
            assert np.all(np.sort(d2, axis=1) == np.take_along_axis(d2, arrival[:1].repeat(len(d2), 0), 1))
            assert not np.all(np.diff(d2[0]) >= 0) and not np.all(np.diff(d2[0]) <= 0)


def test_case_lists_cover_every_value_of_every_axis():
    T = tile_rows()
    assert O.ALL_K == tuple(range(1, 17)) and O.ALL_Z == tuple(range(1, 17))
    assert all(1 <= k < K <= 16 for k, K in O.UNDER_CAPACITY)
    assert set(O.UNDER_CAPACITY) == {(1, 16), (15, 16), (2, 3), (7, 8), (1, 2)}
    assert (O.LIST_TRAIN, O.LIST_QUERY, O.LIST_Z) == (40, 70, 7)
    assert (O.COL_TRAIN, O.COL_QUERY, O.COL_K) == (40, 70, 5)
    train, query, _ = O.three_row_case()
    assert train.shape[0] == 3
    cells = O.pass_cells(T)
    assert {c[0] for c in cells} == {1, 255, 256, 257, 513, 700}
    assert {c[1] for c in cells} == {40, T, T + 1, 2 * T, 2 * T + 1}
    assert O.PASS_Y == (1, 2, 3) and (O.PASS_Z, O.PASS_K) == (2, 5)
    for cell in [(513, 2 * T + 1), (700, 40), (257, T + 1), (255, T)] + O.pass_mixed(T):
        assert cell in cells
    assert [c[0] for c in O.pass_mixed(T)] == [700, 1, 257]
    # at most the largest cell (three passes over three tiles) is beyond the rational oracle
    assert all(O.pass_is_exact(*c) for c in cells if c != (513, 2 * T + 1))
    for nq, nt in cells:
        train, query, want = O.pass_case(nq, nt)
        assert train.shape == (nt, 2) and query.shape == (nq, 2) and (want is None) == (not O.pass_is_exact(nq, nt))
    assert O.ORDER_K == (1, 4, 16) and O.ORDER_TRAIN == 64
    assert set(O.ORDERS) == {"descending", "ascending", "identical", "tie3", "tie2"}
