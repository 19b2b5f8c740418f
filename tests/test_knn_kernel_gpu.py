"""``knn_score_kernel`` (fedmx_knn.hip) at every list size, column group and
pass, bit for bit against the exact oracle of tests/knn_oracle.py (run with
``pytest -m gpu`` on an MI355X; tests/test_knn_kernel.py checks the oracle and
the inputs themselves on the CPU).  The inputs' scaler fit does not depend on
the summation order, so no comparison here has a tolerance except the one cell
named below.  Every launch writes into a sentinel-padded output: the slots
past the last query row keep the sentinel and every real slot is written.

Which case reaches which branch (T = KNN_TILE_ROWS = 480, read from the library)
-------------------------------------------------------------------------------
Instantiation ``knn_score_kernel<K>`` (its unrolled ``knn_insert<K>`` and its
``if (j < k_eff) sel = best[j]`` chain), n_train 40, n_query 70, Z = 7
(``knn_scan_tile<K, 2>``), one pass, one tile:
  K = 1..16, descriptor k = K     k_eff = K: the chain runs to its last entry
                                  (K = 1 has no chain and no shift loop)
  (k, K) = (1, 16), (1, 2)        k_eff = 1: no ``j < k_eff`` holds, sel = best[0]
  (15, 16), (2, 3), (7, 8)        the chain stops one entry before the list's end
  K = 16, k = 1 / 5 / 16 and a    k_eff differs between the workgroups of one
  3-row train set under k = 16    launch; 3 rows: k_eff = n_train = 3, best[3..15]
                                  still hold +inf and must not be selected
Column groups ``groups = (m + 3) >> 2`` -> ``knn_scan_tile<5, G>``, n_train 40,
n_query 70, k = 5:
  Z = 1..4   G = 1  (Z = 4: the group has no zero column)
  Z = 5..8   G = 2  (5: three zero columns; 8: none)
  Z = 9..12  G = 3
  Z = 13..16 G = 4  (16 = ZP: no zero column anywhere, the staging's ``sc < m``
                    and the query's ``c < m`` hold for every column)
  and through row-stride-16 views whose columns Z.. hold NaN (Z < 16): a read
  of one column too many gives NaN, which is never inserted: a score of +inf
Passes and tiles, Z = 2 (``knn_scan_tile<5, 1>``), k = 5, y workgroups per
descriptor given explicitly; workgroup w takes the rows from 256 w in steps of
256 y; "re-stage": ``staged != t0`` holds at a tile that is not the first one
staged (a train set of one tile is staged once, whatever the passes):
  (n_query, n_train)   y = 1                  y = 2                     y = 3
  (513, 2T + 1)        3 passes x 3 tiles     w0: 2 passes, w1: 1       1 pass each
                       (480, 480, 1 rows),    each pass 3 tiles,        3 tiles
                       9 stagings: tile 0     re-staged
                       again over the 1-row
                       tile in passes 2, 3
  (513, T + 1)         3 passes x 2 tiles,    w0: 2 passes, w1: 1       1 pass each
                       6 stagings
  (700, 40)            3 passes, 1 tile       w0: 2 passes (rows 0..,   1 pass each;
                       staged once            512..699), w1: 1 pass     w2 188 rows
                                              (256..511; 768 > 700)
  (257, T + 1)         2 passes x 2 tiles,    1 pass each, w1 one row   w2 returns
                       the second pass one
                       row; 4 stagings
  (255, T)             1 pass, 1 full tile    w1 returns at once        w1, w2 return
  (256, 2T)            1 pass, 2 full tiles   w1 returns                w1, w2 return
  (1, 2T + 1)          1 pass, 3 tiles, 255 idle threads; w1.. return
  and y = knn_grid_y (1, 2 or 3 here: the launch the engine makes).  One
  y = 1 launch holds (700, 40), (1, 2T + 1) and (257, T + 1): 3, 1 and 2
  passes side by side.
  (At n_query 257 and y = 2 each workgroup takes one pass; a workgroup 0 of
  two passes beside a workgroup 1 of one is n_query 513 and 700 at y = 2.)
  Every cell is compared with the exact oracle where it has one (up to
  ``knn_oracle.EXACT_TRIPLES``; with T = 480 that is every cell) and otherwise
  with ``knn_score_numpy`` at GPU_TOL; all y variants are equal to the bit.
Arrival orders, Z = 1 (``knn_scan_tile<K, 1>``), n_train 64, k in {1, 4, 16},
launched at capacity k and at capacity 16:
  descending   ``d2 < best[K - 1]`` holds for every row and every ``d2 < lo``:
               the whole list shifts each time
  ascending    after the first K rows the first compare fails: no insert
  identical    one insert per empty slot, then ``d2 < best[K - 1]`` fails on
               equal values; scale = 1 by the ``var <= upper`` branch
  tie3, tie2   equal d2 at sorted positions (k - 1, k, k + 1) and (k, k + 1):
               the strict compare keeps each copy once
Refusals: capacity 0 and 17, y = 0 and 65536 return an error and launch
nothing; n = 0 returns 0 and launches nothing.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_oracle as O  # noqa: E402
from fedmse_decentralized_amd.engine.torch_engine import knn_score_numpy  # noqa: E402
from test_knn_scorer import GPU_TOL  # noqa: E402

DEV = torch.device("cuda", 0)
SENTINEL = -7.0
EXTRA = 5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strided(a):
    """[n, Z] view with row stride 16 over a [n, 16] buffer whose other columns hold NaN."""
    buf = torch.full((a.shape[0], 16), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = _t(a)
    return buf[:, :a.shape[1]]


def launch(items, capacity, y=None, strided=False):
    """One ``fedmx_knn_score`` launch over items (train, query, descriptor k)
    at list capacity ``capacity`` and ``y`` workgroups per descriptor
    (``knn_grid_y`` when None) into a sentinel-padded output; the scores per item."""
    from fedmse_decentralized_amd.ops import _hip

    rt = _hip.runtime(DEV)
    wrap = _strided if strided else _t
    tr = [wrap(it[0]) for it in items]
    qu = [wrap(it[1]) for it in items]
    latent = items[0][0].shape[1]
    total = sum(int(q.shape[0]) for q in qu)
    out = torch.full((total + EXTRA,), SENTINEL, dtype=torch.float64, device=DEV)
    desc, views = _hip.knn_desc(tr, qu, out, latent, capacity)
    for i, it in enumerate(items):
        desc[i]["k"] = it[2]
    (dptr,) = rt.desc.put(desc)
    _hip._check(_hip.lib().fedmx_knn_score(dptr, len(desc), capacity, _hip.knn_grid_y(qu) if y is None else y,
                                           rt.stream), "fedmx_knn_score")
    rt.sync()
    host = out.cpu().numpy()
    assert np.all(host[total:] == SENTINEL), "slots beyond the launch's query rows were written"
    assert not np.any(host[:total] == SENTINEL), "a score was left unwritten"
    return [v.cpu().numpy() for v in views]


@pytest.fixture(scope="module")
def T():
    from fedmse_decentralized_amd.ops import _hip

    return _hip.knn_tile_rows()


# -- 1. every list size -----------------------------------------------------------------
@pytest.mark.parametrize("K", O.ALL_K)
def test_every_instantiation_at_its_own_capacity(K):
    train, query, s = O.list_case()
    (got,) = launch([(train, query, K)], K)
    O.assert_bits(got, O.kth_score(s, K), f"knn_score_kernel<{K}>, k = {K}")


@pytest.mark.parametrize("k,K", O.UNDER_CAPACITY)
def test_descriptor_k_below_the_launch_capacity(k, K):
    train, query, s = O.list_case()
    (wide,) = launch([(train, query, k)], K)
    (own,) = launch([(train, query, k)], k)
    O.assert_bits(wide, O.kth_score(s, k), f"k = {k} under capacity {K}")
    O.assert_bits(wide, own, f"k = {k} under capacity {K} against capacity {k}")


def test_one_launch_of_unequal_k_and_a_three_row_train_set():
    train, query, s = O.list_case()
    t3, q3, s3 = O.three_row_case()
    items = [(train, query, k) for k in O.MIXED_K] + [(t3, q3, 16), (t3, q3, 2)]
    got = launch(items, 16)
    for g, k in zip(got, O.MIXED_K):
        O.assert_bits(g, O.kth_score(s, k), f"k = {k} in the mixed launch")
    assert np.all(np.isfinite(got[3]))
    O.assert_bits(got[3], O.kth_score(s3, 3), "3 train rows under k = 16: the third nearest")
    O.assert_bits(got[4], O.kth_score(s3, 2), "3 train rows, k = 2")


# -- 2. every column count ----------------------------------------------------------------
@pytest.mark.parametrize("Z", O.ALL_Z)
def test_every_column_count(Z):
    train, query, scores = O.column_case()
    tr, qu = train[:, :Z], query[:, :Z]
    (got,) = launch([(tr, qu, O.COL_K)], O.COL_K)
    O.assert_bits(got, scores[Z - 1], f"Z = {Z}")
    if Z < 16:
        (view,) = launch([(tr, qu, O.COL_K)], O.COL_K, strided=True)
        O.assert_bits(view, got, f"Z = {Z} through row-stride-16 views")


# -- 3. passes and tiles ------------------------------------------------------------------
def _cell_scores(nq, nt):
    """{y: scores} of one cell at y = 1, 2, 3 and knn_grid_y, compared with the cell's reference."""
    train, query, want = O.pass_case(nq, nt)
    got = {}
    for y in O.PASS_Y + (None,):
        (got[y],) = launch([(train, query, O.PASS_K)], O.PASS_K, y=y)
    return train, query, want, got


@pytest.mark.parametrize("i", range(O.PASS_CELLS))
def test_passes_and_tiles(T, i):
    nq, nt = O.pass_cells(T)[i]
    train, query, want, got = _cell_scores(nq, nt)
    name = f"n_query {nq}, n_train {nt}"
    if want is not None:
        O.assert_bits(got[1], want, f"{name}, y = 1")
    else:
        ref = knn_score_numpy(train, query, O.PASS_K)
        err = np.max(np.abs(got[1] - ref) / (1.0 + np.abs(ref)))
        print(f"{name}: max |got - numpy| / (1 + |numpy|) = {err:.3e}")
        np.testing.assert_allclose(got[1], ref, rtol=GPU_TOL, atol=GPU_TOL, err_msg=name)
    for y in (2, 3, None):
        O.assert_bits(got[y], got[1], f"{name}, y = {y or 'knn_grid_y'} against y = 1")


def test_unequal_query_sets_in_one_single_workgroup_launch(T):
    cells = O.pass_mixed(T)
    cases = [O.pass_case(nq, nt) for nq, nt in cells]
    got = launch([(tr, qu, O.PASS_K) for tr, qu, _ in cases], O.PASS_K, y=1)
    for (nq, nt), (tr, qu, want), g in zip(cells, cases, got):
        assert want is not None
        O.assert_bits(g, want, f"n_query {nq}, n_train {nt} in the mixed y = 1 launch")


# -- 4. arrival orders --------------------------------------------------------------------
@pytest.mark.parametrize("k", O.ORDER_K)
@pytest.mark.parametrize("order", O.ORDERS)
def test_arrival_orders(order, k):
    train, query, d2 = O.order_case(order, k)
    want = O.kth_score(O.sorted_d2(d2), k)
    (got,) = launch([(train, query, k)], k)
    O.assert_bits(got, want, f"{order}, k = {k}")
    (wide,) = launch([(train, query, k)], 16)
    O.assert_bits(wide, want, f"{order}, k = {k} under capacity 16")


# -- 5. refusals --------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from fedmse_decentralized_amd.ops import _hip

    rt = _hip.runtime(DEV)
    train, query, _ = O.list_case()
    tr, qu = _t(train), _t(query)
    out = torch.full((query.shape[0] + EXTRA,), SENTINEL, dtype=torch.float64, device=DEV)
    desc, _ = _hip.knn_desc([tr], [qu], out, O.LIST_Z, 5)
    (dptr,) = rt.desc.put(desc)
    score = _hip.lib().fedmx_knn_score
    for what, n, k, y, refused in (("capacity 0", 1, 0, 1, True), ("capacity 17", 1, 17, 1, True),
                                   ("y = 0", 1, 5, 0, True), ("y = 65536", 1, 5, 65536, True),
                                   ("n = 0", 0, 5, 1, False)):
        status = score(dptr, n, k, y, rt.stream)
        rt.sync()
        assert (status != 0) == refused, (what, status)
        assert np.all(out.cpu().numpy() == SENTINEL), f"{what}: the output was written"
    # the same descriptor, accepted: the refusals above left nothing behind
    _hip._check(score(dptr, 1, 5, 1, rt.stream), "fedmx_knn_score")
    rt.sync()
    O.assert_bits(out.cpu().numpy()[:query.shape[0]], O.kth_score(O.list_case()[2], 5), "after the refusals")
