"""Inputs and the exact oracle of ``knn_score_kernel`` (fedmx_knn.hip) for
tests/test_knn_kernel.py (CPU: the oracle and the inputs themselves) and
tests/test_knn_kernel_gpu.py (the kernel, bit for bit).

The kernel documents its arithmetic (header of fedmx_knn.hip); the only part
that depends on how the work is split over threads is the scaler fit, whose
float64 sums run in another order than numpy's.  The inputs here take that
dependence away:

* every latent is a multiple of 2^-8 with |v| <= 8 (``check_grid``);
* every train set is rows ``+x`` and ``-x`` plus one all-zero row when
  n_train is odd (``train_set``).

Then every partial sum of a column is a multiple of 2^-8 below 2^53 * 2^-8 and
exact in any order, the mean is exactly 0, ``df = x``, ``sum df = 0`` and
``sum df^2`` (multiples of 2^-16, at most 64 n) are exact in any order too, so
``var`` is one rounded division and ``scale`` one IEEE square root or the
``var <= upper`` -> 1.0 branch.  ``exact_fit`` computes the sums in rational
arithmetic, asserts that each is a float64, and rounds where the kernel does.

The scaled values (``t0 = fp32(v - mean)``, ``t1 = fp32(fp64(t0) / scale)``)
are elementwise IEEE operations, which numpy rounds as the device does; the
distance is a chain of true fused multiply-adds, which Python 3.10 lacks:
``fma_sq`` forms ``d * d + acc`` over the integers and rounds once (CPython's
``int / int`` is correctly rounded, which is also all ``Fraction.__float__``
does).  The selection counts NaN as +inf and duplicates with multiplicity."""
import functools
import math
from fractions import Fraction

import numpy as np

GRID = 256        # latents are multiples of 1 / GRID ...
LIMIT = 8.0       # ... of magnitude at most LIMIT
# (query, train, column) triples up to which a case gets the exact oracle: a second
# of Python integers; a larger cell is held to knn_score_numpy within GPU_TOL instead
EXACT_TRIPLES = 1_000_000


# -- the exact oracle ---------------------------------------------------------------
def check_grid(a):
    a = np.asarray(a)
    assert a.dtype == np.float32 and a.ndim == 2
    assert np.all(np.abs(a) <= LIMIT) and np.all(a * GRID == np.round(a * GRID)), "not on the 2^-8 grid"


def _as_f64(fr, what):
    """The float64 equal to the rational ``fr``; it is an error if there is none."""
    v = float(fr)
    assert Fraction(v) == fr, f"{what} is no float64: the fit would depend on the summation order"
    return v


def exact_fit(train):
    """(mean [Z], scale [Z]) float64 of ``fit_standard_scaler`` on a train set
    of the construction above: sums in rational arithmetic (each must be a
    float64, as must every ``df``), everything else rounded once per operation
    as the kernel's float64 code does."""
    check_grid(train)
    n, z = train.shape
    eps = float(np.finfo(np.float64).eps)
    nf = float(n)
    mean, scale = np.empty(z), np.empty(z)
    for c in range(z):
        col = [Fraction(float(v)) for v in train[:, c]]
        m = _as_f64(sum(col), "a column sum") / nf
        df = [Fraction(_as_f64(v - Fraction(m), "v - mean")) for v in col]
        a1 = _as_f64(sum(df), "sum df")
        a2 = _as_f64(sum(d * d for d in df), "sum df^2")
        var = (a2 - a1 * a1 / nf) / nf
        upper = nf * eps * var + (nf * m * eps) * (nf * m * eps)
        mean[c] = m
        scale[c] = 1.0 if var <= upper else math.sqrt(var)
    return mean, scale


def scaled(a, mean, scale):
    """``knn_scaled`` of every element, widened to float64."""
    a = np.asarray(a, dtype=np.float32)
    t0 = (a.astype(np.float64) - mean).astype(np.float32)
    t1 = (t0.astype(np.float64) / scale).astype(np.float32)
    return t1.astype(np.float64)


def fma_sq(d, acc):
    """``fma(d, d, acc)`` with one rounding (finite arguments; anything else
    gives what the fused operation gives too: inf or NaN)."""
    if not (math.isfinite(d) and math.isfinite(acc)):
        return d * d + acc
    n, s = d.as_integer_ratio()
    a, t = acc.as_integer_ratio()
    return (n * n * t + a * s * s) / (s * s * t)


def fma_sq_fraction(d, acc):
    """The same through ``Fraction`` (test_knn_kernel.py holds ``fma_sq`` to it)."""
    return float(Fraction(d) * Fraction(d) + Fraction(acc))


def exact_d2_prefixes(train, query, fit=None):
    """[Z, n_query, n_train] float64: entry [c] is the kernel's d2 accumulator
    after columns 0..c, so entry [Z' - 1] is the d2 of the first Z' columns
    (the fit is per column, so a prefix of the columns has the prefix's fit)."""
    mean, scale = exact_fit(train) if fit is None else fit
    x = scaled(train, mean, scale).tolist()
    q = scaled(query, mean, scale).tolist()
    z = len(mean)
    out = np.empty((z, len(q), len(x)), dtype=np.float64)
    for i, qi in enumerate(q):
        for j, xj in enumerate(x):
            acc = 0.0
            for c in range(z):
                acc = fma_sq(qi[c] - xj[c], acc)
                out[c, i, j] = acc
    return out


def exact_d2(train, query, fit=None):
    return exact_d2_prefixes(train, query, fit)[-1]


def sorted_d2(d2):
    """Rows sorted ascending, NaN as +inf."""
    d2 = np.where(np.isnan(d2), np.inf, d2)
    return np.sort(d2, axis=1)


def kth_score(d2_sorted, k):
    """sqrt of the min(k, n_train)-th smallest of every row of ``sorted_d2``."""
    out = np.sqrt(d2_sorted[:, min(int(k), d2_sorted.shape[1]) - 1])
    out.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: "
                           f"{got[bad[0]]!r} ({got[bad[0]].hex()}) != {want[bad[0]]!r} ({want[bad[0]].hex()})")


# -- inputs ---------------------------------------------------------------------------
def grid_rows(rng, n, z, limit=LIMIT):
    """[n, z] float32 multiples of 2^-8; column c spans +-limit / 2^(c % 4), so
    the columns' scales differ."""
    hi = np.array([int(limit * GRID) >> (c % 4) for c in range(z)])
    return (rng.integers(-hi, hi + 1, size=(n, z)) / GRID).astype(np.float32)


def symmetric(x, n_train, rng=None):
    """Rows ``+x`` and ``-x`` (and one zero row when n_train is odd), in the
    order given or shuffled by ``rng``."""
    assert 2 * x.shape[0] + n_train % 2 == n_train
    rows = np.concatenate([x, -x, np.zeros((n_train % 2, x.shape[1]), dtype=np.float32)]).astype(np.float32)
    rows += np.float32(0.0)            # (no -0.0 in the inputs)
    return rows if rng is None else rows[rng.permutation(n_train)]


def train_set(rng, n_train, z, limit=LIMIT):
    return symmetric(grid_rows(rng, n_train // 2, z, limit), n_train, rng)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# section 1: every list size ------------------------------------------------------
LIST_Z, LIST_TRAIN, LIST_QUERY = 7, 40, 70
ALL_K = tuple(range(1, 17))
UNDER_CAPACITY = ((1, 16), (15, 16), (2, 3), (7, 8), (1, 2))     # (descriptor k, launch capacity K)
MIXED_K = (1, 5, 16)


@functools.lru_cache(maxsize=None)
def list_case():
    """(train [40, 7], query [70, 7], sorted exact d2 [70, 40])."""
    rng = np.random.default_rng(9100)
    train, query = train_set(rng, LIST_TRAIN, LIST_Z), grid_rows(rng, LIST_QUERY, LIST_Z)
    return _frozen(train, query, sorted_d2(exact_d2(train, query)))


@functools.lru_cache(maxsize=None)
def three_row_case():
    """A train set of three rows (x, -x, 0): k_eff = 3 under any k >= 3."""
    rng = np.random.default_rng(9101)
    train, query = train_set(rng, 3, LIST_Z), grid_rows(rng, 33, LIST_Z)
    return _frozen(train, query, sorted_d2(exact_d2(train, query)))


# section 2: every column count -----------------------------------------------------
ALL_Z = tuple(range(1, 17))
COL_TRAIN, COL_QUERY, COL_K = 40, 70, 5


@functools.lru_cache(maxsize=None)
def column_case():
    """(train [40, 16], query [70, 16], scores [16, 70]): the case of Z columns
    is the first Z columns of both, and scores[Z - 1] its exact k = 5 score."""
    rng = np.random.default_rng(9200)
    train, query = train_set(rng, COL_TRAIN, 16), grid_rows(rng, COL_QUERY, 16)
    pre = exact_d2_prefixes(train, query)
    scores = np.stack([kth_score(sorted_d2(pre[z - 1]), COL_K) for z in ALL_Z])
    return _frozen(train, query, scores)


# section 3: passes and tiles -------------------------------------------------------
PASS_Z, PASS_K = 2, 5
PASS_Y = (1, 2, 3)              # and knn_grid_y
PASS_QUERY = (1, 255, 256, 257, 513, 700)
PASS_CELLS = 7


def pass_train_sizes(T):
    return (40, T, T + 1, 2 * T, 2 * T + 1)


def pass_cells(T):
    """(n_query, n_train) cells, each run at every y: a pruned product in
    which every value of both axes appears."""
    cells = [(513, 2 * T + 1), (700, 40), (257, T + 1), (255, T), (256, 2 * T), (1, 2 * T + 1), (513, T + 1)]
    assert len(cells) == PASS_CELLS and {c[0] for c in cells} == set(PASS_QUERY)
    assert {c[1] for c in cells} == set(pass_train_sizes(T))
    return cells


def pass_is_exact(n_query, n_train):
    return n_query * n_train * PASS_Z <= EXACT_TRIPLES


@functools.lru_cache(maxsize=None)
def pass_case(n_query, n_train):
    """(train, query, exact k = 5 scores or None where the cell is too large
    for the rational oracle)."""
    rng = np.random.default_rng(9300 + 7 * n_query + n_train)
    train, query = train_set(rng, n_train, PASS_Z), grid_rows(rng, n_query, PASS_Z)
    want = kth_score(sorted_d2(exact_d2(train, query)), PASS_K) if pass_is_exact(n_query, n_train) else None
    return _frozen(train, query) + (want,)


def pass_mixed(T):
    """Cells of one y = 1 launch: unequal n_query 700, 1, 257."""
    return [(700, 40), (1, 2 * T + 1), (257, T + 1)]


# section 4: arrival orders ---------------------------------------------------------
ORDER_TRAIN, ORDER_QUERY = 64, 70
ORDER_K = (1, 4, 16)
ORDERS = ("descending", "ascending", "identical", "tie3", "tie2")


def _distinct_positive(rng, count):
    """``count`` distinct multiples of 2^-8 in (0, 4], largest first."""
    return np.sort(rng.choice(np.arange(1, 4 * GRID + 1), size=count, replace=False))[::-1] / GRID


@functools.lru_cache(maxsize=None)
def order_case(order, k):
    """(train [64, 1], query [70, 1], exact d2 [70, 64] in arrival order).
    The queries lie in [5, 8], above every train value (at most 4), and the
    scaling is monotone, so a larger train value is a nearer one for every
    query row alike.  With ``s`` the d2 of a row sorted ascending (0-based):

    descending  train values ascending: every row is nearer than all before it
    ascending   train values descending: after the first K rows nothing is inserted
    identical   every train row 0 (rows +0 and -0 = 0): variance 0, scale 1, 64 equal d2
    tie3        s[k - 1] = s[k] = s[k + 1], three copies of one value (and
                nothing else equal to them), shuffled
    tie2        s[k - 1] < s[k] = s[k + 1], two copies just past the list, shuffled
    """
    rng = np.random.default_rng(9400 + 20 * ORDERS.index(order) + k)
    half = ORDER_TRAIN // 2
    if order in ("descending", "ascending"):
        pos = _distinct_positive(rng, half)
        vals = np.sort(np.r_[pos, -pos])
        train = (vals if order == "descending" else vals[::-1]).astype(np.float32)[:, None]
    elif order == "identical":
        train = np.zeros((ORDER_TRAIN, 1), dtype=np.float32)
    else:
        copies, lead = (3, k - 1) if order == "tie3" else (2, k)
        pos = _distinct_positive(rng, half - copies + 1)
        pos = np.r_[pos[:lead], np.full(copies, pos[lead]), pos[lead + 1:]]
        assert pos.size == half
        train = symmetric(pos.astype(np.float32)[:, None], ORDER_TRAIN, rng)
    train = np.ascontiguousarray(train)
    query = (rng.integers(5 * GRID, 8 * GRID + 1, size=(ORDER_QUERY, 1)) / GRID).astype(np.float32)
    return _frozen(train, query, exact_d2(train, query))
