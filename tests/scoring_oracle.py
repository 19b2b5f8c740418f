"""Inputs and plain references shared by the scoring-chain tests
(``test_scoring_chain.py`` on the CPU, ``test_scoring_chain_gpu.py`` on the GPU).

The chain: vote standardisation, the row forward, the score reduction, the
weighted sum, adoption (row broadcast and the small f64 copies) and the CEN
scorer.  Every builder here returns fp32 values exactly as the kernels read
them; the references compute in float64 (or wider) from those same values.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from fedmse_decentralized_amd.data.scaler import StandardScaler
from fedmse_decentralized_amd.models.layout import DP

# -- 1. standardisation ---------------------------------------------------------
STD_CHUNK = 256                                  # rows standardize_lds_kernel stages at once
STD_ROWS = [255, 256, 257, 511, 512, 513, 1000]
STD_WIDTHS = [1, 115, 127]
STD_TOL = (1e-5, 1e-5)                           # rtol, atol of the project's tests of this kernel
STD_CONST = (513, 0)                             # (n, column) of the constant-column case
# seed of a case whose default seed (100 * d_in + n) lets the fp32 TorchEngine
# use more than half of STD_TOL: (d_in, n) -> seed.  None needed so far.
STD_SEEDS: Dict[Tuple[int, int], int] = {}


def std_seed(d_in: int, n: int) -> int:
    return STD_SEEDS.get((d_in, n), 100 * d_in + n)


@functools.lru_cache(maxsize=None)
def std_case(d_in: int, n: int, const_col: int = -1) -> torch.Tensor:
    """fp32 [n, DP]: real columns randn * 4 + 2, finite garbage in the padded
    columns d_in..126, 1 in column 127 (the stores' bias column).  With
    ``const_col`` that real column holds one value.  Callers must not modify it."""
    g = torch.Generator().manual_seed(std_seed(d_in, n))
    x = torch.randn(n, DP, generator=g) * 100.0      # garbage everywhere first
    x[:, :d_in] = torch.randn(n, d_in, generator=g) * 4.0 + 2.0
    x[:, DP - 1] = 1.0
    if const_col >= 0:
        x[:, const_col] = float(np.float32(3.1))
    return x


def std_reference(x: torch.Tensor, d_in: int) -> torch.Tensor:
    """float64 (x - mean) / (std_ddof1 + 1e-8) of the real columns."""
    xr = x[:, :d_in].double()
    return (xr - xr.mean(0)) / (xr.std(0) + 1e-8)


# -- 2. score reduction -----------------------------------------------------------
SCORE_THREADS = 1024
REDUCE_SINGLE = [0, 1, 2, 3, 4, 7, 4095, 4096, 12287, 12288, 12291, 12292, 12293, 16387, 53001]
REDUCE_BATCHED = [(3000, b) for b in (1, 128, 1024, 1025, 2999, 3000, 5000)] + [(129, 128)]
REDUCE_D_IN = 115


def exact_sse(n: int) -> torch.Tensor:
    """fp32 [n]: ((i * 2654435761) mod 2^20) / 1024 — distinct multiples of
    2^-10 below 2^10, so a float64 sum of up to 2^20 of them is below 2^30
    with 2^-10 granularity (40 bits): exact in any order."""
    i = np.arange(n, dtype=np.uint64)
    v = ((i * np.uint64(2654435761)) % np.uint64(1 << 20)).astype(np.float64) / 1024.0
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return torch.from_numpy(out)


def reduce_path(n: int, k: int) -> dict:
    """What score_reduce_block's single-batch path does with n floats that
    start k floats past a 16-byte boundary: the head, the float4 count, the
    unrolled-loop iterations of the busiest / idlest thread, the threads in
    the remainder loop's last pass and the tail length."""
    head = min(n, (4 - k) & 3)
    n4 = (n - head) >> 2
    unrolled = [0, 0]
    for j, tid in enumerate((0, SCORE_THREADS - 1)):
        i = tid
        while i + 3 * SCORE_THREADS < n4:
            unrolled[j] += 1
            i += 4 * SCORE_THREADS
    done = 4 * SCORE_THREADS * unrolled[0]
    return {"head": head, "n4": n4, "unrolled_max": unrolled[0], "unrolled_min": unrolled[1],
            "remainder": max(0, n4 - done), "tail": n - head - 4 * n4}


def fsum_scores(x: np.ndarray, d_in: int) -> float:
    """Exactly rounded single-batch score: fsum(x) / (n * d_in)."""
    return math.fsum(np.asarray(x, dtype=np.float64).tolist()) / (len(x) * d_in)


# -- 4. weighted sum ----------------------------------------------------------------
WSUM_K = [1, 2, 9, 64]
WSUM_P = [4, 1028]          # and P_PAD, which the tests add
# seed of a case whose default seed (1000 * K + P) gives a sum that a fused
# multiply-add would round alike in every element (the four-element cases)
WSUM_SEEDS: Dict[Tuple[int, int], int] = {(2, 4): 3, (9, 4): 3}   # seeds 1 and 2 round alike too


def wsum_case(K: int, P: int) -> Tuple[torch.Tensor, List[float]]:
    """(stack fp32 [K, P], weights).  K >= 9 carries every special: weight 1 is
    0 over an inf in column 0 (NaN), weight 2 negative, weight 3 subnormal and
    alone in column 2 (a subnormal result), weight 4 large over a 2.0 alone in
    column 1 (the product overflows to inf).  K = 2: two ordinary weights, one
    negative.  K = 1: a negative subnormal weight (subnormal products)."""
    g = torch.Generator().manual_seed(WSUM_SEEDS.get((K, P), 1000 * K + P))
    stack = torch.randn(K, P, generator=g)
    if K == 1:
        return stack, [-1e-40]
    if K == 2:
        return stack, [0.6180339, -0.37]
    w = (torch.rand(K, generator=g) * 0.2 + 0.01).tolist()
    w[1], w[2], w[3], w[4] = 0.0, -0.37, 1e-40, 3e38
    stack[4] = 0.0                 # the large weight meets zeros but for column 1
    stack[:, 1] = 0.0
    stack[4, 1] = 2.0
    stack[:, 2] = 0.0              # only the subnormal product in column 2
    stack[3, 2] = 1.5
    stack[1, 0] = float("inf")
    return stack, w


def wsum_sequential(stack: torch.Tensor, weights) -> torch.Tensor:
    """The reference's python sum() over fp32 tensors: every product and every
    sum rounded to fp32, in row order from the first product."""
    w = torch.tensor(list(weights), dtype=torch.float32)
    ref = stack[0] * w[0]
    for k in range(1, stack.shape[0]):
        ref = ref + stack[k] * w[k]
    return ref


def wsum_fused(stack: torch.Tensor, weights) -> torch.Tensor:
    """The same sum with each multiply-add fused: the fp32 x fp32 product is
    exact in float64, added to the running fp32 sum there, rounded once."""
    w = torch.tensor(list(weights), dtype=torch.float32).double()
    s = stack.double()
    ref = (s[0] * w[0]).float()
    for k in range(1, stack.shape[0]):
        ref = (ref.double() + s[k] * w[k]).float()
    return ref


def same_floats(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-equal where neither is NaN, NaN in the same places (a NaN's
    payload is the hardware's choice, not the formula's)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.view(it)[~na], b.view(it)[~nb])


# -- 5. CEN ---------------------------------------------------------------------------
CEN_TRAIN = [1, 2, 255, 257, 70001]
CEN_TEST = [0, 1, 2047, 2048, 2049]
CEN_LATENT = [1, 7, 15]
CEN_TOL = (1e-12, 1e-12)
CEN_ILL_MEAN, CEN_ILL_STD = 1e3, 1e-2     # the ill-conditioned train set (the offset needed no scaling down)
CEN_ILL_ROWS = 70001


@functools.lru_cache(maxsize=None)
def cen_train(n: int, latent: int) -> np.ndarray:
    rng = np.random.default_rng(7000 + 31 * latent + n)
    return (rng.normal(size=(n, latent)) * 3 + 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cen_test(n: int, latent: int) -> np.ndarray:
    rng = np.random.default_rng(9000 + 31 * latent + n)
    return (rng.normal(size=(n, latent)) * 5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cen_ill(latent: int) -> Tuple[np.ndarray, np.ndarray]:
    """(train, test): every train column has mean 1e3 and standard deviation
    1e-2 (fp32 values on the 2^-14 grid there), the last one is constant;
    test rows lie five deviations around the same mean."""
    rng = np.random.default_rng(500 + latent)
    tr = (CEN_ILL_MEAN + CEN_ILL_STD * rng.normal(size=(CEN_ILL_ROWS, latent))).astype(np.float32)
    if latent > 1:
        tr[:, latent - 1] = np.float32(1000.25)
    te = (CEN_ILL_MEAN + 5 * CEN_ILL_STD * rng.normal(size=(2049, latent))).astype(np.float32)
    return tr, te


def wide_sum_is_longdouble() -> bool:
    return np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def _colsum(a: np.ndarray) -> np.ndarray:
    """Column sums carried wider than double: in numpy.longdouble where that
    is wider, else exactly (math.fsum)."""
    if wide_sum_is_longdouble():
        return np.sum(a.astype(np.longdouble), axis=0)
    return np.array([math.fsum(a[:, j].tolist()) for j in range(a.shape[1])], dtype=np.float64)


def cen_score_wide(train_lat: np.ndarray, test_lat: np.ndarray) -> np.ndarray:
    """cen_score_numpy with the scaler fitted in wider arithmetic: the same
    corrected two-pass variance and near-constant rule, the sums (and, with
    longdouble, the differences) carried wider, mean and scale rounded to
    double once; then the same float32 in-place transform and float64 norm."""
    x = np.asarray(train_lat, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    eps = np.finfo(np.float64).eps
    wide = np.longdouble if wide_sum_is_longdouble() else np.float64
    mean = _colsum(x) / wide(n)
    df = x.astype(wide) - mean
    corr = _colsum(df)
    var = (_colsum(df * df) - corr * corr / wide(n)) / wide(n)
    mean64, var64 = mean.astype(np.float64), var.astype(np.float64)
    upper = n * eps * var64 + (n * mean64 * eps) ** 2
    scale = np.sqrt(var).astype(np.float64)
    scale[var64 <= upper] = 1.0
    t = np.asarray(test_lat, dtype=np.float32).copy()
    t -= mean64
    t /= scale
    t64 = t.astype(np.float64)
    return np.sqrt(np.sum(t64 * t64, axis=1))


def cen_scaler(train_lat: np.ndarray) -> StandardScaler:
    return StandardScaler().fit(np.asarray(train_lat, dtype=np.float32))


# -- 6. forward -------------------------------------------------------------------------
# one below, at and above the compact order's special input columns 113 / 114,
# the first shape past each compact bound (d_in 115, hidden 27, latent 7)
FWD_NEW_SHAPES = [(112, 27, 7), (113, 27, 7), (114, 27, 7), (116, 27, 7), (115, 28, 7), (115, 27, 8)]
FWD_ROWS = (5, 40, 257, 15, 16, 17, 63, 64, 65)
FWD_TOL = (2e-5, 1e-5)


def fwd_rows(n: int, d_in: int, seed: int, garbage: bool = False) -> torch.Tensor:
    """fp32 [n, DP]: randn in the real columns; the rest zero, or with
    ``garbage`` finite noise in d_in..126 and 1 in column 127."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, DP)
    x[:, :d_in] = torch.randn(n, d_in, generator=g)
    if garbage:
        x[:, d_in:] = torch.randn(n, DP - d_in, generator=g) * 50.0
        x[:, DP - 1] = 1.0
    return x
