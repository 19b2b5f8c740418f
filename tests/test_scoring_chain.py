"""CPU side of the scoring-chain tests (``tests/scoring_oracle.py``): what has
to hold for the GPU tests of ``test_scoring_chain_gpu.py`` to be fair, and
the parts of the chain that need no device.

* the exact score-reduction inputs really sum to one double in any order,
  and the sizes really reach the branches they are named for;
* the fp32 ``TorchEngine.standardize_ddof1`` alone uses at most half of the
  standardisation tolerance on every case, so the other half is the kernel's;
  both engines' contract for a single row (NaN, the reference's answer);
* the weighted-sum inputs can tell a fused multiply-add from the reference's
  separately rounded product and sum;
* ``cen_score_numpy`` agrees with the same fit carried in wider arithmetic on
  the ill-conditioned train set, at the tolerance the kernel is held to;
* ``_hip.cen_desc`` refuses latents it would misread (it reads pointers and
  strides only, so this needs neither a device nor the library).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scoring_oracle as S  # noqa: E402
from oracle_f64 import usage  # noqa: E402
from fedmse_decentralized_amd.engine.base import batch_mean_scores  # noqa: E402
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine, cen_score_numpy  # noqa: E402
from fedmse_decentralized_amd.models.layout import DP, P_PAD, ModelDims  # noqa: E402
from fedmse_decentralized_amd.ops import _hip  # noqa: E402


# -- 1. standardisation ---------------------------------------------------------
@pytest.mark.parametrize("d_in", S.STD_WIDTHS)
def test_fp32_standardisation_uses_at_most_half_the_tolerance(d_in):
    eng = TorchEngine(ModelDims(d_in, 27, 7), torch.device("cpu"))
    for n in S.STD_ROWS:
        x = S.std_case(d_in, n)
        assert torch.isfinite(x).all() and bool((x[:, DP - 1] == 1).all())
        y = eng.standardize_ddof1(x)
        use = usage(y[:, :d_in].numpy(), S.std_reference(x, d_in).numpy(), *S.STD_TOL)
        assert use <= 0.5, (d_in, n, use)
        assert torch.count_nonzero(y[:, d_in:]) == 0
    assert all(n > S.STD_CHUNK for n in S.STD_ROWS[2:]) and S.STD_ROWS[:2] == [S.STD_CHUNK - 1, S.STD_CHUNK]


def test_standardisation_of_one_row_is_nan_as_torch_std():
    """The reference standardises with ``torch.std`` (ddof 1), which is NaN
    over one row; TorchEngine follows it and the kernel now does too."""
    for d_in in S.STD_WIDTHS:
        x = S.std_case(d_in, 255)[:1].clone()
        assert bool(torch.isnan(x[:, :d_in].std(0)).all())
        y = TorchEngine(ModelDims(d_in, 27, 7), torch.device("cpu")).standardize_ddof1(x)
        assert bool(torch.isnan(y[:, :d_in]).all())
        assert torch.count_nonzero(y[:, d_in:]) == 0


def test_constant_column_reference_is_zero():
    n, col = S.STD_CONST
    x = S.std_case(115, n, const_col=col)
    assert bool((x[:, col] == x[0, col]).all())
    assert torch.count_nonzero(S.std_reference(x, 115)[:, col]) == 0


# -- 2. score reduction -----------------------------------------------------------
def test_exact_sse_sums_to_one_double_in_any_order():
    n = max(S.REDUCE_SINGLE) + 3
    x = S.exact_sse(n).double().numpy()
    assert len(np.unique(x)) == n and x.max() < 1024 and np.array_equal(x * 1024, np.round(x * 1024))
    want = math.fsum(x.tolist())
    rng = np.random.default_rng(0)
    for _ in range(3):
        p = rng.permutation(n)
        assert float(np.sum(x[p])) == want                 # numpy's pairwise order
        assert float(np.cumsum(x[p])[-1]) == want          # strictly sequential
        assert sum(float(np.sum(c)) for c in np.array_split(x[p], 1024)) == want
    # so batch_mean_scores (numpy sums) is the exactly rounded answer
    vote, mse = batch_mean_scores(torch.from_numpy(x[:53001]), 1 << 30, S.REDUCE_D_IN)
    assert vote == mse == want_of(x[:53001])


def want_of(x):
    return S.fsum_scores(x, S.REDUCE_D_IN)


def test_reduce_sizes_reach_their_branches():
    P = S.reduce_path
    assert S.REDUCE_SINGLE == [0, 1, 2, 3, 4, 7, 4095, 4096, 12287, 12288, 12291, 12292, 12293, 16387, 53001]
    # heads 0, 3, 2, 1 for k = 0..3; n below the head is all head
    assert [P(7, k)["head"] for k in range(4)] == [0, 3, 2, 1]
    assert P(1, 1) == {"head": 1, "n4": 0, "unrolled_max": 0, "unrolled_min": 0, "remainder": 0, "tail": 0}
    assert P(3, 0)["tail"] == 3 and P(4, 0)["n4"] == 1 and P(7, 0)["tail"] == 3
    # remainder loop: 1023 float4 leave thread 1023 idle, 1024 give every thread one
    assert P(4095, 0)["n4"] == 1023 and P(4096, 0)["n4"] == 1024
    # the unrolled loop starts at n4 = 3073
    assert P(12288, 0)["n4"] == 3072 and P(12288, 0)["unrolled_max"] == 0
    assert P(12291, 0)["n4"] == 3072 and P(12291, 0)["unrolled_max"] == 0 and P(12291, 0)["tail"] == 3
    assert P(12292, 0)["n4"] == 3073 and (P(12292, 0)["unrolled_max"], P(12292, 0)["unrolled_min"]) == (1, 0)
    assert P(12292, 1)["n4"] == 3072 and P(12292, 1)["unrolled_max"] == 0     # the head takes it back out
    assert P(12293, 3)["n4"] == 3073 and P(12293, 3)["unrolled_max"] == 1
    assert P(12293, 0)["tail"] == 1
    # every thread one unrolled pass and nothing left; three passes and a partial remainder
    assert P(16387, 0) == {"head": 0, "n4": 4096, "unrolled_max": 1, "unrolled_min": 1, "remainder": 0, "tail": 3}
    assert P(53001, 0) == {"head": 0, "n4": 13250, "unrolled_max": 3, "unrolled_min": 3, "remainder": 962, "tail": 1}
    for n in S.REDUCE_SINGLE:
        for k in range(4):
            p = P(n, k)
            assert p["head"] + 4 * p["n4"] + p["tail"] == n and 0 <= p["tail"] < 4
    # batched: a stride past 1024 rows, a last batch of one row, batches at and beyond n
    assert (3000, 1025) in S.REDUCE_BATCHED and 3000 % 2999 == 1 and 129 % 128 == 1
    assert {(3000, 3000), (3000, 5000)} <= set(S.REDUCE_BATCHED)


def test_batch_mean_scores_of_nothing():
    v, m = batch_mean_scores(torch.zeros(0), 128, S.REDUCE_D_IN)
    assert v == float("inf") and math.isnan(m)


# -- 4. weighted sum ----------------------------------------------------------------
@pytest.mark.parametrize("P", S.WSUM_P + [P_PAD])
@pytest.mark.parametrize("K", S.WSUM_K)
def test_weighted_sum_inputs_tell_fma_from_separate_rounding(K, P):
    stack, w = S.wsum_case(K, P)
    seq, fused = S.wsum_sequential(stack, w), S.wsum_fused(stack, w)
    assert seq.dtype == torch.float32 and seq.shape == (P,)
    if K == 1:
        # one product, no sum: nothing to fuse; the products are subnormal
        assert S.same_floats(seq, fused)
        assert bool((seq.abs() < np.finfo(np.float32).tiny).all()) and torch.count_nonzero(seq) > 0
        return
    assert not S.same_floats(seq, fused)
    if K >= 9:
        assert w[1] == 0.0 and w[2] < 0 and 0 < np.float32(w[3]) < np.finfo(np.float32).tiny
        assert math.isnan(float(seq[0])) and math.isinf(float(seq[1]))       # inf x 0; the overflowing product
        assert 0 < float(seq[2]) < np.finfo(np.float32).tiny                  # the subnormal product survives
        assert bool(torch.isfinite(seq[3:]).all())


# -- 5. CEN -----------------------------------------------------------------------------
@pytest.mark.parametrize("latent", S.CEN_LATENT)
def test_cen_oracle_agrees_with_a_wider_fit_on_the_ill_conditioned_set(latent):
    tr, te = S.cen_ill(latent)
    col = tr[:, 0].astype(np.float64)
    assert abs(col.mean() - S.CEN_ILL_MEAN) < 1e-3 and abs(col.std() / S.CEN_ILL_STD - 1) < 0.05
    sc = S.cen_scaler(tr)
    if latent > 1:
        assert sc.scale_[latent - 1] == 1.0          # the constant column: the near-constant rule
    assert 0.9 * S.CEN_ILL_STD < sc.scale_[0] < 1.1 * S.CEN_ILL_STD
    got, want = cen_score_numpy(tr, te), S.cen_score_wide(tr, te)
    assert usage(got, want, *S.CEN_TOL) <= 1.0, usage(got, want, *S.CEN_TOL)
    np.testing.assert_allclose(got, want, rtol=S.CEN_TOL[0], atol=S.CEN_TOL[1])


def test_cen_oracle_agrees_with_a_wider_fit_on_regular_sets():
    for n in (2, 257, 70001):
        tr, te = S.cen_train(n, 7), S.cen_test(2049, 7)
        np.testing.assert_allclose(cen_score_numpy(tr, te), S.cen_score_wide(tr, te), rtol=S.CEN_TOL[0],
                                   atol=S.CEN_TOL[1])


def _launch_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("cen_desc touched the library")

    monkeypatch.setattr(_hip, "lib", boom)
    monkeypatch.setattr(_hip, "runtime", boom)


def test_cen_desc_refuses_latents_it_would_misread(monkeypatch):
    _launch_nothing(monkeypatch)
    out = torch.zeros(64, dtype=torch.float64)
    wide = torch.zeros(20, 24)
    tr, te = torch.zeros(20, 7), torch.zeros(9, 7)
    desc, views = _hip.cen_desc([tr], [te], out, 7)                    # the plain case still works
    assert int(desc[0]["stride"]) == 7 and int(desc[0]["n_train"]) == 20 and views[0].shape == (9,)
    bad = [
        ([tr], [wide[:9, 3:10]]),                   # row strides 7 and 24
        ([wide[:, :7]], [te]),                      # 24 and 7
        ([wide[:, 0:14:2]], [wide[:9, 0:14:2]]),    # column stride 2, both
        ([tr], [torch.zeros(7, 9).t()]),            # column stride 9 in the test set only
        ([torch.zeros(20, 6)], [torch.zeros(9, 6)]),   # fewer than latent columns, both
        ([tr], [torch.zeros(9, 6)]),                # ... the test set only
        ([tr.double()], [te]),                      # not float32
        ([tr, tr], [te]),                           # a train set without a test set
    ]
    for trl, tel in bad:
        with pytest.raises(ValueError):
            _hip.cen_desc(trl, tel, out, 7)


def test_cen_desc_takes_equal_stride_views(monkeypatch):
    _launch_nothing(monkeypatch)
    out = torch.zeros(64, dtype=torch.float64)
    a, b = torch.zeros(20, 24), torch.zeros(9, 24)
    desc, views = _hip.cen_desc([a[:, 3:10], a[:, :7]], [b[:, 5:12], b[:0, :7]], out, 7)
    assert [int(s) for s in desc["stride"]] == [24, 24]
    assert int(desc[0]["train_lat"]) == a.data_ptr() + 12 and int(desc[0]["test_lat"]) == b.data_ptr() + 20
    assert [v.shape[0] for v in views] == [9, 0]
    assert int(desc[1]["out"]) == out.data_ptr() + 8 * 9
    # a set of at most one row is read at its first row only: its row stride is not applied, the other's is
    desc, _ = _hip.cen_desc([a[:1, 3:10], torch.zeros(20, 7)], [torch.zeros(9, 7), b[:1, 5:12]], out, 7)
    assert [int(s) for s in desc["stride"]] == [7, 7]
    desc, _ = _hip.cen_desc([torch.zeros(1, 7)], [torch.from_numpy(np.zeros((0, 7), np.float32))], out, 7)
    assert int(desc[0]["n_test"]) == 0
    # one real column: the column stride of a one-column view is immaterial
    desc, _ = _hip.cen_desc([a[:, 4:5]], [b[:, 2:3]], out, 1)
    assert int(desc[0]["stride"]) == 24


# -- 6. forward ---------------------------------------------------------------------------
def test_forward_shapes_sit_on_the_compact_bounds():
    compact = [s for s in S.FWD_NEW_SHAPES if s[0] <= 115 and s[1] <= 27 and s[2] <= 7]
    assert compact == [(112, 27, 7), (113, 27, 7), (114, 27, 7)]
    assert [s for s in S.FWD_NEW_SHAPES if s not in compact] == [(116, 27, 7), (115, 28, 7), (115, 27, 8)]
    for s in S.FWD_NEW_SHAPES:
        ModelDims(*s)
    # partial 16-row tiles on both sides of one tile and of one 64-row block
    assert {15, 16, 17, 63, 64, 65} <= set(S.FWD_ROWS) and {5, 40, 257} <= set(S.FWD_ROWS)
    x = S.fwd_rows(17, 113, 1, garbage=True)
    assert torch.isfinite(x).all() and bool((x[:, DP - 1] == 1).all()) and torch.count_nonzero(x[:, 113:127]) > 0
    assert torch.equal(x[:, :113], S.fwd_rows(17, 113, 1)[:, :113])
