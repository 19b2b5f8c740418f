"""The scoring-chain kernels where their other code paths start, against the
plain references of ``tests/scoring_oracle.py`` (run with ``pytest -m gpu`` on
an MI355X).  ``tests/test_scoring_chain.py`` checks the references and inputs
themselves on the CPU.

Which case reaches which branch
-------------------------------
standardize_lds_kernel (STD_CHUNK = 256 rows per LDS tile, 8 row groups):
  n = 255, 256   one chunk, ``single``: the tile loaded in the sum pass is kept
                 (255: row group 7 has one row fewer than the others)
  n = 257        2 chunks, ``!single``: the last chunk is one row (rows * DP / 4 =
                 32 float4: threads 32..1023 load nothing, groups 1..7 add nothing),
                 reloaded in the variance pass and again in the output pass
  n = 511, 513   2 chunks of 256 + 255; 3 chunks of 256 + 256 + 1
  n = 512        2 full chunks, no partial one
  n = 1000       4 chunks, the last of 232 rows
  n = 1          the unbiased variance is 0 / 0: NaN in the real columns
score_reduce_block, single batch; a slice k floats past a 16-byte boundary has
head = (4 - k) & 3 floats (0, 3, 2, 1), n4 = (n - head) >> 2 float4 words and a
tail of n - head - 4 n4; the unrolled loop runs while i + 3072 < n4:
  n = 0          nb = 0: neither path, outputs (inf, nan)
  n = 1, 2, 3    k = 0: all tail; k = 1: all head (n <= 3 = head); n4 = 0
  n = 4, 7       one float4 for k = 0 (7: tail 3); for k = 1 head 3 + one float4 at n = 7
  n = 4095/4096  k = 0: n4 = 1023 / 1024: the remainder loop leaves thread 1023
                 idle / gives every thread one word
  n = 12287..12291  k = 0: n4 = 3071 / 3072 / 3072: three remainder passes, no unrolled one
  n = 12292      k = 0: n4 = 3073 > 3072: unrolled loop, one iteration for thread 0
                 only, then nothing left for it; k = 1: head 3, n4 = 3072: not entered
  n = 12293      k = 0: as 12292 with a tail of 1; k = 3: head 1, n4 = 3073: entered
  n = 16387      k = 0: n4 = 4096: every thread exactly one unrolled iteration, no
                 remainder, tail 3
  n = 53001      k = 0: n4 = 13250: three unrolled iterations for every thread
                 (i + 3072 < 13250 up to i = 9215), 962 words in the remainder, tail 1
batched path (nb > 1) at n = 3000: batch 1 (3000 batches of one row), 128 (24,
the last of 56), 1024 (one row per thread; last batch 952), 1025 (thread 0 takes
a second row: the ``r += 1024`` stride), 2999 (a last batch of one row); batch
3000 and 5000 give nb = 1 and take the single-batch path with batch > 0;
n = 129, batch 128: a last batch of one row.
score_reduce_copy_kernel: nfloats 4 (thread 0 alone), P_PAD = 9216 (2304 float4:
three passes, the last of 256 threads), 4100 (1025 float4: thread 0 twice).
broadcast_rows_kernel: P_PAD / 4 = 2304 float4 = 9 blocks of 256 exactly.
copy_f64 / copy2_f64 (256 threads a block): n = 255 / 256 / 257 around one block;
copy2's grid is sized by the longer pair, so (257, 3) has a second block in which
the short pair writes nothing, and (0, 5) a pair that writes nothing at all.
weighted_sum_kernel: P = 4 one thread, 1028 = 257 float4 (a second block of one
thread), P_PAD 9 blocks; K = 1 takes only the ``k == 0`` product.
cen_score_kernel (256 threads, gridDim.y = 8): n_test 2048 = one row per thread
of the 8 workgroups, 2047 leaves the last thread idle, 2049 gives thread 0 of
workgroup 0 a second row, 0 / 1 leave whole workgroups idle; n_train 255 / 257 one
row fewer / more than threads in the fit, 70001 = 273 passes + 113 rows, 1 / 2 the
zero-variance (scale 1) branch and the smallest real variance.
fwd_rows_kernel: d_in 112 / 113 / 114 at hidden 27, latent 7 take the compact order
(k-step (7, 0) carries x[112], x[113], x[114] and the bias): at 112 all three are
padding, at 113 x[112] is real and the two columns moved across lanes are padding,
at 114 x[113] is real and x[114] padding (115, both real, is the default shape);
116 / 27 / 7, 115 / 28 / 7 and 115 / 27 / 8 are the first shapes past each compact
bound (identity order).  Rows 15 / 16 / 17 and 63 / 64 / 65: a partial tile, a full
one, one row into the next, around one tile and one 64-row block.

Baseline for later tolerance changes: the largest fraction of
``atol + rtol * |ref|`` used on an MI355X (``oracle_f64.usage``; 1 would fail);
the tests print the same figures per case (``DIST`` lines, ``pytest -s``).

  kernel       cases                                   tolerance (rtol, atol)   largest use
  standardize  d_in 1,   n 255..1000                   1e-5, 1e-5               0.0064
  standardize  d_in 115, n 255..1000                   1e-5, 1e-5               0.0113
  standardize  d_in 127, n 255..1000                   1e-5, 1e-5               0.0114
  (fp32 TorchEngine on the CPU, same cases: at most 0.5 by test_scoring_chain.py)
  cen          latent 1, 7: all 25 size pairs, ill     1e-12, 1e-12             0 (equal)
  cen          latent 15: all 25 size pairs            1e-12, 1e-12             3.0e-04
  cen          latent 15: ill-conditioned train set    1e-12, 1e-12             2.9e-04
  forward      113/27/7   SSE / latents                2e-5, 1e-5               0.0077 / 0.0216
  forward      115/27/7   SSE / latents                2e-5, 1e-5               0.0080 / 0.0287
  forward      116/27/7   SSE / latents                2e-5, 1e-5               0.0088 / 0.0233
  forward      127/31/15  SSE / latents                2e-5, 1e-5               0.0088 / 0.0400
The score reduction, the copies and the weighted sum are compared bit for bit.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scoring_oracle as S  # noqa: E402
from oracle_f64 import usage  # noqa: E402
from fedmse_decentralized_amd.engine.base import batch_mean_scores  # noqa: E402
from fedmse_decentralized_amd.engine.torch_engine import cen_score_numpy  # noqa: E402
from fedmse_decentralized_amd.models.layout import DP, P_PAD, ModelDims, canonical_to_padded  # noqa: E402
from fedmse_decentralized_amd.models.reference import init_client_params, rowwise_sse  # noqa: E402
from fedmse_decentralized_amd.ops import _hip  # noqa: E402

DEV = torch.device("cuda", 0)
SENTINEL = -12345.5


def _sync():
    torch.cuda.synchronize()
    _hip.runtime(DEV).sync()


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# -- 1. standardize_lds_kernel -----------------------------------------------------
@pytest.mark.parametrize("n", S.STD_ROWS)
@pytest.mark.parametrize("d_in", S.STD_WIDTHS)
def test_standardize_multi_chunk(d_in, n):
    x = S.std_case(d_in, n)
    xd = x.to(DEV)
    fresh = _hip.standardize_ddof1(xd, d_in)
    into = torch.full((n, DP), float("nan"), device=DEV)
    assert _hip.standardize_ddof1(xd, d_in, out=into) is into
    _sync()
    ref = S.std_reference(x, d_in)
    print(f"DIST standardize d_in {d_in} n {n} use {usage(fresh[:, :d_in].cpu().numpy(), ref.numpy(), *S.STD_TOL):.4f}")
    for y in (fresh, into):
        y = y.cpu()
        torch.testing.assert_close(y[:, :d_in].double(), ref, rtol=S.STD_TOL[0], atol=S.STD_TOL[1])
        assert torch.count_nonzero(y[:, d_in:]) == 0 and not bool(torch.isnan(y[:, d_in:]).any())
    assert _same_bits(fresh, into)
    assert torch.equal(xd.cpu(), x)     # the input is only read
    if n == 1000:
        assert _same_bits(_hip.standardize_ddof1(xd, d_in), fresh)


def test_standardize_constant_column_is_exactly_zero():
    n, col = S.STD_CONST
    for d_in in S.STD_WIDTHS:
        x = S.std_case(d_in, n, const_col=col)
        y = _hip.standardize_ddof1(x.to(DEV), d_in).cpu()
        assert torch.count_nonzero(y[:, col]) == 0 and not bool(torch.isnan(y[:, col]).any())
        if d_in > 1:
            ref = S.std_reference(x, d_in)
            torch.testing.assert_close(y[:, 1:d_in].double(), ref[:, 1:], rtol=S.STD_TOL[0], atol=S.STD_TOL[1])
        assert torch.count_nonzero(y[:, d_in:]) == 0


@pytest.mark.parametrize("d_in", S.STD_WIDTHS)
def test_standardize_one_row_is_nan_as_the_reference(d_in):
    """``torch.std`` over one row is NaN, so the reference's standardised row
    is: the kernel answers the same (it used to divide by max(n - 1, 1) and
    return zeros), padding still 0."""
    x = S.std_case(d_in, 255)[:1].clone()
    y = _hip.standardize_ddof1(x.to(DEV), d_in).cpu()
    assert bool(torch.isnan(y[:, :d_in]).all())
    assert torch.count_nonzero(y[:, d_in:]) == 0 and not bool(torch.isnan(y[:, d_in:]).any())


# -- 2. score_reduce / score_reduce_copy ---------------------------------------------
def _reduce(segs, batches, d_in=S.REDUCE_D_IN) -> np.ndarray:
    red = _hip.score_reduce(segs, batches, d_in)
    _sync()
    return np.array(red)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_score_reduce_single_batch_every_misalignment(k):
    """Slices base[k : k + n] of one 16-byte-aligned tensor: exact inputs, so
    both outputs equal batch_mean_scores bit for bit whatever the order."""
    base = S.exact_sse(max(S.REDUCE_SINGLE) + 4).to(DEV)
    assert base.data_ptr() % 16 == 0
    segs = [base[k:k + n] for n in S.REDUCE_SINGLE]
    assert all((s.data_ptr() >> 2) & 3 == k for s in segs if s.numel())   # (an empty slice has no address)
    got = _reduce(segs, [0] * len(segs))
    for n, s, g in zip(S.REDUCE_SINGLE, segs, got):
        want = batch_mean_scores(s, 1 << 30, S.REDUCE_D_IN)
        if n == 0:
            assert g[0] == float("inf") and np.isnan(g[1]), g
            assert want[0] == float("inf") and np.isnan(want[1])
            continue
        assert g[0] == want[0] and g[1] == want[1] and g[0] == g[1], (n, k, g, want, S.reduce_path(n, k))
        assert g[1] == S.fsum_scores(s.cpu().numpy(), S.REDUCE_D_IN), (n, k)


def test_score_reduce_batched():
    base = S.exact_sse(3000).to(DEV)
    segs = [base[:n] for n, _ in S.REDUCE_BATCHED]
    batches = [b for _, b in S.REDUCE_BATCHED]
    got = _reduce(segs, batches)
    for (n, b), s, g in zip(S.REDUCE_BATCHED, segs, got):
        want = batch_mean_scores(s, b, S.REDUCE_D_IN)
        assert g[0] == want[0] and g[1] == want[1], (n, b, g, want)
    # the vote score really depends on the batching: a wrong batch length shows
    votes = {float(g[0]) for (n, b), g in zip(S.REDUCE_BATCHED, got) if n == 3000}
    assert len(votes) >= 5


def test_score_reduce_random_values_against_fsum():
    """randn^2 at the 80-client dev-set size: no order is exact any more; a
    sum of n non-negative doubles is within n u = n 2^-53 of the true one,
    relatively.  rtol n 2^-52, twice that."""
    n = 53001
    g = torch.Generator().manual_seed(53)
    x = (torch.randn(n + 3, generator=g) ** 2).to(DEV)
    segs = [x[k:k + n] for k in range(4)]
    got = _reduce(segs, [0] * 4)
    for s, gk in zip(segs, got):
        want = S.fsum_scores(s.cpu().numpy(), S.REDUCE_D_IN)
        np.testing.assert_allclose(gk, [want, want], rtol=n * 2.0 ** -52, atol=0)


def test_score_reduce_to_with_copies():
    """Three reductions and three row copies in one launch: the reductions as
    in a launch without copies, every destination equal to its source, the
    guard floats around it untouched."""
    base = S.exact_sse(16387).to(DEV)
    segs, batches = [base[:12293], base[1:3001], base[:129]], [0, 128, 128]
    alone = torch.full((3, 2), -1.0, dtype=torch.float64, device=DEV)
    both = torch.full((3, 2), -1.0, dtype=torch.float64, device=DEV)
    _hip.score_reduce_to(segs, batches, S.REDUCE_D_IN, [alone.data_ptr() + 16 * i for i in range(3)])
    g = torch.Generator().manual_seed(5)
    sizes = [4, P_PAD, 4100]
    srcs = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    dsts = [torch.full((64 + n + 64,), SENTINEL, device=DEV) for n in sizes]
    copies = [(s.data_ptr(), d.data_ptr() + 4 * 64, n) for s, d, n in zip(srcs, dsts, sizes)]
    assert all(c[0] % 16 == 0 and c[1] % 16 == 0 for c in copies)
    _hip.score_reduce_to(segs, batches, S.REDUCE_D_IN, [both.data_ptr() + 16 * i for i in range(3)], copies=copies)
    _sync()
    assert _same_bits(alone, both)
    for s, b, row in zip(segs, batches, both.cpu().numpy()):
        assert tuple(row) == batch_mean_scores(s, b or (1 << 30), S.REDUCE_D_IN)
    for s, d, n in zip(srcs, dsts, sizes):
        assert _same_bits(d[64:64 + n], s), n
        assert bool((d[:64] == SENTINEL).all()) and bool((d[64 + n:] == SENTINEL).all()), n
    with pytest.raises(ValueError):
        _hip.score_reduce_to(segs, batches, S.REDUCE_D_IN, [both.data_ptr()] * 3, copies=[(copies[0][0], copies[0][1], 6)])


# -- 3. copies and adoption -------------------------------------------------------------
@pytest.mark.parametrize("with_dst1", [True, False])
@pytest.mark.parametrize("rows", [[4, 1], [3], [5, 4, 3, 2, 1, 0]], ids=lambda r: "-".join(map(str, r)))
def test_broadcast_rows(rows, with_dst1):
    g = torch.Generator().manual_seed(11)
    src = torch.randn(P_PAD, generator=g).to(DEV)
    # one allocation per destination with a guard row on each side
    bufs = [torch.full((8, P_PAD), SENTINEL, device=DEV) for _ in range(2)]
    dst0, dst1 = bufs[0][1:7], bufs[1][1:7]
    _hip.broadcast_rows(dst0, dst1 if with_dst1 else None, rows, src)
    _sync()
    for i, buf in enumerate(bufs):
        written = i == 0 or with_dst1
        for r in range(8):
            if written and (r - 1) in rows:
                assert _same_bits(buf[r], src), (i, r)
            else:
                assert bool((buf[r] == SENTINEL).all()), (i, r)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_copy_f64(n):
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, dtype=torch.float64, generator=g).to(DEV)
    buf = torch.full((16 + n + 16,), SENTINEL, dtype=torch.float64, device=DEV)
    _hip.copy_f64(buf.data_ptr() + 8 * 16, src.data_ptr(), n, DEV)
    _sync()
    assert _same_bits(buf[16:16 + n], src)
    assert bool((buf[:16] == SENTINEL).all()) and bool((buf[16 + n:] == SENTINEL).all())


@pytest.mark.parametrize("n0,n1", [(0, 5), (5, 0), (257, 3), (3, 257), (256, 256)])
def test_copy2_f64(n0, n1):
    g = torch.Generator().manual_seed(1000 * n0 + n1)
    srcs = [torch.randn(max(n, 1), dtype=torch.float64, generator=g).to(DEV) for n in (n0, n1)]
    bufs = [torch.full((16 + n + 16,), SENTINEL, dtype=torch.float64, device=DEV) for n in (n0, n1)]
    _hip.copy2_f64(bufs[0].data_ptr() + 8 * 16, srcs[0].data_ptr(), n0,
                   bufs[1].data_ptr() + 8 * 16, srcs[1].data_ptr(), n1, DEV)
    _sync()
    for n, s, b in zip((n0, n1), srcs, bufs):
        assert _same_bits(b[16:16 + n], s[:n])
        assert bool((b[:16] == SENTINEL).all()) and bool((b[16 + n:] == SENTINEL).all())   # n = 0: the whole buffer


# -- 4. weighted_sum ------------------------------------------------------------------------
@pytest.mark.parametrize("P", S.WSUM_P + [P_PAD])
@pytest.mark.parametrize("K", S.WSUM_K)
def test_weighted_sum_is_the_sequential_fp32_formula(K, P):
    """Bit-equal to product-then-sum, each rounded to fp32, in row order; NaN
    (inf under a zero weight), inf (an overflowing product) and subnormal
    products exactly as the formula gives them — and not what a fused
    multiply-add would give (test_scoring_chain.py: the two differ on these
    inputs for K >= 2)."""
    stack, w = S.wsum_case(K, P)
    out = torch.full((P,), SENTINEL, device=DEV)
    got = _hip.weighted_sum(stack.to(DEV), w, out=out)
    fresh = _hip.weighted_sum(stack.to(DEV), w)
    _sync()
    seq = S.wsum_sequential(stack, w)
    assert got is out and S.same_floats(got, seq) and S.same_floats(fresh, seq)
    if K >= 2:
        assert not S.same_floats(got, S.wsum_fused(stack, w))


# -- 5. CEN -------------------------------------------------------------------------------------
@pytest.mark.parametrize("latent", S.CEN_LATENT)
def test_cen_scores_sizes(latent):
    """Every train size against every test size in one launch (25 items)."""
    pairs = [(a, b) for a in S.CEN_TRAIN for b in S.CEN_TEST]
    trd = {a: torch.from_numpy(S.cen_train(a, latent)).to(DEV) for a in S.CEN_TRAIN}
    ted = {b: torch.from_numpy(S.cen_test(b, latent)).to(DEV) for b in S.CEN_TEST}
    out = _hip.cen_scores([trd[a] for a, _ in pairs], [ted[b] for _, b in pairs], latent)
    _sync()
    worst = 0.0
    for (a, b), o in zip(pairs, out):
        want = cen_score_numpy(S.cen_train(a, latent), S.cen_test(b, latent))
        assert o.shape == (b,) and o.dtype == torch.float64
        worst = max(worst, usage(o.cpu().numpy(), want, *S.CEN_TOL))
    print(f"DIST cen latent {latent} sizes use {worst:.2e}")
    for (a, b), o in zip(pairs, out):
        want = cen_score_numpy(S.cen_train(a, latent), S.cen_test(b, latent))
        np.testing.assert_allclose(o.cpu().numpy(), want, rtol=S.CEN_TOL[0], atol=S.CEN_TOL[1], err_msg=f"{a} x {b}")


@pytest.mark.parametrize("latent", S.CEN_LATENT)
def test_cen_scores_ill_conditioned_train_set(latent):
    """Mean 1e3, deviation 1e-2, one constant column: the corrected two-pass
    variance and the near-constant rule."""
    tr, te = S.cen_ill(latent)
    out = _hip.cen_scores([torch.from_numpy(tr).to(DEV)], [torch.from_numpy(te).to(DEV)], latent)[0]
    _sync()
    want = cen_score_numpy(tr, te)
    print(f"DIST cen latent {latent} ill use {usage(out.cpu().numpy(), want, *S.CEN_TOL):.2e}")
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=S.CEN_TOL[0], atol=S.CEN_TOL[1])


@pytest.mark.parametrize("latent", S.CEN_LATENT)
def test_cen_scores_equal_stride_views_of_wider_buffers(latent):
    """Train and test latents as column slices (row stride 24) of buffers
    whose other columns hold garbage; a pair with unequal strides is refused."""
    rng = np.random.default_rng(77)
    tr, te = S.cen_train(257, latent), S.cen_test(2049, latent)
    wtr = (rng.normal(size=(257, 24)) * 1e6).astype(np.float32)
    wte = (rng.normal(size=(2049, 24)) * 1e6).astype(np.float32)
    wtr[:, 3:3 + latent], wte[:, 5:5 + latent] = tr, te
    dtr, dte = torch.from_numpy(wtr).to(DEV), torch.from_numpy(wte).to(DEV)
    out = _hip.cen_scores([dtr[:, 3:3 + latent]], [dte[:, 5:5 + latent]], latent)[0]
    _sync()
    np.testing.assert_allclose(out.cpu().numpy(), cen_score_numpy(tr, te), rtol=S.CEN_TOL[0], atol=S.CEN_TOL[1])
    with pytest.raises(ValueError):
        _hip.cen_scores([torch.from_numpy(tr).to(DEV)], [dte[:, 5:5 + latent]], latent)


# -- 6. fwd_rows_kernel -----------------------------------------------------------------------------
def _model(dims, n_models=2, seed=11):
    md = ModelDims(*dims)
    params, _ = init_client_params(n_models, seed, md)
    params = params + 0.05 * torch.randn(params.shape, generator=torch.Generator().manual_seed(3))
    return md, params, canonical_to_padded(params, md).to(DEV)


MODE_SHAPES = [(113, 27, 7), (115, 27, 7), (116, 27, 7), (127, 31, 15)]


@pytest.mark.parametrize("dims", MODE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_output_modes_agree_bitwise(dims):
    """SSE only, latents only and both: the same bits on the same items; and
    within the forward tolerances of the fp64 reference (DIST figures)."""
    md, params, pad = _model(dims)
    xs = [S.fwd_rows(n, md.d_in, 40 + n).to(DEV) for n in (17, 64, 65, 257)]
    items = [(i % 2, x) for i, x in enumerate(xs)]
    sse_b, lat_b = _hip.forward_rows(pad, items, md, True, True)
    sse_s, none_l = _hip.forward_rows(pad, items, md, True, False)
    none_s, lat_l = _hip.forward_rows(pad, items, md, False, True)
    _sync()
    assert none_l == [] and none_s == []
    use_s = use_z = 0.0
    for (row, x), sb, zb, ss, zl in zip(items, sse_b, lat_b, sse_s, lat_l):
        assert _same_bits(sb, ss) and _same_bits(zb, zl)
        rs, rz = rowwise_sse(params[row].double(), x[:, :md.d_in].cpu().double(), md)
        use_s = max(use_s, usage(sb.cpu().numpy(), rs.numpy(), *S.FWD_TOL))
        use_z = max(use_z, usage(zb.cpu().numpy(), rz.numpy(), *S.FWD_TOL))
        torch.testing.assert_close(sb.cpu().double(), rs, rtol=S.FWD_TOL[0], atol=S.FWD_TOL[1])
        torch.testing.assert_close(zb.cpu().double(), rz, rtol=S.FWD_TOL[0], atol=S.FWD_TOL[1])
    print(f"DIST forward {dims} sse use {use_s:.4f} latent use {use_z:.4f}")


@pytest.mark.parametrize("dims", [(113, 27, 7), (46, 27, 7), (116, 27, 7), (120, 30, 10)],
                         ids=lambda s: "x".join(map(str, s)))
def test_forward_ignores_padded_input_columns(dims):
    """Finite garbage in x columns d_in..126 and 1 in column 127 (the stores'
    bias column) change no bit: compact shapes (113: x[113] / x[114] are
    padding the cross-lane move still carries) and general ones."""
    md, _, pad = _model(dims)
    for n in (17, 65):
        clean, dirty = S.fwd_rows(n, md.d_in, 7 * n), S.fwd_rows(n, md.d_in, 7 * n, garbage=True)
        a_s, a_z = _hip.forward_rows(pad, [(0, clean.to(DEV))], md, True, True)
        b_s, b_z = _hip.forward_rows(pad, [(0, dirty.to(DEV))], md, True, True)
        _sync()
        assert _same_bits(a_s[0], b_s[0]) and _same_bits(a_z[0], b_z[0]), (dims, n)


@pytest.mark.parametrize("nrows", [17, 33])
@pytest.mark.parametrize("dims", [(115, 27, 7), (115, 28, 7)], ids=lambda s: "x".join(map(str, s)))
def test_forward_non_finite_rows_stay_in_their_rows(dims, nrows):
    """Row 0 all NaN (the row a partial tile's padding rows re-read) and an inf
    in another row: exactly those rows' SSEs are non-finite, every other row
    has the bits of a run where the two rows hold ordinary values."""
    md, _, pad = _model(dims)
    plain = S.fwd_rows(nrows, md.d_in, 90 + nrows)
    hurt = plain.clone()
    other = nrows - 2
    hurt[0, :] = float("nan")
    hurt[other, 5] = float("inf")
    a_s, a_z = _hip.forward_rows(pad, [(1, plain.to(DEV))], md, True, True)
    b_s, b_z = _hip.forward_rows(pad, [(1, hurt.to(DEV))], md, True, True)
    _sync()
    a_s, a_z, b_s, b_z = a_s[0].cpu(), a_z[0].cpu(), b_s[0].cpu(), b_z[0].cpu()
    assert bool(torch.isfinite(a_s).all())
    bad = ~torch.isfinite(b_s)
    assert torch.nonzero(bad).flatten().tolist() == [0, other]
    assert _same_bits(a_s[~bad], b_s[~bad]) and _same_bits(a_z[~bad], b_z[~bad])


@pytest.mark.parametrize("dims", [(115, 27, 7), (115, 27, 8)], ids=lambda s: "x".join(map(str, s)))
def test_forward_filler_descriptors_write_nothing(dims):
    """Fillers (nrows 0) between live blocks, their sse / lat pointers aimed
    at a sentinel buffer: it stays as it was, and the live outputs equal the
    launch without fillers."""
    md, _, pad = _model(dims)
    rt = _hip.runtime(DEV)
    xs = [S.fwd_rows(n, md.d_in, 60 + n).to(DEV) for n in (130, 65)]
    sizes = np.array([130, 65])
    pptr = pad.data_ptr() + 4 * P_PAD * np.array([0, 1], dtype=np.int64)
    xptr = np.array([x.data_ptr() for x in xs], dtype=np.int64)

    def launch(with_fillers: bool):
        sse = torch.full((195,), SENTINEL, device=DEV)
        lat = torch.full((195, md.latent), SENTINEL, device=DEV)
        offs = np.array([0, 130], dtype=np.int64)
        desc = _hip.build_fwd_desc(pptr, xptr, sizes, sse.data_ptr() + 4 * offs,
                                   lat.data_ptr() + 4 * md.latent * offs, md, rows_per_block=64)
        assert len(desc) == 5 and desc["nrows"].tolist() == [64, 64, 2, 64, 1]
        if with_fillers:
            filler = np.zeros(1, dtype=_hip.FWD_DTYPE)
            filler["params"], filler["x"] = pptr[0], xptr[0]
            filler["sse"], filler["lat"] = guard.data_ptr(), guard.data_ptr()
            filler["lat_stride"], filler["d_in"], filler["latent"], filler["hidden"] = (md.latent, md.d_in, md.latent,
                                                                                    md.hidden)
            desc = np.concatenate([filler, desc[:1], filler, filler, desc[1:4], filler, desc[4:], filler])
            assert (desc["nrows"] == 0).sum() == 5
        (dptr,) = rt.desc.put(desc)
        _hip._check(_hip.lib().fedmx_forward_rows(dptr, len(desc), rt.stream), "fedmx_forward_rows")
        _sync()
        return sse.cpu(), lat.cpu()

    guard = torch.full((64 * 16,), SENTINEL, device=DEV)
    s0, z0 = launch(False)
    s1, z1 = launch(True)
    assert bool((guard == SENTINEL).all())
    assert _same_bits(s0, s1) and _same_bits(z0, z1)
    assert bool((s0 != SENTINEL).all()) and bool((z0 != SENTINEL).all())
