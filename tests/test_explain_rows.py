"""Explaining alarms on the CPU (README "Explaining an alarm"): the selection
rule on hand-built residual rows, ``explain_rows_numpy`` against a literal
per-row Python loop, ``TorchEngine.explain_rows`` (subsets, repeats, nothing to
explain, bad arguments), the ties to ``score_rows`` (an autoencoder's score
from ``sse``, a CEN score from ``latent_terms``, both to the bit),
``expected_raw`` as the inverse of ``standardise``, and ``detect --explain``."""
import math

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.deploy.detector import (EXPLAIN_MAX_K, Detector, Explanation, _ae_scores, check_which,
                                                      expected_raw, explain_rows_numpy, select_top_k)
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
from fedmse_decentralized_amd.models.layout import ModelDims
from fedmse_decentralized_amd.models.reference import functional_forward, unflatten

DIMS = ModelDims(5, 3, 2)
KINDS = [("autoencoder", None), ("hybrid", "cen"), ("hybrid", "knn")]


def make_detector(model_type="autoencoder", scaler="standard", scorer=None, dims=DIMS, seed=0, threshold=0.75):
    rng = np.random.default_rng(seed)
    D, Z = dims.d_in, dims.latent
    if scaler == "standard":
        sc = {"mean_": rng.normal(size=D), "scale_": rng.uniform(0.5, 2.0, size=D)}
    else:
        sc = {"scale_": rng.uniform(0.5, 2.0, size=D), "min_": rng.normal(size=D)}
    kw = {}
    if model_type == "hybrid":
        kw = dict(latent_scorer=scorer, latent_mean=rng.normal(size=Z), latent_scale=rng.uniform(0.5, 2.0, size=Z))
        if scorer == "knn":
            kw.update(knn_k=3, train_latents=rng.normal(size=(9, Z)).astype(np.float32))
    return Detector(dims=dims, model_type=model_type, params=(0.3 * rng.normal(size=dims.num_params)).astype(np.float32),
                    scaler_kind=scaler, scaler=sc, threshold=threshold, detect_quantile=0.9, **kw)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def engine(dims=DIMS):
    return TorchEngine(dims, torch.device("cpu"))


# ---------------------------------------------------------------------------
# the selection rule
# ---------------------------------------------------------------------------
def test_selection_orders_by_squared_residual_ties_to_the_lower_index():
    r = np.array([[1.0, -3.0, 2.0, 3.0, -0.5, 0.0],      # |-3| == |3|: feature 1 before 3
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)   # all equal: 0, 1, 2
    idx, top = select_top_k(r, 3)
    assert idx.dtype == np.int32 and top.dtype == np.float32
    assert idx.tolist() == [[1, 3, 2], [0, 1, 2]]
    assert top.tolist() == [[-3.0, 3.0, 2.0], [0.0, 0.0, 0.0]]


def test_selection_puts_nan_first_and_inf_next():
    big = np.float32(3e38)   # squares to +inf in fp32: ties with the infinite residual, both behind no NaN
    r = np.array([[1.0, big, np.nan, -np.inf, np.nan, 2.0]], np.float32)
    idx, top = select_top_k(r, 6)
    # NaN ranks as +inf, so NaN, the overflowed square and the infinity tie: ascending feature
    assert idx.tolist() == [[1, 2, 3, 4, 5, 0]]
    assert np.isnan(top[0, 1]) and np.isnan(top[0, 3]) and top[0, 0] == big and top[0, 2] == -np.inf
    assert top[0, 4] == 2.0 and top[0, 5] == 1.0
    r = np.array([[1.0, 5.0, np.nan, 2.0]], np.float32)
    assert select_top_k(r, 2)[0].tolist() == [[2, 1]]


def test_selection_pads_past_the_feature_count_and_checks_k():
    r = np.array([[0.5, -2.0, 1.0]], np.float32)
    idx, top = select_top_k(r, EXPLAIN_MAX_K)
    assert idx.shape == (1, 16) and idx[0, :3].tolist() == [1, 2, 0] and np.all(idx[0, 3:] == -1)
    assert top[0, :3].tolist() == [-2.0, 1.0, 0.5] and np.all(top[0, 3:] == 0.0)
    idx, top = select_top_k(r, 1)
    assert idx.tolist() == [[1]] and top.tolist() == [[-2.0]]
    one = np.array([[4.0]], np.float32)
    assert select_top_k(one, 3)[0].tolist() == [[0, -1, -1]]
    for bad in (0, EXPLAIN_MAX_K + 1, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            select_top_k(r, bad)


# ---------------------------------------------------------------------------
# the oracle against a literal loop
# ---------------------------------------------------------------------------
def literal(det, rows, top_k):
    """One row at a time, in plain Python on fp32 scalars."""
    D = det.dims.d_in
    tensors = unflatten(torch.from_numpy(det.params), det.dims)
    x = det.standardise(rows)
    with torch.no_grad():
        _, y = functional_forward(tensors, torch.from_numpy(x))
    y = y.numpy()
    out_idx, out_res, dense = [], [], []
    for i in range(x.shape[0]):
        r = [np.float32(y[i, d] - x[i, d]) for d in range(D)]
        with np.errstate(all="ignore"):
            key = [math.inf if math.isnan(float(v * v)) else float(np.float32(v * v)) for v in r]
        left = list(range(D))
        idx, res = [], []
        for _ in range(top_k):
            if not left:
                idx.append(-1), res.append(np.float32(0))
                continue
            best = left[0]
            for d in left[1:]:
                if key[d] > key[best]:
                    best = d
            left.remove(best)
            idx.append(best), res.append(r[best])
        out_idx.append(idx), out_res.append(res), dense.append(r)
    return np.array(out_idx, np.int32), np.array(out_res, np.float32), np.array(dense, np.float32)


@pytest.mark.parametrize("scaler", ["standard", "minmax"])
@pytest.mark.parametrize("model_type,scorer", KINDS)
@pytest.mark.parametrize("top_k", [1, 3, EXPLAIN_MAX_K])
def test_oracle_matches_a_literal_loop(model_type, scorer, scaler, top_k):
    det = make_detector(model_type, scaler, scorer)
    rng = np.random.default_rng(4)
    rows = rng.normal(size=(23, 5)) * 3.0
    rows[7, 2] = np.nan          # the whole row reconstructs as NaN: every key ties, ascending feature
    rows[11, 0] = 1e300          # fp32 infinity after standardising
    ex = explain_rows_numpy(det, rows, top_k, dense=True)
    idx, res, dense = literal(det, rows, top_k)
    assert isinstance(ex, Explanation) and ex.rows.dtype == np.int64 and ex.rows.tolist() == list(range(23))
    assert same_bits(ex.idx, idx) and same_bits(ex.resid, res) and same_bits(ex.resid_full, dense)
    assert ex.sse.dtype == np.float32 and ex.sse.shape == (23,)
    assert (ex.latent_terms is not None) == (scorer == "cen")
    assert explain_rows_numpy(det, rows, top_k).resid_full is None


# ---------------------------------------------------------------------------
# TorchEngine.explain_rows
# ---------------------------------------------------------------------------
def test_which_unsorted_with_repeats_empty_and_no_rows():
    det = make_detector("hybrid", "standard", "cen")
    other = make_detector("autoencoder", "minmax", dims=ModelDims(6, 4, 3), seed=3)
    rng = np.random.default_rng(6)
    rows, rows6 = rng.normal(size=(40, 5)) * 2.0, (rng.normal(size=(9, 6)) * 2.0).astype(np.float32)
    which = np.array([33, 2, 2, 39, 0, 17, 2], np.int64)
    eng = engine()
    full = eng.explain_rows([det], [rows], top_k=4, dense=True)[0]
    got = eng.explain_rows([det, other, det, other],
                           [rows, rows6, rows, np.zeros((0, 6))], top_k=4,
                           which=[which, None, np.zeros(0, np.int64), None], dense=True)
    sub = got[0]
    assert sub.rows.tolist() == which.tolist()
    # the chosen rows are gathered first and forwarded as one batch: the bits of explaining rows[which]
    # (torch's CPU matrix product rounds a row differently in a batch of 7 than in one of 40)
    gathered = eng.explain_rows([det], [rows[which]], top_k=4, dense=True)[0]
    for name in ("idx", "resid", "resid_full", "sse", "latent_terms"):
        assert same_bits(getattr(sub, name), getattr(gathered, name)), name
        np.testing.assert_allclose(getattr(sub, name), getattr(full, name)[which], rtol=1e-5, atol=1e-6, err_msg=name)
    assert same_bits(sub.resid_full[1], sub.resid_full[2]) and same_bits(sub.idx[1], sub.idx[6])   # row 2, thrice
    assert got[1].rows.tolist() == list(range(9)) and got[1].idx.shape == (9, 4) and got[1].latent_terms is None
    assert same_bits(got[1].idx, explain_rows_numpy(other, rows6, 4).idx)
    for empty, D, Z in ((got[2], 5, 2), (got[3], 6, None)):
        assert empty.rows.shape == (0,) and empty.idx.shape == (0, 4) and empty.idx.dtype == np.int32
        assert empty.resid.shape == (0, 4) and empty.sse.shape == (0,) and empty.resid_full.shape == (0, D)
        assert (empty.latent_terms is None) if Z is None else (empty.latent_terms.shape == (0, Z))
    # a list of indices and a tensor are taken too
    by_list = eng.explain_rows([det], [rows], which=[[3, 1]])[0]   # (top_k defaults to 5: all five features)
    assert by_list.idx.shape == (2, 5) and by_list.idx[:, :4].tolist() == full.idx[[3, 1]].tolist()
    assert eng.explain_rows([det], [torch.from_numpy(rows)], top_k=4, which=[torch.tensor([3, 1])])[0].idx.tolist() \
        == full.idx[[3, 1]].tolist()


def test_bad_arguments_raise():
    det = make_detector()
    rows = np.zeros((4, 5))
    eng = engine()
    for bad in (0, EXPLAIN_MAX_K + 1):
        with pytest.raises(ValueError):
            eng.explain_rows([det], [rows], top_k=bad)
    for bad in ([4], [-1], [0, 7], np.array([0.0, 1.0]), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            eng.explain_rows([det], [rows], which=[bad])
    with pytest.raises(ValueError):
        eng.explain_rows([det], [np.zeros((4, 6))])
    with pytest.raises(ValueError):
        eng.explain_rows([det], [np.zeros(5)])
    with pytest.raises(ValueError):
        eng.explain_rows([det], [rows, rows])
    with pytest.raises(ValueError):
        eng.explain_rows([det], [rows], which=[None, None])
    assert check_which(None, 3).tolist() == [0, 1, 2] and check_which([], 0).shape == (0,)


@pytest.mark.parametrize("scaler", ["standard", "minmax"])
def test_autoencoder_score_from_sse_to_the_bit(scaler):
    det = make_detector("autoencoder", scaler)
    rng = np.random.default_rng(8)
    rows = rng.normal(size=(50, 5)) * 3.0
    which = np.array([5, 49, 0, 5, 21], np.int64)
    eng = engine()
    ex = eng.explain_rows([det], [rows], top_k=5, which=[which])[0]
    scores = eng.score_rows([det], [rows[which]])[0][0]
    assert same_bits(np.nan_to_num(_ae_scores(ex.sse, 5)), scores)
    ex = eng.explain_rows([det], [rows], top_k=5, dense=True)[0]
    assert same_bits(np.nan_to_num(_ae_scores(ex.sse, 5)), eng.score_rows([det], [rows])[0][0])
    # the top five of five features are all of them: their squares are the row's error
    np.testing.assert_allclose((ex.resid.astype(np.float64) ** 2).sum(axis=1), ex.sse, rtol=1e-5)
    np.testing.assert_array_equal(np.sort(ex.idx, axis=1), np.tile(np.arange(5, dtype=np.int32), (50, 1)))


def test_cen_score_from_latent_terms_to_the_bit():
    det = make_detector("hybrid", "standard", "cen")
    rng = np.random.default_rng(9)
    rows = rng.normal(size=(37, 5)) * 3.0
    eng = engine()
    ex = eng.explain_rows([det], [rows], top_k=2)[0]
    assert ex.latent_terms.dtype == np.float64 and ex.latent_terms.shape == (37, 2)
    acc = np.zeros(37)
    for j in range(2):
        acc += ex.latent_terms[:, j]
    assert same_bits(np.nan_to_num(np.sqrt(acc)), eng.score_rows([det], [rows])[0][0])
    knn = make_detector("hybrid", "standard", "knn")
    exk = eng.explain_rows([knn], [rows], top_k=2)[0]
    assert exk.latent_terms is None and exk.idx.shape == (37, 2)


@pytest.mark.parametrize("scaler", ["standard", "minmax"])
def test_expected_raw_inverts_standardise(scaler):
    det = make_detector("autoencoder", scaler)
    rng = np.random.default_rng(10)
    rows = rng.normal(size=(30, 5)) * 10.0 + 3.0
    x = det.standardise(rows)
    back = expected_raw(det, x, np.zeros_like(x))
    assert back.dtype == np.float64 and back.shape == rows.shape
    # the float64 forward transform of `back` gives (double)x back to float64 round-off.  With
    # u = 2^-53, first order: standard  back = fl(fl(x s) + m), then fl(fl(back - m) / s): four roundings
    # of relative u on quantities of size <= |x| + |m| / |s| in standardised units -> u (4 |x| + |m| / |s|);
    # minmax  back = fl(fl(x - min) / s), then fl(fl(back s) + min): u (3 |x - min| + |x|) <= u (4 |x| + 3 |min|).
    # Both lie under 5 u (|x| + |offset|), the 5 leaving room for the second-order terms.
    sc = det.scaler
    x64 = x.astype(np.float64)
    if scaler == "standard":
        fwd = (back - sc["mean_"]) / sc["scale_"]
        weight = np.abs(x64) + np.abs(sc["mean_"] / sc["scale_"])
    else:
        fwd = back * sc["scale_"] + sc["min_"]
        weight = np.abs(x64) + np.abs(sc["min_"])
    err = np.abs(fwd - x64)
    print(f"expected_raw {scaler}: max |forward(back) - x| {err.max():.3e}, worst / bound "
          f"{(err / (5 * 2.0 ** -53 * weight)).max():.3f}")
    assert np.all(err <= 5 * 2.0 ** -53 * weight)
    # so standardising the expectation gives x's own bits
    assert same_bits(det.standardise(back), x)
    # (extra) against the raw rows it is fp32-close only: x is the fp32 rounding of the standardised row
    scale = sc["scale_"] if scaler == "standard" else 1.0 / sc["scale_"]
    assert np.all(np.abs(back - rows) <= 2.0 ** -23 * (np.abs(x64) * np.abs(scale) + np.abs(rows)))
    # picked features
    idx = np.array([[4, 0, -1]] * 30, np.int32)
    pick = expected_raw(det, x[:, [4, 0, 0]], np.zeros((30, 3), np.float32), idx)
    assert same_bits(pick[:, :2], back[:, [4, 0]]) and np.all(np.isnan(pick[:, 2]))
    # a residual moves the expectation by resid * scale in raw units
    moved = expected_raw(det, x, np.ones_like(x))
    np.testing.assert_allclose(moved - back, np.broadcast_to(scale, rows.shape), rtol=1e-9)


# ---------------------------------------------------------------------------
# the command-line tool
# ---------------------------------------------------------------------------
def test_cli_explain_round_trip(tmp_path, capsys):
    from fedmse_decentralized_amd import detect

    det = make_detector("autoencoder", "standard")
    rng = np.random.default_rng(2)
    rows = rng.normal(size=(41, 5)) * 3.0
    base = engine().score_rows([det], [rows])[0]
    det.threshold = float(np.sort(base[0])[30]) * (1 + 1e-9)
    bundle = det.save(str(tmp_path / "detector.npz"))
    inp = str(tmp_path / "traffic.csv")
    np.savetxt(inp, rows, delimiter=",", fmt="%.17g")
    plain, out = str(tmp_path / "plain.npz"), str(tmp_path / "explained.npz")
    assert detect.main(["--detector", bundle, "--input", inp, "--output", plain, "--backend", "torch"]) == 0
    line0 = capsys.readouterr().out.strip().splitlines()[-1]
    assert "explained" not in line0
    assert detect.main(["--detector", bundle, "--input", inp, "--output", out, "--backend", "torch",
                        "--explain", "3"]) == 0
    words = capsys.readouterr().out.strip().splitlines()[-1].split()
    with np.load(plain, allow_pickle=False) as z:
        assert sorted(z.files) == ["alarms", "flags", "scores", "threshold"]
        flags = z["flags"]
    which = np.flatnonzero(flags)
    assert 0 < which.size < 41
    assert words[words.index("explained") + 1] == str(which.size) and words[words.index("top_k") + 1] == "3"
    assert words[:words.index("explained")][:2] == line0.split()[:2]
    want = explain_rows_numpy(det, rows, 3, which=which)
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["alarms", "flags", "scores", "threshold", "explain_rows", "explain_idx",
                                          "explain_resid", "explain_share", "explain_observed", "explain_expected"])
        assert same_bits(z["flags"], flags)
        assert same_bits(z["explain_rows"], which.astype(np.int64)) and same_bits(z["explain_idx"], want.idx)
        assert same_bits(z["explain_resid"], want.resid)
        share, obs, exp = z["explain_share"], z["explain_observed"], z["explain_expected"]
    assert share.dtype == np.float64 and share.shape == (which.size, 3)
    assert np.all(share >= 0) and np.all(share.sum(axis=1) <= 1 + 1e-6) and np.all(np.diff(share, axis=1) <= 0)
    np.testing.assert_array_equal(obs, np.take_along_axis(rows[which], want.idx.astype(np.int64), axis=1))
    # expected - observed = resid * scale_ in raw units
    scale = det.scaler["scale_"][want.idx]
    np.testing.assert_allclose(exp - obs, want.resid.astype(np.float64) * scale, rtol=1e-5, atol=1e-6)
    for bad in ("17", "0", "-1"):
        with pytest.raises(SystemExit):
            detect.main(["--detector", bundle, "--input", inp, "--backend", "torch", "--explain", bad])
