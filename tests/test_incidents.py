"""Incidents on the CPU (README "Incidents"): ``incidents_numpy`` against a
row-by-row walk of the rule, the bound on the number of incidents, hand cases,
``incident_min_alarms`` against exact binomial tails, every ``ValueError``,
``TorchEngine.incidents`` / ``score_incidents`` against the oracle composed
with ``score_rows``, and ``detect --incidents``."""
import dataclasses
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from fedmse_decentralized_amd.deploy.detector import (Detector, Incidents, incident_bound, incident_min_alarms,
                                                      incidents_numpy, score_rows_numpy)
from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
from fedmse_decentralized_amd.models.layout import ModelDims

DBL_MAX = np.finfo(np.float64).max
ARRAYS = ("start", "end", "alarms", "peak_row", "peak_score")
SCALARS = ("n", "window", "min_alarms", "hold", "hot_rows", "count", "rows_covered", "longest")


def walk(flags, scores, w, m, h):
    """The rule, one row at a time: a dict of plain lists and ints."""
    n = len(flags)
    f = [1 if v != 0 else 0 for v in flags]
    s = [float(v) for v in np.nan_to_num(np.asarray(scores, dtype=np.float64))]
    hot = [sum(f[max(0, i - w + 1):i + 1]) >= m for i in range(n)]
    inc, open_, last_hot = [], None, None
    for i in range(n):
        if not hot[i]:
            continue
        if open_ is None or i - last_hot - 1 > h:      # more than h cold rows since the last hot one
            if open_ is not None:
                inc.append((open_, last_hot))
            open_ = i
        last_hot = i
    if open_ is not None:
        inc.append((open_, last_hot))
    out = dict(start=[], end=[], alarms=[], peak_row=[], peak_score=[], hot_rows=sum(hot), count=len(inc),
               rows_covered=sum(b - a + 1 for a, b in inc), longest=max([b - a + 1 for a, b in inc], default=0))
    for a, b in inc:
        best = a
        for r in range(a, b + 1):
            if s[r] > s[best]:
                best = r
        out["start"].append(a)
        out["end"].append(b)
        out["alarms"].append(sum(f[max(0, a - w + 1):b + 1]))
        out["peak_row"].append(best)
        out["peak_score"].append(s[best])
    return out


def agree(got: Incidents, want: dict, what):
    for k in ("hot_rows", "count", "rows_covered", "longest"):
        assert getattr(got, k) == want[k], (what, k, getattr(got, k), want[k])
    for k in ("start", "end", "alarms", "peak_row"):
        a = getattr(got, k)
        assert a.dtype == np.int64 and a.tolist() == want[k], (what, k, a, want[k])
    assert got.peak_score.dtype == np.float64
    assert got.peak_score.tobytes() == np.array(want["peak_score"], np.float64).tobytes(), (what, got.peak_score)


def same(a: Incidents, b: Incidents, what=""):
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), (what, k)
    for k in ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k, x, y)


def test_oracle_against_a_row_by_row_walk():
    rng = np.random.default_rng(20240)
    bound_hit = 0
    for case in range(3000):
        n = int(rng.integers(0, 81))
        w = int(rng.integers(1, 10))
        m = int(rng.integers(1, w + 1))
        h = int(rng.integers(0, 6))
        f = (rng.random(n) < rng.choice([0.05, 0.3, 0.5, 0.9])).astype(np.uint8) * rng.integers(1, 4, size=n).astype(np.uint8)
        s = np.round(rng.normal(size=n), 1)          # ties are common
        if case % 7 == 0 and n:
            s[rng.integers(0, n, size=3)] = rng.choice([np.nan, np.inf, -np.inf, -0.0, 0.0], size=3)
        got = incidents_numpy(f, s, w, m, h)
        what = f"case {case}: n={n} w={w} m={m} h={h}"
        assert (got.n, got.window, got.min_alarms, got.hold) == (n, w, m, h), what
        agree(got, walk(f, s, w, m, h), what)
        assert got.count <= incident_bound(n, h) == (n + h + 1) // (h + 2), what
        assert np.all(np.diff(got.start) >= h + 2), what
        assert np.all(got.start <= got.peak_row) and np.all(got.peak_row <= got.end), what
        bound_hit += got.count == incident_bound(n, h) and n > 0
    assert bound_hit > 0


def test_hand_cases():
    z = incidents_numpy(np.zeros(50, np.uint8), np.arange(50.0), 4, 2, 1)
    assert z.count == 0 and z.hot_rows == 0 and z.rows_covered == 0 and z.longest == 0 and z.start.shape == (0,)
    assert z.start.dtype == np.int64 and z.peak_score.dtype == np.float64
    for w, m in ((1, 1), (4, 1), (4, 3), (9, 9)):
        one = incidents_numpy(np.ones(30), np.zeros(30), w, m, 2)
        assert (one.start.tolist(), one.end.tolist(), one.count) == ([m - 1], [29], 1), (w, m)
        assert one.alarms.tolist() == [30] and one.hot_rows == 30 - (m - 1) and one.longest == 30 - (m - 1)
    for n in (1, 2, 9, 10):        # w = 1, m = 1, h = 0 on alternating flags reaches the bound
        alt = incidents_numpy(np.arange(n) % 2 == 0, np.zeros(n), 1, 1, 0)
        assert alt.count == incident_bound(n, 0) == (n + 1) // 2
        assert alt.start.tolist() == alt.end.tolist() == list(range(0, n, 2)) and alt.alarms.tolist() == [1] * alt.count
    # two hot runs [2, 3] and [3 + g + 1, ...]: a hold of g merges them, g - 1 does not
    f = np.array([0, 0, 1, 1, 0, 0, 0, 1, 1, 0], np.uint8)     # w = 1: hot = flags; three cold rows between
    merged = incidents_numpy(f, np.zeros(10), 1, 1, 3)
    assert (merged.start.tolist(), merged.end.tolist(), merged.alarms.tolist()) == ([2], [8], [4])
    assert merged.rows_covered == 7 and merged.hot_rows == 4
    apart = incidents_numpy(f, np.zeros(10), 1, 1, 2)
    assert (apart.start.tolist(), apart.end.tolist(), apart.alarms.tolist()) == ([2, 7], [3, 8], [2, 2])
    # the evidence window of the start counts: w = 3, m = 2
    ev = incidents_numpy(np.array([1, 0, 1, 0, 0, 0]), np.zeros(6), 3, 2, 0)
    assert (ev.start.tolist(), ev.end.tolist(), ev.alarms.tolist()) == ([2], [2], [2])
    # a peak tie: the earlier row; -0.0 ties with +0.0 and keeps its own bits
    tie = incidents_numpy(np.ones(6), np.array([1.0, 7.0, 3.0, 7.0, 7.0, 2.0]), 1, 1, 0)
    assert tie.peak_row.tolist() == [1] and tie.peak_score.tolist() == [7.0]
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        zt = incidents_numpy(np.ones(4), np.array([-1.0, first, second, -2.0]), 1, 1, 0)
        assert zt.peak_row.tolist() == [1] and np.signbit(zt.peak_score[0]) == np.signbit(first)
    # NaN -> 0, +-inf -> +-DBL_MAX before anything is compared
    un = incidents_numpy(np.ones(5), np.array([np.nan, -1.0, -np.inf, -3.0, -2.0]), 1, 1, 0)
    assert un.peak_row.tolist() == [0] and un.peak_score.tolist() == [0.0]
    un = incidents_numpy(np.ones(4), np.array([1.0, np.inf, DBL_MAX, np.nan]), 1, 1, 0)
    assert un.peak_row.tolist() == [1] and un.peak_score.tolist() == [DBL_MAX]
    un = incidents_numpy(np.ones(3), np.array([-np.inf, -DBL_MAX, -np.inf]), 1, 1, 0)
    assert un.peak_row.tolist() == [0] and un.peak_score.tolist() == [-DBL_MAX]
    cleaned = np.nan_to_num(np.array([np.nan, np.inf, -np.inf, 2.0]))
    same(incidents_numpy(np.ones(4), cleaned, 2, 1, 0), incidents_numpy(np.ones(4), np.nan_to_num(cleaned), 2, 1, 0))
    e = incidents_numpy(np.zeros(0), np.zeros(0), 3, 2, 1)
    assert e.n == 0 and e.count == 0 and e.start.shape == (0,)


def exact_tail(w, rate: Fraction, m):
    return sum(math.comb(w, j) * rate ** j * (1 - rate) ** (w - j) for j in range(m, w + 1))


def test_incident_min_alarms():
    rate = Fraction(1, 20)
    want = {(16, 1e-3): 5, (16, 1e-6): 8, (64, 1e-3): 11, (64, 1e-6): 15, (256, 1e-3): 26, (256, 1e-6): 33}
    for (w, tail), m in want.items():
        assert incident_min_alarms(w, 0.05, tail) == m, (w, tail)
        assert exact_tail(w, rate, m) <= Fraction(tail) < exact_tail(w, rate, m - 1), (w, tail)
    tails = [0.3, 1e-1, 1e-2, 1e-3, 1e-6, 1e-9, 1e-12]
    for w in (1, 2, 16, 64, 256, 4096):
        ms = [incident_min_alarms(w, 0.05, t) for t in tails]
        assert ms == sorted(ms) and 1 <= ms[0] and ms[-1] <= w, (w, ms)      # a smaller tail never asks for less
    for t in (1e-3, 1e-6):
        ms = [incident_min_alarms(w, 0.05, t) for w in range(1, 200)]
        assert all(b >= a for a, b in zip(ms, ms[1:])), t                      # nor does a longer window
    assert incident_min_alarms(4, 0.5, 1e-6) == 4        # 0.5^4 > 1e-6: unreachable, the window itself
    assert incident_min_alarms(1, 0.05, 1e-6) == 1
    assert incident_min_alarms(64, 0.0, 1e-6) == 1 and incident_min_alarms(64, 1.0, 1e-6) == 64
    assert "independent" in incident_min_alarms.__doc__ and "not a guarantee" in incident_min_alarms.__doc__
    for bad in ((0, 0.05, 1e-6), (4097, 0.05, 1e-6), (2.5, 0.05, 1e-6), (16, -0.1, 1e-6), (16, 1.5, 1e-6),
                (16, float("nan"), 1e-6), (16, 0.05, 0.0), (16, 0.05, 1.0), (16, 0.05, float("nan"))):
        with pytest.raises(ValueError):
            incident_min_alarms(*bad)


@pytest.mark.parametrize("run", ["oracle", "engine"])
def test_value_errors(run):
    eng = TorchEngine(ModelDims(5, 3, 2), torch.device("cpu"))
    call = incidents_numpy if run == "oracle" else (lambda f, s, *a: eng.incidents([f], [s], *a))
    f, s = np.ones(8, np.uint8), np.zeros(8)
    for bad in ((0, 1, 0), (4097, 1, 0), (True, 1, 0), (4.0, 1, 0), (4, 0, 0), (4, 5, 0), (4, 2.0, 0), (4, 2, -1),
                (4, 2, 4097), (4, 2, None)):
        with pytest.raises(ValueError):
            call(f, s, *bad)
    call(f, s, 4096, 4096, 4096)
    with pytest.raises(ValueError):
        call(f, s[:7], 4, 2, 0)
    with pytest.raises(ValueError):
        call(f.reshape(2, 4), s.reshape(2, 4), 4, 2, 0)
    with pytest.raises(ValueError):
        call(f[0], s[0], 4, 2, 0)
    if run == "engine":
        with pytest.raises(ValueError):
            eng.incidents([f, f], [s], 4, 2, 0)


def make_detector(model_type="autoencoder", scorer=None, dims=ModelDims(5, 3, 2), seed=0, threshold=0.75):
    rng = np.random.default_rng(seed)
    D, Z = dims.d_in, dims.latent
    sc = {"mean_": rng.normal(size=D), "scale_": rng.uniform(0.5, 2.0, size=D)}
    kw = {}
    if model_type == "hybrid":
        kw = dict(latent_scorer=scorer, latent_mean=rng.normal(size=Z), latent_scale=rng.uniform(0.5, 2.0, size=Z))
        if scorer == "knn":
            kw.update(knn_k=3, train_latents=rng.normal(size=(9, Z)).astype(np.float32))
    return Detector(dims=dims, model_type=model_type, params=(0.3 * rng.normal(size=dims.num_params)).astype(np.float32),
                    scaler_kind="standard", scaler=sc, threshold=threshold, detect_quantile=0.9, **kw)


def test_torch_engine_runs_the_oracle():
    eng = TorchEngine(ModelDims(5, 3, 2), torch.device("cpu"))
    rng = np.random.default_rng(4)
    flags = [(rng.random(n) < 0.4).astype(np.uint8) for n in (0, 1, 57, 300)]
    scores = [rng.normal(size=f.shape[0]) for f in flags]
    got = eng.incidents([flags[0], torch.from_numpy(flags[1]), flags[2].astype(np.int64) * 5, torch.from_numpy(flags[3])],
                        [scores[0], scores[1], torch.from_numpy(scores[2]), scores[3]], 6, 3, 2)
    assert len(got) == 4 and got[0].n == 0 and got[0].count == 0 and got[3].count > 1
    for f, s, g in zip(flags, scores, got):
        same(g, incidents_numpy(f, s, 6, 3, 2))
    assert eng.incidents([], [], 6, 3, 2) == []
    dets = [make_detector(), make_detector("hybrid", "cen", threshold=1.2), make_detector("hybrid", "knn", threshold=0.9),
            make_detector("autoencoder", dims=ModelDims(7, 4, 2), seed=3)]
    rows = [rng.normal(size=(n, d.dims.d_in)) * 2.0 for n, d in zip((120, 77, 0, 33), dets)]
    got = eng.score_incidents(dets, rows, 5, 2, 1)
    plain = eng.score_rows(dets, rows)
    assert len(got) == 4
    for g, p, d, x in zip(got, plain, dets, rows):
        assert len(g) == 4 and g[0].tobytes() == p[0].tobytes() and g[1].tobytes() == p[1].tobytes() and g[2] == p[2]
        s, f, a = score_rows_numpy(d, x)
        assert g[0].tobytes() == s.tobytes() and g[1].tobytes() == f.tobytes() and g[2] == a
        same(g[3], incidents_numpy(f, s, 5, 2, 1))
    assert got[0][3].count >= 1 and got[2][3].n == 0
    with pytest.raises(ValueError):
        eng.score_incidents(dets, rows, 5, 6, 1)


def test_cli_incidents(tmp_path, capsys):
    from fedmse_decentralized_amd import detect

    rng = np.random.default_rng(2)
    rows = rng.normal(size=(90, 5)) * 3.0
    det = make_detector("hybrid", "cen")
    det = dataclasses.replace(det, threshold=float(np.quantile(score_rows_numpy(det, rows)[0], 0.6)))
    bundle = det.save(str(tmp_path / "detector.npz"))
    src = tmp_path / "traffic"
    src.mkdir()
    np.savetxt(str(src / "a.csv"), rows[:50], delimiter=",", fmt="%.17g")
    np.savetxt(str(src / "b.csv"), rows[50:], delimiter=",", fmt="%.17g")   # (a window runs across the file boundary)
    base = ["--detector", bundle, "--input", str(src), "--backend", "torch"]
    plain, out = str(tmp_path / "plain.npz"), str(tmp_path / "inc.npz")
    assert detect.main(base + ["--output", plain]) == 0
    plain_lines = capsys.readouterr().out.strip().splitlines()
    assert len(plain_lines) == 1 and plain_lines[0].startswith("detect:")
    with np.load(plain, allow_pickle=False) as z:
        assert sorted(z.files) == ["alarms", "flags", "scores", "threshold"]     # the keys of before
        plain_arrays = {k: z[k] for k in z.files}
    s, f, a = score_rows_numpy(det, rows)
    assert 0 < a < 90

    def run(extra, w, m, h):
        assert detect.main(base + ["--output", out, "--incidents"] + extra) == 0
        lines = capsys.readouterr().out.strip().splitlines()
        want = incidents_numpy(f, s, w, m, h)
        assert len(lines) == 2 and lines[0].split()[:5] == plain_lines[0].split()[:5]
        assert lines[1] == (f"incidents: count {want.count} rows_covered {want.rows_covered} longest {want.longest} "
                            f"hot_rows {want.hot_rows} window {w} min {m} hold {h}")
        with np.load(out, allow_pickle=False) as z:
            assert sorted(z.files) == sorted(list(plain_arrays) + ["incident_" + k for k in ARRAYS] + ["incident_params"])
            for k, v in plain_arrays.items():
                assert z[k].dtype == v.dtype and z[k].tobytes() == v.tobytes(), k
            for k in ARRAYS:
                g = z["incident_" + k]
                assert g.dtype == getattr(want, k).dtype and g.tobytes() == getattr(want, k).tobytes(), k
            assert z["incident_params"].dtype == np.int64 and z["incident_params"].tolist() == [w, m, h]
        return want

    got = run(["--incident-window", "4", "--incident-min", "2", "--incident-hold", "1"], 4, 2, 1)
    assert got.count >= 1
    run(["--incident-window", "8", "--incident-min", "3"], 8, 3, 8)                       # hold defaults to the window
    auto = incident_min_alarms(64, 1.0 - det.detect_quantile, 1e-6)
    run([], 64, auto, 64)                                                                 # the defaults: 64, auto, 1e-6
    run(["--incident-window", "16", "--incident-min", "auto", "--incident-tail", "1e-3"], 16,
        incident_min_alarms(16, 1.0 - det.detect_quantile, 1e-3), 16)
    for bad in (["--incident-window", "0"], ["--incident-window", "4097"], ["--incident-min", "0"],
                ["--incident-window", "4", "--incident-min", "5"], ["--incident-min", "many"],
                ["--incident-hold", "-1"], ["--incident-hold", "4097"], ["--incident-tail", "0"],
                ["--incident-tail", "1.5"]):
        with pytest.raises(SystemExit):
            detect.main(base + ["--incidents"] + bad)
        capsys.readouterr()
    # with --explain the explained rows stay the flagged rows
    assert detect.main(base + ["--output", out, "--incidents", "--incident-window", "4", "--incident-min", "2",
                               "--explain", "2"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and f"explained {a} top_k 2" in lines[0] and lines[1].startswith("incidents: ")
    with np.load(out, allow_pickle=False) as z:
        assert z["explain_rows"].tolist() == np.flatnonzero(f).tolist() and "incident_start" in z.files
