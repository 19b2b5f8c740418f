"""Geometric-median aggregation on the GPU: geomed_step_kernel
(fedmx_geomed.hip) against the numpy oracles of
tests/test_geomed_aggregation.py bit for bit -- aggregate, final weights and
the squared distances they came from -- iteration count by iteration count,
the skipped-election contract, the argument checks, the two engines against
each other, and the device-resident round against the host-decision path
under a poisoning client."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.config import ExperimentConfig
from test_geomed_aggregation import INF, NAN_BITS, make_stack, oracle_fast, oracle_literal, same_f64_bits
from test_robust_aggregation import assert_same_bits

P_PAD = 9216
ITERS = (0, 1, 2, 3, 8)   # on one stack: a failure names the step at which it starts
SENT = -7.0
SLACK = 5                 # sentinel elements behind every result and the workspace


def _launch(base, rows_ptr, k, iters, nu, state=None):
    """One geomed_aggregate over sentinel-filled outputs and workspace:
    (out, weights, dist); nothing behind the results may be written."""
    from fedmse_decentralized_amd.ops import _hip

    dev = base.device
    P = base.shape[1]
    need = _hip.geomed_workspace_size(k, P)
    assert need == 2 * (-(-P // 256)) * k
    out = torch.full((P,), SENT, dtype=torch.float32, device=dev)
    ws = torch.full((need + SLACK,), SENT, dtype=torch.float64, device=dev)
    w = torch.full((k + SLACK,), SENT, dtype=torch.float64, device=dev)
    d = torch.full((k + SLACK,), SENT, dtype=torch.float64, device=dev)
    _hip.geomed_aggregate(base, rows_ptr, k, iters, nu, out, state_ptr=0 if state is None else state.data_ptr(),
                          workspace=ws, weights_out=w, dist_out=d)
    torch.cuda.synchronize()
    ws, w, d = ws.cpu().numpy(), w.cpu().numpy(), d.cpu().numpy()
    assert np.all(ws[need:] == SENT) and np.all(w[k:] == SENT) and np.all(d[k:] == SENT)
    return out.cpu().numpy(), w[:k], d[:k], ws[:need]


def _check(base_t, rows_ptr, stack, nu=1e-6, iters=ITERS, literal=False):
    k = stack.shape[0]
    for T in iters:
        z, w, d, _ = _launch(base_t, rows_ptr, k, T, nu)
        zo, wo, do = (oracle_literal if literal else oracle_fast)(stack, T, nu)
        try:
            same_f64_bits(d, do)      # the distances the final weights came from
            same_f64_bits(w, wo)      # the final weights
            assert_same_bits(z, zo)   # the aggregate
        except AssertionError as e:
            raise AssertionError(f"first mismatch at iters = {T} (k = {k}, P = {stack.shape[1]}, nu = {nu}): {e}")
    return z, w, d


def _mapped_rows(rows: np.ndarray):
    """The row table in mapped host memory: (buffer kept alive, device-visible address)."""
    from fedmse_decentralized_amd.ops import _hiprt

    buf = _hiprt.MappedBuffer(8 * len(rows))
    buf.view(0, np.int64, len(rows))[:] = rows
    return buf, buf.dev_ptr


# the lane-sum edges (k) against the block edges (P); the large corners are
# k = 1024 with P = 257 and k = 257 with P = 9216
SHAPES = [(k, P) for k in (1, 2, 3, 5, 6) for P in (1, 255, 256, 257, 513, 9216)] + \
         [(k, P) for k in (255, 256, 257) for P in (1, 257, 513)] + [(257, 9216), (1024, 257)]


@pytest.mark.parametrize("k,P", SHAPES)
def test_kernel_matches_oracle(k, P):
    """A base of k + 3 rows read through a permuted row table with one row
    repeated, in mapped host memory; honest rows around one base, one pushed
    away."""
    rng = np.random.default_rng(1000 * k + P)
    base = (rng.normal(size=(1, P)) + 0.05 * rng.normal(size=(k + 3, P))).astype(np.float32)
    rows = rng.permutation(k + 3)[:k].astype(np.int64)
    if k >= 2:
        rows[-1] = rows[0]                       # a repeated row
        base[rows[k // 2]] *= np.float32(25.0)
    if k >= 3 and not np.any(np.diff(rows) < 0):
        rows[:-1] = rows[:-1][::-1].copy()
    buf, ptr = _mapped_rows(rows)
    base_t = torch.from_numpy(base).cuda()
    _check(base_t, ptr, base[rows], literal=(k <= 6 and P <= 257))
    torch.cuda.synchronize()
    del buf


@pytest.mark.parametrize("k,P", [(1, 257), (6, 513), (6, 9216), (257, 257)])
def test_kernel_null_row_table(k, P):
    stack = make_stack("crowd", np.random.default_rng(k + P), k, P)
    _check(torch.from_numpy(stack).cuda(), None, stack)


def _corner(kind, rng, k, P):
    if kind == "mean_row":
        # k = 5, small multiples of 4: the last row is the other four's mean
        # exactly and so the mean of all five, which z_0 meets to f64 rounding:
        # its distance from z_0 is far below nu
        assert k == 5
        x = (4.0 * rng.integers(-8, 9, size=(k, P))).astype(np.float32)
        x[4] = (x[:4].astype(np.float64).sum(0) / 4.0).astype(np.float32)
        return x
    if kind == "denormal":
        x = make_stack("subnormal", rng, k, P)
        x[k // 2] = np.float32(2.0 ** -149)
        return x
    if kind in ("first", "middle", "last"):
        x = make_stack("crowd", rng, k, P)
        nb = -(-P // 256)
        blk = {"first": 0, "middle": nb // 2, "last": nb - 1}[kind]
        lo, hi = 256 * blk, min(256 * blk + 256, P)
        for i, v in zip((0, k // 2, k - 1), (np.nan, np.inf, -np.inf)):
            x[i, int(rng.integers(lo, hi))] = v
        return x
    return make_stack(kind, rng, k, P)


@pytest.mark.parametrize("P", [600, P_PAD])
@pytest.mark.parametrize("kind", ["mean_row", "huge", "denormal", "first", "middle", "last", "allbad", "identical"])
def test_kernel_value_corners(kind, P):
    k = 5 if kind == "mean_row" else 6
    x = _corner(kind, np.random.default_rng(len(kind) + P), k, P)
    z, w, d = _check(torch.from_numpy(x).cuda(), None, x, literal=(P == 600))
    if kind == "mean_row":
        d1 = oracle_fast(x, 1, 1e-6)[2]
        assert np.sqrt(d1[k - 1]) < 1e-6 and np.argmax(w) == k - 1   # r < nu: beta = 1 / nu
    if kind in ("first", "middle", "last"):
        bad = [0, k // 2, k - 1]
        assert np.all(w[bad] == 0.0) and np.all(d[bad] == INF) and not np.isnan(z).any()
    if kind == "allbad":
        assert np.all(z.view(np.uint32) == NAN_BITS) and np.all(w == 0.0) and np.all(d == INF)
    if kind == "identical":
        assert_same_bits(z, x[0])
    if kind == "huge":
        assert np.all(np.isfinite(w)) and abs(w.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("nu", [1e3, 1e-300])
def test_kernel_smoothing(nu):
    x = make_stack("crowd", np.random.default_rng(3), 6, 700)
    z, w, d = _check(torch.from_numpy(x).cuda(), None, x, nu=nu)
    if nu == 1e3:   # larger than every distance: equal weights
        assert np.sqrt(d.max()) < nu
        same_f64_bits(w, np.full(6, w[0]))


def test_kernel_skipped_election():
    rng = np.random.default_rng(9)
    base = rng.normal(size=(13, P_PAD)).astype(np.float32)
    rows = rng.permutation(13)[:5].astype(np.int64)
    buf, ptr = _mapped_rows(rows)
    base_t = torch.from_numpy(base).cuda()
    state = torch.tensor([-1, -1, 0, 0], dtype=torch.int32, device="cuda")
    z, w, d, ws = _launch(base_t, ptr, 5, 3, 1e-6, state=state)
    assert np.all(z == SENT) and np.all(w == SENT) and np.all(d == SENT) and np.all(ws == SENT)
    state[0] = 0   # client 0 elected
    z, w, d, _ = _launch(base_t, ptr, 5, 3, 1e-6, state=state)
    zo, wo, do = oracle_fast(base[rows], 3, 1e-6)
    assert_same_bits(z, zo)
    same_f64_bits(w, wo)
    same_f64_bits(d, do)
    del buf


def test_kernel_argument_checks():
    from fedmse_decentralized_amd.ops import _hip

    assert _hip.lib().fedmx_geomed_max_k() == _hip.GEOMED_MAX_K == 1024
    dev = torch.device("cuda", 0)
    big = torch.zeros(1025, 8, dtype=torch.float32, device=dev)
    sent = torch.full((8,), SENT, dtype=torch.float32, device=dev)
    w = torch.full((1025,), SENT, dtype=torch.float64, device=dev)
    d = torch.full((1025,), SENT, dtype=torch.float64, device=dev)
    ws = torch.full((_hip.geomed_workspace_size(1024, 8),), SENT, dtype=torch.float64, device=dev)
    ok = dict(workspace=ws, weights_out=w, dist_out=d)
    for k, T, nu in [(0, 3, 1e-6), (1025, 3, 1e-6), (-1, 3, 1e-6), (5.0, 3, 1e-6), (5, -1, 1e-6), (5, 65, 1e-6),
                     (5, 1.5, 1e-6), (5, True, 1e-6), (5, 3, 0.0), (5, 3, -1.0), (5, 3, INF), (5, 3, float("nan")),
                     (5, 3, "1e-6"), (5, 3, None)]:
        with pytest.raises(ValueError):
            _hip.geomed_aggregate(big, None, k, T, nu, sent, **ok)
    bad_calls = [
        lambda: _hip.geomed_aggregate(big.double(), None, 5, 3, 1e-6, sent, **ok),             # base dtype
        lambda: _hip.geomed_aggregate(big.t(), None, 5, 3, 1e-6, sent, **ok),                  # base contiguity
        lambda: _hip.geomed_aggregate(big[0], None, 1, 3, 1e-6, sent, **ok),                   # base rank
        lambda: _hip.geomed_aggregate(big.cpu(), None, 5, 3, 1e-6, sent.cpu()),                # base device
        lambda: _hip.geomed_aggregate(big[:4], None, 5, 3, 1e-6, sent, **ok),                  # k past the stack
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent.cpu(), **ok),                # out device
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent.double(), **ok),             # out dtype
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent[:7], **ok),                  # out size
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, torch.zeros(16, device=dev)[::2], **ok),   # out stride
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, workspace=ws.float()),      # workspace dtype
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, workspace=ws[:9]),          # workspace size
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, workspace=ws.cpu()),        # workspace device
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, weights_out=w.float()),     # weights dtype
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, weights_out=w[:4]),         # weights size
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, weights_out=w.cpu()),       # weights device
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, dist_out=d.float()),        # dist dtype
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, dist_out=d[:4]),            # dist size
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, dist_out=d.cpu()),          # dist device
        lambda: _hip.geomed_aggregate(big, None, 5, 3, 1e-6, sent, dist_out=d[::2]),           # dist stride
    ]
    for n, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {n} went through")
    torch.cuda.synchronize()
    assert torch.all(sent == SENT) and torch.all(w == SENT) and torch.all(d == SENT) and torch.all(ws == SENT)
    # and the same arguments in range go through
    _hip.geomed_aggregate(big, None, 5, 0, 1e-6, sent, **ok)
    torch.cuda.synchronize()
    assert torch.all(sent == 0.0) and torch.all(w[:5] == 0.2) and torch.all(w[5:] == SENT)


@pytest.mark.parametrize("k", [5, 40])
def test_hip_engine_matches_torch_engine(k):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
    from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS

    stack = torch.from_numpy(make_stack("crowd", np.random.default_rng(k), k, P_PAD))
    hip = HipEngine(DEFAULT_DIMS, torch.device("cuda", 0))
    cpu = TorchEngine(DEFAULT_DIMS, torch.device("cpu"))
    for T, nu in ((0, 1e-6), (3, 1e-6), (8, 1e-3)):
        got, w = hip.geomed_aggregate(stack.cuda(), T, nu)
        torch.cuda.synchronize()
        want, ww = cpu.geomed_aggregate(stack, T, nu)
        assert got.shape == (P_PAD,) and isinstance(w, list) and len(w) == k
        same_f64_bits(np.asarray(w), np.asarray(ww))
        assert int(np.argmin(w)) == k // 2 or T == 0
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------
# the device-resident round against the host-decision path
# ----------------------------------------------------------------------------

SHRINK = dict(normal_rows=(150, 170), abnormal_rows=(200, 220), test_normal_rows=30)


@pytest.fixture()
def shrunk(monkeypatch):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.data import synthetic

    # (the unshrunk method when another GPU test file already shrank the class for the session)
    orig = getattr(synthetic.SyntheticSpec, "_fedmx_orig_resolved", synthetic.SyntheticSpec.resolved)

    def resolved(self):
        s = orig(self)
        s.normal_rows, s.abnormal_rows, s.test_normal_rows = SHRINK["normal_rows"], SHRINK["abnormal_rows"], \
            SHRINK["test_normal_rows"]
        return s
    monkeypatch.setattr(synthetic.SyntheticSpec, "resolved", resolved)
    federation._PREP_CACHE.clear()
    yield
    federation._PREP_CACHE.clear()


def _cfg(out, **kw):
    base = dict(synthetic="nbaiot", network_size=6, num_rounds=4, epoch=2, batch_size=12, output_root=out,
                backend="hip", device="cuda", log_level="WARNING", compat="fixed", global_early_stop=False,
                save_checkpoints=False, model_types=["hybrid"], update_types=["geomed"],
                malicious_clients=[2], malicious_scale=25.0)
    base.update(kw)
    return ExperimentConfig(**base)


def _run(cfg, rounds):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.federation import Federation

    federation._PREP_CACHE.clear()
    fed = Federation(cfg, "hybrid", "geomed", 0).setup()
    aggs = []
    if fed._fast is None:   # the host path's aggregates; the device round's is read below
        geomed = fed.engine.geomed_aggregate

        def rec(stack, iters, nu):
            out = geomed(stack, iters, nu)
            aggs.append(out[0].clone())
            return out
        fed.engine.geomed_aggregate = rec
    rs = []
    for _ in range(rounds):
        r = fed.run_round()
        if fed._fast is not None and r.aggregator is not None:
            aggs.append(fed._fast.agg.clone())
        rs.append(r)
    fed.finish()
    fed.writer.flush()
    out = dict(agg=[r.aggregator for r in rs], metrics=[r.metrics.tolist() for r in rs],
               ver=[r.verification for r in rs], sel=[r.selected for r in rs], w=[r.agg_weights for r in rs],
               kept=[r.agg_kept for r in rs], aggs=aggs)
    torch.cuda.synchronize()
    return fed, out


@pytest.mark.parametrize("participants", [0.5, 1.0])
def test_device_round_matches_host_path(tmp_path, shrunk, participants):
    """Six clients, client 2 poisons its update (x 25), four rounds: the device
    round (elect_wsum + the Weiszfeld launches) and the host-decision path
    elect the same aggregators, form the same aggregates and weights bit for
    bit, take the same adoption decisions and measure the same AUCs; the
    poisoned client's weight is the smallest whenever it is selected."""
    kw = dict(num_participants=participants)
    fa, a = _run(_cfg(str(tmp_path / "dev"), device_protocol=True, **kw), 4)
    fb, b = _run(_cfg(str(tmp_path / "host"), device_protocol=False, **kw), 4)
    assert fa._fast is not None and fb._fast is None
    assert fa._fast.geomed and fa._fast.rule == 0 and not fa._fast.krum and not fa._fast.robust
    assert any(x is not None for x in a["agg"])
    assert a["sel"] == b["sel"]
    assert a["agg"] == b["agg"]
    assert a["ver"] == b["ver"]
    assert a["kept"] == b["kept"] == [None] * 4
    assert len(a["aggs"]) == len(b["aggs"]) == sum(x is not None for x in a["agg"])
    for x, y in zip(a["aggs"], b["aggs"]):
        assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32))
    for agg, sel, wa, wb in zip(a["agg"], a["sel"], a["w"], b["w"]):
        if agg is None:
            assert wa is None and wb is None
            continue
        assert isinstance(wa, list) and len(wa) == len(sel)
        same_f64_bits(np.asarray(wa), np.asarray(wb))
        assert abs(sum(wa) - 1.0) < 1e-12
        if 2 in sel and len(sel) >= 3:
            assert sel[int(np.argmin(wa))] == 2
    for x, y in zip(a["metrics"], b["metrics"]):
        np.testing.assert_array_equal(np.array(x), np.array(y))
    assert torch.equal(fa.engine.store.params, fb.engine.store.params)
    assert torch.equal(fa.engine.store.anchor, fb.engine.store.anchor)
    assert fa.agg_counts == fb.agg_counts
