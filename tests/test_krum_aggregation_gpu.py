"""Krum / Multi-Krum on the GPU: the three kernels of fedmx_krum.hip against
the numpy oracles of tests/test_krum_aggregation.py bit for bit, stage by
stage (distances, scores, kept mask and positions, aggregate), the
skipped-election contract, the argument checks, the two engines against each
other, and the device-resident round against the host-decision path under a
poisoning client."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fedmse_decentralized_amd.config import ExperimentConfig
from test_krum_aggregation import RATIOS, RULES, counts, make_stack, oracle_dist, oracle_fast, oracle_literal, \
    same_f64_bits
from test_robust_aggregation import assert_same_bits

P_PAD = 9216
# The issue's sizes, plus the edges the implementation introduces: the distance
# kernel tiles the pairs 4 x 4 (edges at every multiple of 4: k = 4 and 8 are
# full tiles, 5 and 9 one past; 64 / 65 and 256 / 257 likewise), and the score
# and selection kernels walk k in strides of their 256 threads (256 is the last
# single-stride k, 257 the first that takes a second pass).
KS = [1, 2, 3, 4, 5, 8, 9, 40, 64, 65, 256, 257]


def _launch(base_np, rows_np, k, f, m, state=None):
    """One krum_aggregate over sentinel-filled outputs: (out, D, score, kept, pos)."""
    from fedmse_decentralized_amd.ops import _hip

    dev = torch.device("cuda", 0)
    base = base_np if isinstance(base_np, torch.Tensor) else torch.from_numpy(base_np).to(dev)
    rows = None
    if rows_np is not None:
        rows = rows_np if isinstance(rows_np, torch.Tensor) else torch.from_numpy(rows_np).to(dev)
    P = base.shape[1]
    out = torch.full((P,), -7.0, dtype=torch.float32, device=dev)
    ws = torch.full((_hip.krum_workspace_size(k),), -7.0, dtype=torch.float64, device=dev)
    score = torch.full((k,), -7.0, dtype=torch.float64, device=dev)
    kept = torch.full((k,), -7, dtype=torch.int32, device=dev)
    _hip.krum_aggregate(base, None if rows is None else rows.data_ptr(), k, f, m, out,
                        state_ptr=0 if state is None else state.data_ptr(), workspace=ws, kept_out=kept,
                        score_out=score)
    torch.cuda.synchronize()
    ws = ws.cpu()
    pos = ws[k * k + k:].numpy().view(np.int32)[:k].copy()
    return out.cpu().numpy(), ws[:k * k].numpy().reshape(k, k).copy(), score.cpu().numpy(), kept.cpu().numpy(), pos


def _check(got, stack, D, q, m, literal=False):
    out, gD, score, kept, pos = got
    k = stack.shape[0]
    off = ~np.eye(k, dtype=bool)
    same_f64_bits(gD[off], D[off])                      # stage 1: the distance workspace
    want, wkept, wscore = (oracle_literal if literal else oracle_fast)(stack, D, q, m)
    same_f64_bits(score, wscore)                        # stage 2: scores
    np.testing.assert_array_equal(kept, wkept)          # selection: mask and compacted positions
    np.testing.assert_array_equal(pos[:m], np.flatnonzero(wkept))
    assert_same_bits(out, want)                         # stage 3: the aggregate


@pytest.mark.parametrize("P", [P_PAD, 100])
@pytest.mark.parametrize("k", KS)
def test_kernels_match_oracle(k, P):
    """A base of 2k + 3 rows read through a scattered, non-monotone row table;
    both rules at ratios 0 and 0.2 over one oracle distance matrix."""
    rng = np.random.default_rng(1000 * k + P)
    base = rng.normal(size=(2 * k + 3, P)).astype(np.float32)
    rows = rng.permutation(2 * k + 3)[:k].astype(np.int64)
    if k >= 2 and not np.any(np.diff(rows) < 0):
        rows = rows[::-1].copy()
    assert k < 2 or np.any(np.diff(rows) < 0)
    stack = base[rows]
    D = oracle_dist(stack)
    dev = torch.device("cuda", 0)
    base_t, rows_t = torch.from_numpy(base).to(dev), torch.from_numpy(rows).to(dev)
    for rule in RULES:
        for ratio in RATIOS:
            f, q, m = counts(rule, k, ratio)
            _check(_launch(base_t, rows_t, k, f, m), stack, D, q, m, literal=(k <= 9 and P == 100))


def test_kernels_largest_k():
    k, P = 1024, 100
    rng = np.random.default_rng(1024)
    base = rng.normal(size=(2 * k + 3, P)).astype(np.float32)
    rows = rng.permutation(2 * k + 3)[:k].astype(np.int64)
    stack = base[rows]
    D = oracle_dist(stack)
    f, q, m = counts("multi_krum", k, 0.2)
    _check(_launch(base, rows, k, f, m), stack, D, q, m)


@pytest.mark.parametrize("kind", ["tie", "identical", "inf", "nan", "subnormal"])
@pytest.mark.parametrize("k", [5, 9])
def test_kernels_special_stacks(k, kind):
    stack = make_stack(kind, np.random.default_rng(10 * k), k, 300)
    D = oracle_dist(stack)
    if kind == "subnormal":
        assert D[k // 2, k - 1] == 2.0 ** -298
    for rule in RULES:
        for ratio in RATIOS:
            f, q, m = counts(rule, k, ratio)
            got = _launch(stack, None, k, f, m)
            _check(got, stack, D, q, m, literal=True)
            if kind in ("inf", "nan") and f >= 1:
                assert got[3][k // 2] == 0


def test_kernels_skipped_election():
    rng = np.random.default_rng(9)
    base = rng.normal(size=(13, P_PAD)).astype(np.float32)
    rows = rng.permutation(13)[:5].astype(np.int64)
    dev = torch.device("cuda", 0)
    state = torch.tensor([-1, -1, 0, 0], dtype=torch.int32, device=dev)
    out, D, score, kept, pos = _launch(base, rows, 5, 1, 4, state=state)
    assert np.all(out == -7.0) and np.all(D == -7.0) and np.all(score == -7.0) and np.all(kept == -7)
    state[0] = 0   # client 0 elected
    stack = base[rows]
    _check(_launch(base, rows, 5, 1, 4, state=state), stack, oracle_dist(stack), 2, 4)


def test_kernels_bounds():
    from fedmse_decentralized_amd.ops import _hip

    assert _hip.lib().fedmx_krum_max_k() == _hip.KRUM_MAX_K == 1024 and _hip.lib().fedmx_krum_tile() == 4
    dev = torch.device("cuda", 0)
    big = torch.zeros(1025, 8, dtype=torch.float32, device=dev)
    sent = torch.full((8,), -7.0, dtype=torch.float32, device=dev)
    kept = torch.full((1025,), -7, dtype=torch.int32, device=dev)
    score = torch.full((1025,), -7.0, dtype=torch.float64, device=dev)
    for k, f, m in [(0, 0, 1), (1025, 0, 1), (5, 0, 0), (5, 0, 6), (5, -1, 1)]:
        with pytest.raises(ValueError):
            _hip.krum_aggregate(big, None, k, f, m, sent, kept_out=kept, score_out=score)
    with pytest.raises(ValueError):   # wrong dtypes / devices
        _hip.krum_aggregate(big.double(), None, 5, 0, 1, sent)
    with pytest.raises(ValueError):
        _hip.krum_aggregate(big, None, 5, 0, 1, sent.cpu())
    with pytest.raises(ValueError):
        _hip.krum_aggregate(big, None, 5, 0, 1, sent, workspace=torch.zeros(64, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        _hip.krum_aggregate(big, None, 5, 0, 1, sent, kept_out=kept.long())
    with pytest.raises(ValueError):
        _hip.krum_aggregate(big, None, 5, 0, 1, sent, score_out=score.cpu())
    torch.cuda.synchronize()
    assert torch.all(sent == -7.0) and torch.all(kept == -7) and torch.all(score == -7.0)


@pytest.mark.parametrize("k", [5, 40])
def test_hip_engine_matches_torch_engine(k):
    from fedmse_decentralized_amd.engine.hip_engine import HipEngine
    from fedmse_decentralized_amd.engine.torch_engine import TorchEngine
    from fedmse_decentralized_amd.models.layout import DEFAULT_DIMS
    from fedmse_decentralized_amd.protocol.aggregation import krum_counts

    stack = torch.from_numpy(np.random.default_rng(k).normal(size=(k, P_PAD)).astype(np.float32))
    stack[k // 2] *= 25.0
    hip = HipEngine(DEFAULT_DIMS, torch.device("cuda", 0))
    cpu = TorchEngine(DEFAULT_DIMS, torch.device("cpu"))
    for ut in RULES:
        f, _, m = krum_counts(ut, k, 0.2)
        got, pos = hip.krum_aggregate(stack.cuda(), f, m)
        torch.cuda.synchronize()
        want, wpos = cpu.krum_aggregate(stack, f, m)
        assert got.shape == (P_PAD,) and pos == wpos and len(pos) == m and k // 2 not in pos
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
    base = dict(synthetic="nbaiot", network_size=6, num_rounds=6, epoch=2, batch_size=12, output_root=out,
                backend="hip", device="cuda", log_level="WARNING", compat="fixed", global_early_stop=False,
                save_checkpoints=True, model_types=["hybrid"], update_types=["multi_krum"],
                malicious_clients=[2], malicious_scale=25.0)
    base.update(kw)
    return ExperimentConfig(**base)


def _run(cfg, update_type, rounds):
    from fedmse_decentralized_amd import federation
    from fedmse_decentralized_amd.federation import Federation

    federation._PREP_CACHE.clear()
    fed = Federation(cfg, "hybrid", update_type, 0).setup()
    rs = [fed.run_round() for _ in range(rounds)]
    fed.finish()
    fed.writer.flush()
    out = dict(agg=[r.aggregator for r in rs], metrics=[r.metrics.tolist() for r in rs],
               ver=[r.verification for r in rs], sel=[r.selected for r in rs], kept=[r.agg_kept for r in rs])
    torch.cuda.synchronize()
    return fed, out


@pytest.mark.parametrize("update_type,participants", [("multi_krum", 0.5), ("multi_krum", 1.0), ("krum", 1.0)])
def test_device_round_matches_host_path(tmp_path, shrunk, update_type, participants):
    """Six clients, client 2 poisons its update (x 25): the device round
    (elect_wsum + the krum kernels) and the host-decision path take the same
    decisions, keep the same clients and leave the same parameters, anchors and
    files.  Three selections per round (f = 0: all three kept), and all six
    (f = 1: five kept, or one under krum)."""
    kw = dict(update_types=[update_type], num_participants=participants)
    fa, a = _run(_cfg(str(tmp_path / "dev"), device_protocol=True, **kw), update_type, 6)
    fb, b = _run(_cfg(str(tmp_path / "host"), device_protocol=False, **kw), update_type, 6)
    assert fa._fast is not None and fb._fast is None
    assert fa._fast.krum and fa._fast.rule == 0
    assert any(x is not None for x in a["agg"])
    assert a["sel"] == b["sel"]
    assert a["agg"] == b["agg"]
    assert a["ver"] == b["ver"]
    assert a["kept"] == b["kept"]
    for agg, sel, kept in zip(a["agg"], a["sel"], a["kept"]):
        if agg is None:
            assert kept is None
        elif participants == 1.0:
            assert len(kept) == (1 if update_type == "krum" else 5) and 2 not in kept
            assert kept == [c for c in sel if c in kept]
        else:
            assert kept == sel
    for x, y in zip(a["metrics"], b["metrics"]):
        np.testing.assert_array_equal(np.array(x), np.array(y))
    assert torch.equal(fa.engine.store.params, fb.engine.store.params)
    assert torch.equal(fa.engine.store.anchor, fb.engine.store.anchor)
    assert fa.agg_counts == fb.agg_counts
    n_ckpt = n_json = 0
    for root_a, _, files in os.walk(str(tmp_path / "dev")):
        for fn in files:
            pa = os.path.join(root_a, fn)
            pb = pa.replace(str(tmp_path / "dev"), str(tmp_path / "host"))
            if fn in ("model.cpt", "training_tracking.pkl"):
                assert open(pa, "rb").read() == open(pb, "rb").read(), pa
                n_ckpt += 1
            if fn.endswith(".json"):
                assert open(pa).read() == open(pb).read(), fn
                n_json += 1
    assert n_ckpt >= 2 * 3 and n_json >= 1


def test_device_round_centralized_matches_host_path(tmp_path, shrunk):
    kw = dict(save_checkpoints=False, aggregation_mode="centralized", num_participants=1.0)
    fa, a = _run(_cfg(str(tmp_path / "dev"), device_protocol=True, **kw), "multi_krum", 4)
    fb, b = _run(_cfg(str(tmp_path / "host"), device_protocol=False, **kw), "multi_krum", 4)
    assert fa._fast is not None and fb._fast is None
    assert a["kept"] == b["kept"]
    assert torch.equal(fa.engine.store.params, fb.engine.store.params)
