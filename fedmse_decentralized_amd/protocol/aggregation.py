"""Aggregation rules as (source model, weight) plans.

The plan is computed on the host, identically on every rank; the engine then
executes ``sum_k w_k * theta_src(k)`` in plan order on the device
(``weighted_sum``), so every rank produces a bit-identical aggregate.

* ``avg`` / ``fedprox`` — plain mean over the selected clients: every weight
  is ``num_samples / total = 1 / K`` (`src/Trainer/client_trainer.py:107-113`,
  `:132-134`; FedProx's proximal term lives in local training).
* ``mse_avg`` (FedMSE) — weights proportional to ``1 / MSE`` of each model on
  the shared dev set (`src/Trainer/client_trainer.py:115-130`).
* ``fusion_avg`` — the legacy centralised aggregator's KDE/JS-similarity
  weighting: weights from ``utils.similarity.fusion_weights``
  of each model's dev-set reconstruction similarity, computed by the caller.

``compat="reference"`` reproduces the state-dict aliasing of the reference's
``fed_mse_avg``: the aggregator loads every gathered state into
its own module, and its own ``state_dict()`` entries alias that module, so

* its own entry is weighted with the MSE of the model loaded just before it
  (its own model if it is first), and
* its own entry's *values* at averaging time are those of the last model
  loaded (the last selected model, or the second to last if the aggregator is
  itself last).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

Plan = List[Tuple[int, float]]


def plan_mean(selected: Sequence[int], num_samples: Dict[int, float] = None) -> Plan:
    """FedAvg / FedProx.  The reference passes ``num_samples = 1.0`` for every
    model (Q13), i.e. a plain mean; ``num_samples`` (client -> training-set
    size) gives the textbook sample-weighted FedAvg instead."""
    if num_samples is None:
        k = len(selected)
        return [(cid, 1.0 / k) for cid in selected]
    tot = sum(float(num_samples[c]) for c in selected)
    return [(cid, float(num_samples[cid]) / tot) for cid in selected]


def plan_mse_avg(selected: Sequence[int], aggregator: int, dev_mse: Dict[int, float], compat: str = "reference") -> Plan:
    sel = list(selected)
    K = len(sel)
    raw: List[Tuple[int, float]] = []
    if compat == "reference" and aggregator in sel and K >= 1:
        a = sel.index(aggregator)
        for k, cid in enumerate(sel):
            if k != a:
                raw.append((cid, 1.0 / dev_mse[cid]))
                continue
            w_src = sel[a - 1] if a >= 1 else sel[a]
            if a != K - 1:
                v_src = sel[K - 1]
            else:
                v_src = sel[K - 2] if K >= 2 else sel[a]
            raw.append((v_src, 1.0 / dev_mse[w_src]))
    else:
        raw = [(cid, 1.0 / dev_mse[cid]) for cid in sel]
    tot = sum(w for _, w in raw)
    return [(cid, w / tot) for cid, w in raw]


def plan_fusion(selected: Sequence[int], sim: Dict[int, float] = None, weights: Sequence[float] = None) -> Plan:
    """``weights``: already formed (the HIP engine forms them on the device,
    ``utils.similarity.fusion_weights_t``); else from the similarity scores."""
    from ..utils.similarity import fusion_weights

    w = weights if weights is not None else fusion_weights([sim[c] for c in selected])
    return [(cid, float(x)) for cid, x in zip(selected, w)]


UPDATE_TYPES = ("avg", "fedprox", "mse_avg", "fusion_avg", "trimmed_mean", "median", "krum", "multi_krum", "geomed")

# Robust rules: a per-coordinate order-statistic selection over the selected
# models, which no (source, weight) plan expresses.  For every coordinate the
# k values are ranked under the total order -inf < ... < -0 < +0 < ... < +inf
# < NaN (ties by selection position), the ``t`` lowest and ``t`` highest are
# dropped, and the rest are added in selection order (fp32, one rounding per
# add) and divided by ``k - 2t`` (``Engine.robust_aggregate``).  The result
# depends only on the gathered models and their order, so every rank computes
# the same bits.  Local training is plain (mu = 0), as for ``avg``.
ROBUST_TYPES = ("trimmed_mean", "median")


def trim_count(update_type: str, k: int, ratio: float = 0.2) -> int:
    """Models dropped at EACH end of every coordinate's order.
    ``trimmed_mean``: ``floor(ratio * k)``, at most ``(k - 1) // 2`` (at least
    one model is always kept); ``median``: ``(k - 1) // 2`` (the middle value
    for odd k, the mean of the two middle values for even k)."""
    if k < 1:
        raise ValueError(f"trim_count: k = {k}")
    half = (k - 1) // 2
    if update_type == "median":
        return half
    if update_type == "trimmed_mean":
        if not 0.0 <= ratio < 0.5:
            raise ValueError(f"robust_trim_ratio must be in [0, 0.5), got {ratio}")
        return min(int(ratio * k), half)
    raise ValueError(f"Not a robust update type: {update_type}")


# Distance-based rules (Blanchard et al. 2017): whole models far from the crowd
# are discarded, so the aggregate holds only models that clients trained.  With
# k selected models (rows of P fp32 values, selection order) and
# ``f, q, m = krum_counts(...)``:
#   1. d(i, j): per coordinate e = fp32(a - b), s = (double)e * (double)e; the
#      row zero-extended to a multiple of 256; p_l = s_l + s_{l+256} + ... in
#      that order in f64 (l < 256); eight folds p_l += p_{l+h}, h = 128 .. 1;
#      d = p_0, NaN -> +inf;
#   2. score_i: model i's k - 1 distances ranked ascending (ties by the smaller
#      j), the q lowest added in order of j in f64 (q = 0: 0.0);
#   3. rank_i = #{l : score_l < score_i or (score_l == score_i and l < i)};
#      model i is kept iff rank_i < m;
#   4. per coordinate the kept values added in selection order in fp32, divided
#      (IEEE) by (float)m  (``Engine.krum_aggregate``).
# Like the robust rules these are no (source, weight) plan and train plainly.
KRUM_TYPES = ("krum", "multi_krum")


def krum_counts(update_type: str, k: int, ratio: float = 0.2):
    """``(f, q, m)``: models assumed poisoned ``f = min(floor(ratio * k),
    max((k - 3) // 2, 0))``, neighbours scored ``q = max(k - f - 2, 0)``, models
    kept ``m`` (``krum``: 1, ``multi_krum``: ``k - f``)."""
    if update_type not in KRUM_TYPES:
        raise ValueError(f"Not a krum update type: {update_type}")
    if k < 1:
        raise ValueError(f"krum_counts: k = {k}")
    if not 0.0 <= ratio < 0.5:
        raise ValueError(f"robust_trim_ratio must be in [0, 0.5), got {ratio}")
    f = min(int(ratio * k), max((k - 3) // 2, 0))
    return f, max(k - f - 2, 0), 1 if update_type == "krum" else k - f


# Geometric median (RFA: Pillutla, Kakade, Harchaoui 2019) by smoothed Weiszfeld
# iterations: a model is down-weighted continuously with its distance from the
# crowd, no share of poisoned clients is assumed and every honest model keeps
# its contribution (breakdown point 1/2).  k selected models (rows of P fp32
# values, selection order; the whole row counts, padding included), T =
# ``geomed_iters`` in 0..64, nu = ``geomed_nu`` a finite float64 > 0.  All
# arithmetic is IEEE, one rounding per operation, no contraction.
#   * block sum of a length-P f64 vector s: zero-extended to nb = ceil(P / 256)
#     blocks of 256; in block b lane l holds s[256 b + l]; eight folds p_l +=
#     p_{l+h}, h = 128 .. 1, give q_b = p_0; the sum is ((+0.0 + q_0) + q_1) +
#     ... + q_{nb-1} in block order;
#   * lane sum of a length-k f64 vector x: zero-extended to a multiple of 256;
#     lane l adds x_l + x_{l+256} + ... in that order from +0.0; then the same
#     eight folds.
#   1. d_i(z): per coordinate e = fp32(theta_i[c] - z[c]) (one rounding), s_c =
#      (double)e * (double)e (exact in f64), d_i the block sum of s; d_i(None)
#      has z = 0, so e = theta_i[c].  A d_i that is NaN or +inf is stored as
#      +inf, and the row is bad for that step.
#   2. step -1: d_i = d_i(None), beta_i = 1.0 for a finite d_i, else 0.0 (the
#      squared norm of a finite fp32 row cannot overflow f64: a row is bad iff
#      it holds a NaN or an infinity).
#   3. steps t = 0 .. T: B the lane sum of beta.  B == 0 (every row bad): every
#      w_i = 0.0, every output coordinate the fp32 NaN 0x7FC00000, and the rule
#      ends.  Else w_i = beta_i / B (f64); per coordinate acc = +0.0 (f64), and
#      for i = 0 .. k-1 in selection order with beta_i != 0: acc = acc + (w_i *
#      (double)theta_i[c]) (the product rounded, then the sum; rows with beta_i
#      == 0 are not read into the sum); z_t[c] = (float)acc.  t == T stops; else
#      d_i = d_i(z_t), r_i = sqrt(d_i), beta_i = 1.0 / max(r_i, nu) for a finite
#      d_i, else 0.0.
#   4. the aggregate is z_T; weights[k] (f64) the w_i that formed it; dist[k]
#      (f64) the squared distances d_i those weights came from, +inf for a bad
#      row  (``Engine.geomed_aggregate``).
# T = 0 is the mean over the rows that hold no NaN / infinity, accumulated in
# f64.  Like the other robust rules this is no (source, weight) plan (the
# weights depend on the models) and it trains plainly.
GEOMED_TYPES = ("geomed",)
GEOMED_MAX_ITERS = 64


def geomed_check(iters, nu):
    """``(int(iters), float(nu))`` for ``iters`` an integer in 0..64 and ``nu``
    a finite float > 0; ValueError otherwise."""
    import math

    if isinstance(iters, bool) or not hasattr(iters, "__index__"):   # (no floats, no strings)
        raise ValueError(f"geomed_iters must be an integer in 0..{GEOMED_MAX_ITERS}, got {iters!r}")
    it = int(iters)
    if not 0 <= it <= GEOMED_MAX_ITERS:
        raise ValueError(f"geomed_iters must be an integer in 0..{GEOMED_MAX_ITERS}, got {iters!r}")
    try:
        x = float(nu)
    except (TypeError, ValueError):
        raise ValueError(f"geomed_nu must be a finite number > 0, got {nu!r}") from None
    if isinstance(nu, bool) or not (x > 0.0 and math.isfinite(x)):
        raise ValueError(f"geomed_nu must be a finite number > 0, got {nu!r}")
    return it, x


def make_plan(update_type: str, selected: Sequence[int], aggregator: int, dev_mse: Dict[int, float] = None,
              compat: str = "reference", sim: Dict[int, float] = None, num_samples: Dict[int, float] = None,
              fusion_w: Sequence[float] = None) -> Plan:
    if update_type in ("avg", "fedprox"):
        return plan_mean(selected, num_samples)
    if update_type == "mse_avg":
        return plan_mse_avg(selected, aggregator, dev_mse, compat)
    if update_type == "fusion_avg":
        return plan_fusion(selected, sim, fusion_w)
    raise ValueError(f"Unknown update type: {update_type}")
