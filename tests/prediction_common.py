"""Prediction resampling and safety metrics restated in NumPy float64 for the tests (CPU and GPU), plus the seeded
generators of the rows and cases the differential tests run.

The restatements are written from the reference's definitions (trajectory_predictor.py:188-353,
data_structures.py:301-388) one (sample, pedestrian, axis) / one ego at a time, independent of ``oracle/`` and of the
library; ``tests/test_prediction_common.py`` pins them to the reference's own vectors under ``tests/golden/`` before
anything else uses them as a checker.

``close_to`` is np.allclose for finite values (|a - b| <= 1e-8 + 1e-5 |b|, elementwise) without its broadcasting and
NaN handling, because the GPU tests evaluate it a million times; the CPU tests hold it equal to np.allclose on every
generated row.
"""
import math

import numpy as np

MAX_WALKING_SPEED = 2.5
MAX_PRED_LEN = 32
MAX_NT = 256


# ---- process_prediction ---------------------------------------------------------------------------------------------
def time_target(sgan_dt, sim_dt, plan_horizon, pred_len):
    return np.arange(sim_dt, max(plan_horizon, pred_len * sgan_dt) + 1e-9, sim_dt)


def n_dense(sgan_dt, sim_dt, plan_horizon, pred_len):
    return len(time_target(sgan_dt, sim_dt, plan_horizon, pred_len))


def time_source(pred_len, sgan_dt, staleness, with_anchor):
    ts = np.arange(1, pred_len + 1) * sgan_dt - staleness
    return np.concatenate(([-staleness], ts)) if with_anchor else ts


def close_to(co, b):
    return bool(np.all(np.abs(co - b) <= 1e-8 + 1e-5 * abs(b)))


def row_is_constant(co):
    return close_to(co, co[0]) or close_to(co, 0.0)


def tail_velocity(co, sgan_dt, clamp=True):
    """Velocity of the last (up to) three sources, clamped to walking speed; 0 for a single source."""
    if len(co) < 2:
        return 0.0
    lookback = min(3, len(co))
    v = (co[-1] - co[-lookback]) / ((lookback - 1) * sgan_dt)
    return max(min(v, MAX_WALKING_SPEED), -MAX_WALKING_SPEED) if clamp else v


def resample_row(co, t_src, t_tgt, sgan_dt):
    """One coordinate axis of one pedestrian: float64 sources ``co`` at times ``t_src`` -> values at ``t_tgt``."""
    co = np.asarray(co, dtype=np.float64)
    if row_is_constant(co):
        return np.full(len(t_tgt), co[-1])
    out = np.interp(t_tgt, t_src, co)
    if len(co) >= 2:
        tail = t_tgt > t_src[-1]
        if tail.any():
            out[tail] = co[-1] + tail_velocity(co, sgan_dt) * (t_tgt[tail] - t_src[-1])
    return out


def process_prediction(pred, anchor, staleness, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0):
    """pred [pred_len, P, 2] (any float dtype, widened exactly), anchor [P, 2] or None -> [P, n_dense, 2] float64."""
    pred = np.asarray(pred).astype(np.float64)
    L, P = pred.shape[0], pred.shape[1]
    t_src = time_source(L, sgan_dt, staleness, anchor is not None)
    if anchor is not None:
        pred = np.concatenate((np.asarray(anchor, dtype=np.float64)[None], pred), axis=0)
    t_tgt = time_target(sgan_dt, sim_dt, plan_horizon, L)
    out = np.zeros((P, len(t_tgt), 2))
    for p in range(P):
        for ax in range(2):
            out[p, :, ax] = resample_row(pred[:, p, ax], t_src, t_tgt, sgan_dt)
    return out


def process_samples(pred, anchor, staleness, **kw):
    """pred [S, pred_len, P, 2] -> [S, P, n_dense, 2]."""
    return np.stack([process_prediction(pred[s], anchor, staleness, **kw) for s in range(pred.shape[0])])


# ---- predict_cv ------------------------------------------------------------------------------------------------------
def predict_cv(obs_last, obs_prev, staleness, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0):
    """obs_last / obs_prev [P, 2] in the observations' own dtype (obs_prev None: zero velocity) -> [P, n_dense, 2].
    The velocity is formed in that dtype (array / Python float keeps it), the extrapolation in float64 (a float32 array
    times a float64 value gives float64)."""
    cur = np.asarray(obs_last)
    assert cur.dtype in (np.float32, np.float64)
    if obs_prev is None:
        vel = np.zeros(cur.shape)
    else:
        prev = np.asarray(obs_prev)
        assert prev.dtype == cur.dtype
        vel = (cur - prev) / sgan_dt
        assert vel.dtype == cur.dtype
    t_tgt = time_target(sgan_dt, sim_dt, plan_horizon, pred_len)
    out = np.zeros((cur.shape[0], len(t_tgt), 2))
    for i in range(len(t_tgt)):
        t = np.asarray(t_tgt[i] + staleness, dtype=np.float64)
        step = cur + vel * t
        assert step.dtype == np.float64
        out[:, i, :] = step
    return out


# ---- closest to the sample mean ---------------------------------------------------------------------------------------
def sample_distances(x):
    """x [S, P, T, 2] -> [S]: each sample's summed distance to the sample mean; its argmin is the representative."""
    x = np.asarray(x).astype(np.float64)
    return np.linalg.norm(x - x.mean(axis=0)[None], axis=-1).sum(axis=(1, 2))


# ---- compute_safety_metrics_static -------------------------------------------------------------------------------------
def safety_metrics(ego, pos, vel, ego_radius, ped_radius, offsets=None, footprint_radius=None):
    """ego = x, y, yaw, v; pos / vel [P, 2]; offsets: footprint circle centres along the heading (None: one centre
    circle of ego_radius).  Returns the reference's dictionary."""
    x, y, yaw, v = (float(e) for e in ego)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    heading = np.array([np.cos(yaw), np.sin(yaw)])
    if offsets is None:
        centers = np.array([[x, y]])
        combined = ego_radius + ped_radius
    else:
        centers = np.array([x, y]) + np.asarray(offsets, dtype=np.float64)[:, None] * heading
        combined = footprint_radius + ped_radius
    inf = float("inf")
    if len(pos) == 0:
        return dict(min_distance=inf, collision=False, ttc=inf, clearance=inf - combined, clearance_ahead=inf)
    dist = np.linalg.norm(pos[None, :, :] - centers[:, None, :], axis=2)               # [circle, pedestrian]
    min_distance = float(dist.min())
    ego_vel = np.array([v * np.cos(yaw), v * np.sin(yaw)])
    ttc = inf
    for ci, c in enumerate(centers):
        for pi in range(len(pos)):
            rel_pos, rel_vel = pos[pi] - c, vel[pi] - ego_vel
            along = -np.dot(rel_pos, rel_vel) / (np.linalg.norm(rel_pos) + 1e-8)
            if along > 1e-5:
                t = (dist[ci, pi] - combined) / along
                if t >= 0:
                    ttc = min(ttc, float(t))
    ahead = (pos - np.array([x, y])) @ heading > 0.0
    clearance_ahead = float(dist[:, ahead].min()) - combined if ahead.any() else inf
    return dict(min_distance=min_distance, collision=bool(min_distance < combined), ttc=ttc,
                clearance=min_distance - combined, clearance_ahead=clearance_ahead)


# ---- generators --------------------------------------------------------------------------------------------------------
ROW_KINDS = ("walk", "fast_up", "fast_down", "constant", "zeros", "in_first", "out_first", "in_zero", "out_zero")
BOUND_MARGIN = 1e-3                       # the allclose classes sit this far (relative) from 1e-8 + 1e-5 |b|
# CPU only (exact arithmetic on both sides, no contraction): rows 5e-6 (relative) from the bound, where 1e-5 |b| and
# 1e-5 |co_i| -- np.allclose is not symmetric -- decide differently: one value away from zero just outside, or towards
# zero just inside
EDGE_MARGIN = 5e-6
CPU_ROW_KINDS = ROW_KINDS + ("edge_out_away", "edge_in_toward")


def _f32_near_bound_base(rng, factor):
    """A float32-representable b in [32, 64) and a deviation d = k ulp(b) with d = factor x (1e-8 + 1e-5 b) up to the
    rounding of b (6e-8 relative): float32 has 84..168 ulp per bound in a binade, so k is chosen and b solved for."""
    ulp = 2.0 ** -18
    k = int(rng.integers(90, 160))
    b = float(np.float32((k * ulp / factor - 1e-8) / 1e-5))
    assert 32.0 <= b < 64.0
    return b, k * ulp


def source_row(rng, kind, n_src, dtype, sgan_dt, first=None):
    """(kind, n_src source values) -- the anchor first when there is one -- every value representable in dtype and
    within +-100 m.  first: the value co[0] must take (a pedestrian's anchor is shared by its samples); a kind that
    cannot be built on it becomes a "walk"."""
    f = lambda a: np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)
    f32 = np.dtype(dtype) == np.float32
    if first is not None and (kind in ("zeros", "in_zero", "out_zero") or
                              (kind in ("in_first", "out_first") and (f32 or abs(first) < 1.0))):
        kind = "walk"
    if kind == "walk":
        co = rng.uniform(-60, 60) + np.cumsum(rng.normal(0, 0.5, n_src))
    elif kind in ("fast_up", "fast_down"):                 # a tail faster than walking speed: the clamp holds it
        sign = 1.0 if kind == "fast_up" else -1.0
        co = rng.uniform(-30, 30) + sign * rng.uniform(3.0, 6.0) * sgan_dt * np.arange(n_src) + rng.normal(0, 0.01, n_src)
    elif kind == "constant":
        co = np.full(n_src, rng.uniform(-90, 90) if first is None else first)
    elif kind == "zeros":
        co = np.zeros(n_src)
    elif kind in ("edge_out_away", "edge_in_toward"):
        assert first is None and not f32
        b = float(rng.uniform(5, 90))
        d = (1.0 + EDGE_MARGIN if kind == "edge_out_away" else 1.0 - EDGE_MARGIN) * (1e-8 + 1e-5 * b)
        co = np.full(n_src, b)
        co[int(rng.integers(1, n_src)) if n_src > 1 else 0] = b + d if kind == "edge_out_away" else b - d
        if rng.random() < 0.5:
            co = -co
    elif kind in ("in_first", "out_first"):
        factor = 1.0 - BOUND_MARGIN if kind == "in_first" else 1.0 + BOUND_MARGIN
        if f32:
            b, d = _f32_near_bound_base(rng, factor)
        else:
            b = float(rng.uniform(5, 90)) if first is None else abs(first)
            d = factor * (1e-8 + 1e-5 * b)
        sign = rng.choice([-1.0, 1.0])
        co = b + sign * d * rng.uniform(0.0, 0.9, n_src)    # the others stay well inside
        co[0] = b
        co[int(rng.integers(1, n_src)) if n_src > 1 else 0] = b + sign * d
        if (rng.random() < 0.5) if first is None else (first < 0):
            co = -co
    else:                                                    # in_zero / out_zero: not close to co[0], (not) close to 0
        factor = 1.0 - BOUND_MARGIN if kind == "in_zero" else 1.0 + BOUND_MARGIN
        co = rng.uniform(-0.9e-8, 0.9e-8, n_src)
        co[0] = factor * 1e-8
        if n_src > 1:
            co[int(rng.integers(1, n_src))] = -0.95e-8
    if first is not None and kind in ("walk", "fast_up", "fast_down"):
        co = co - co[0] + first
    co = f(co)
    if first is not None:
        co[0] = first
    if n_src > 1 and kind in ("walk", "fast_up", "fast_down") and min(bound_ratio(co, co[0]), bound_ratio(co, 0.0)) < 10.0:
        return source_row(rng, kind, n_src, dtype, sgan_dt, first)       # a walk that barely moved: far from the bounds only
    return kind, co


def bound_ratio(co, b):
    """max |co_i - b| over the bound of np.allclose(co, b)."""
    return float(np.max(np.abs(np.asarray(co, dtype=np.float64) - b)) / (1e-8 + 1e-5 * abs(b)))


def check_row_kind(kind, co):
    """The generated row is what its kind says (so the generator cannot drift): bound classes within 10 % of
    BOUND_MARGIN of their place, and the constant flag that follows."""
    lo, hi = 0.9 * BOUND_MARGIN, 1.1 * BOUND_MARGIN
    if len(co) == 1:
        assert row_is_constant(co)
        return
    if kind in ("in_first", "out_first"):
        r = bound_ratio(co, co[0]) - 1.0
        assert (-hi <= r <= -lo) if kind == "in_first" else (lo <= r <= hi), (kind, r)
        assert not close_to(co, 0.0) and row_is_constant(co) == (kind == "in_first")
    elif kind in ("edge_out_away", "edge_in_toward"):
        r = bound_ratio(co, co[0]) - 1.0
        assert 0.8 * EDGE_MARGIN <= (r if kind == "edge_out_away" else -r) <= 1.2 * EDGE_MARGIN, (kind, r)
        assert row_is_constant(co) == (kind == "edge_in_toward")
        # with the bound taken from the value instead of from co[0] the row would be classified the other way
        assert bool(np.all(np.abs(co - co[0]) <= 1e-8 + 1e-5 * np.abs(co))) == (kind == "edge_out_away")
    elif kind in ("in_zero", "out_zero"):
        r = bound_ratio(co, 0.0) - 1.0
        assert (-hi <= r <= -lo) if kind == "in_zero" else (lo <= r <= hi), (kind, r)
        assert not close_to(co, co[0]) and row_is_constant(co) == (kind == "in_zero")
    elif kind in ("constant", "zeros"):
        assert row_is_constant(co)
    else:
        assert not row_is_constant(co)
        if kind != "walk" and len(co) >= 2:
            v = tail_velocity(co, 1.0, clamp=False)          # sign only
            assert (v > 0) == (kind == "fast_up")


# staleness classes: name -> staleness for a given (sgan_dt, sim_dt); "tie" needs sgan_dt a multiple of sim_dt
STALENESS = {
    "zero": lambda sg, sd, rng: 0.0,
    "tie": lambda sg, sd, rng: float(rng.integers(1, 4)) * sd,                        # a multiple of sim_dt: knot ties
    "generic": lambda sg, sd, rng: float(rng.uniform(0.01, 0.9) * sg),
    "past_first": lambda sg, sd, rng: sg * float(rng.choice([1.0, 1.5, 2.0, 3.25])),   # >= sgan_dt: targets before ts(0)
    "negative": lambda sg, sd, rng: -sd * float(rng.choice([1.0, 2.5, 4.0])),          # ... even with an anchor
    "long": lambda sg, sd, rng: 1.3,
}

# (sgan_dt, sim_dt, plan_horizon)
PARAM_SETS = ((0.4, 0.1, 5.0), (0.4, 0.1, 3.0), (0.4, 0.02, 5.0), (0.5, 0.25, 4.0), (0.4, 0.13, 6.5), (0.3, 0.04, 10.0))


def is_multiple(a, b):
    r = a / b
    return abs(r - round(r)) < 1e-9


def sources_tensor(rng, S, L, P, with_anchor, dtype, sgan_dt):
    """pred [S, L, P, 2] in dtype, anchor [P, 2] float64 or None, kinds [S, P, 2]: every (sample, pedestrian, axis) row
    of its own kind, the kinds cycling so that all are present once there are enough rows."""
    pred = np.zeros((S, L, P, 2), dtype=dtype)
    anchor = np.zeros((P, 2)) if with_anchor else None
    kinds = np.empty((S, P, 2), dtype=object)
    n_src = L + (1 if with_anchor else 0)
    start = int(rng.integers(0, len(ROW_KINDS)))
    for p in range(P):
        for ax in range(2):
            for s in range(S):
                kind = ROW_KINDS[(start + (s * P + p) * 2 + ax) % len(ROW_KINDS)]
                if rng.random() < 0.35 or (p == 0 and ax == 0):      # one row that differs in every sample: the samples'
                    kind = "walk"                                      # distances to their mean are then distinct
                first = anchor[p, ax] if with_anchor and s > 0 else None
                kind, co = source_row(rng, kind, n_src, dtype, sgan_dt, first)
                if with_anchor:
                    anchor[p, ax] = co[0]
                    pred[s, :, p, ax] = co[1:]
                else:
                    pred[s, :, p, ax] = co
                kinds[s, p, ax] = kind
    return pred, anchor, kinds


def pairwise_cases(axes, valid, seed, pool=3000):
    """A seeded greedy pairwise selection: dictionaries over ``axes`` (name -> values) such that every pair of values
    of two axes that some valid combination holds is held by a chosen one."""
    rng = np.random.default_rng(seed)
    names = list(axes)
    cands = []
    for _ in range(pool):
        c = {n: axes[n][int(rng.integers(0, len(axes[n])))] for n in names}
        if valid(c):
            cands.append(c)
    pairs_of = lambda c: {(a, c[a], b, c[b]) for i, a in enumerate(names) for b in names[i + 1:]}
    todo = set().union(*(pairs_of(c) for c in cands))
    chosen = []
    while todo:
        best = max(cands, key=lambda c: len(pairs_of(c) & todo))
        gain = pairs_of(best) & todo
        assert gain
        todo -= gain
        chosen.append(best)
    return chosen


RESAMPLE_AXES = dict(
    dtypes=(("f32", "f32"), ("f32", "f64"), ("f64", "f32"), ("f64", "f64")),
    tmajor=(False, True), device=(False, True), anchor=(False, True), current=(False, True),
    S=(1, 2, 20, 64), P=(1, 63, 64, 65, 300, 3000), L=(1, 2, 3, 12, 32),
    stale=tuple(STALENESS), params=tuple(range(len(PARAM_SETS))))


def resample_case_valid(c):
    sg, sd, h = PARAM_SETS[c["params"]]
    T = n_dense(sg, sd, h, c["L"]) + (1 if c["current"] else 0)
    if T > MAX_NT:
        return False
    if c["stale"] == "tie" and not is_multiple(sg, sd):
        return False
    return c["S"] * c["P"] * T <= 10_000_000               # points: the largest tensors stay below 160 MB


def resample_cases(seed=2024):
    return pairwise_cases(RESAMPLE_AXES, resample_case_valid, seed)


def build_resample_case(c, index):
    """The arrays of one pairwise case: dict with pred, anchor, current, staleness, kinds and the parameters."""
    rng = np.random.default_rng(100_000 + index)
    sg, sd, h = PARAM_SETS[c["params"]]
    in_dt = np.float32 if c["dtypes"][0] == "f32" else np.float64
    out_dt = np.float32 if c["dtypes"][1] == "f32" else np.float64
    pred, anchor, kinds = sources_tensor(rng, c["S"], c["L"], c["P"], c["anchor"], in_dt, sg)
    current = rng.uniform(-100, 100, (c["P"], 2)) if c["current"] else None
    return dict(pred=pred, anchor=anchor, current=current, staleness=STALENESS[c["stale"]](sg, sd, rng), kinds=kinds,
                sgan_dt=sg, sim_dt=sd, plan_horizon=h, in_dtype=in_dt, out_dtype=out_dt)


def within_one_ulp_f32(got, want64):
    """got (float32) is the float32 rounding of want64 or one of its two float32 neighbours."""
    w = np.asarray(want64).astype(np.float32)
    g = np.asarray(got)
    assert g.dtype == np.float32
    return (g == w) | (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))


def assert_matches_restatement(got, want64, label):
    """The tolerances of the device tests: float64 output rtol = atol = 1e-12 (the bar the entry points are already held
    to; contraction moves a value of at most 100 m by a few 1e-14), float32 output the rounded restatement +- 1 ulp."""
    assert got.shape == want64.shape, (label, got.shape, want64.shape)
    if got.dtype == np.float32:
        ok = within_one_ulp_f32(got, want64)
        assert ok.all(), f"{label}: {int((~ok).sum())} of {ok.size} float32 values off by more than one ulp; first at " \
                         f"{tuple(np.argwhere(~ok)[0])}: {got[tuple(np.argwhere(~ok)[0])]!r} vs {want64[tuple(np.argwhere(~ok)[0])]!r}"
    else:
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want64, rtol=1e-12, atol=1e-12, err_msg=label)


def first_two_gap(d):
    """Relative gap between the two smallest of d (inf for a single value)."""
    s = np.sort(np.asarray(d, dtype=np.float64))
    return math.inf if len(s) < 2 else float((s[1] - s[0]) / max(s[0], 1e-300))
