"""Shared by the encounter-fidelity tests (fot_fidelity_eval, integrated_path_planning_amd/fidelity.py): a NumPy restatement
of the separation series, the avoidance onset and the roll-out error in plain elementwise operations (no dot, no 1-D
norm: every product, sum and quotient is one NumPy operation, hence one rounding, exactly the sequence of
csrc/fot_fidelity.hpp), the reference-shaped Python loop, the bounds against the reference, generators of encounters, and
the emulation's file formats (tests/emu/fot_fidelity_emu.cpp)."""
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fidelity", "cases.npz")

ENC_DT = np.dtype([("closest", "<f8"), ("err_sum", "<f8"), ("err_count", "<i8"), ("n_onset", "<i4"), ("closest_step", "<i4")])
assert ENC_DT.itemsize == 32
DEFAULTS = dict(accel_threshold=0.3, max_distance=5.0)
MIN_DIST = 1e-9
DTS = (0.4, 0.1, 1 / 23.98)

# ---- the bounds ---------------------------------------------------------------------------------------------------------------
# Restatement against the reference: np.dot of two pairs and the 1-D norm may fuse one multiply-add, everything in front of
# them is the same roundings -- onset distances and away within 4 * 2^-52 relative.  A sum of `count` non-negative terms in
# two different orders differs by at most count * 2^-52 * sum.
EPS = 2.0 ** -52
REL_FUSED = 4 * EPS
# Device against the restatement: the same IEEE sequence; held to 2 ulp.
ULPS = 2
# A decision is left out of the comparison only inside the project's band around its threshold.
BAND = 1e-9


def sum_tol(count, total):
    return float(count) * EPS * abs(float(total))


def ulp_diff(a, b):
    """the largest |a - b| in units of the larger magnitude's ulp (0 where both are NaN or equal)"""
    a, b = np.asarray(a, float).reshape(-1), np.asarray(b, float).reshape(-1)
    assert a.shape == b.shape
    both_nan = np.isnan(a) & np.isnan(b)
    same = both_nan | (a == b)
    if same.all():
        return 0.0
    assert not np.any(np.isnan(a[~same]) | np.isnan(b[~same])), "a NaN on one side only"
    with np.errstate(invalid="ignore"):
        d = np.abs(a[~same] - b[~same]) / np.spacing(np.maximum(np.abs(a[~same]), np.abs(b[~same])))
    return float(np.max(d))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def dist(dx, dy):
    """sqrt(dx dx + dy dy): square, square, add, root"""
    return np.sqrt(dx * dx + dy * dy)


def gradient(f, dt):
    """np.gradient(f, dt, axis=0) with scalar spacing, written out"""
    f = np.asarray(f, float)
    out = np.empty_like(f)
    out[1:-1] = (f[2:] - f[:-2]) / (2.0 * dt)
    out[0] = (f[1] - f[0]) / dt
    out[-1] = (f[-1] - f[-2]) / dt
    return out


def distances(ego_xy, ped_xy):
    """[T, N] centre distances"""
    ego_xy, ped_xy = np.asarray(ego_xy, float), np.asarray(ped_xy, float)
    rel = ped_xy - ego_xy[:, None, :]
    return dist(rel[..., 0], rel[..., 1])


def separation(ego_xy, ped_xy):
    ego_xy, ped_xy = np.asarray(ego_xy, float), np.asarray(ped_xy, float)
    steps = (len(ego_xy), len(ped_xy))
    if steps[0] != steps[1]:
        raise ValueError(f"ego_xy T={steps[0]} != ped_xy T={steps[1]}")
    return np.min(distances(ego_xy, ped_xy), axis=1, initial=np.inf)      # (nobody there: +inf)


def onset_terms(ego_xy, ped_xy, ped_vel=None, dt=0.4, max_distance=5.0):
    """(dist, away, in_range), each [T, N]; away is NaN outside the range.  T >= 2."""
    ego_xy, ped_xy = np.asarray(ego_xy, float), np.asarray(ped_xy, float)
    vel = gradient(ped_xy, dt) if ped_vel is None else np.asarray(ped_vel, float)
    acc = gradient(vel, dt)
    rel = ped_xy - ego_xy[:, None, :]
    d = dist(rel[..., 0], rel[..., 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        in_range = ~(d < MIN_DIST) & ~(d > max_distance)
        away = acc[..., 0] * (rel[..., 0] / d) + acc[..., 1] * (rel[..., 1] / d)
    return d, np.where(in_range, away, np.nan), in_range


def onset(ego_xy, ped_xy, ped_vel=None, dt=0.4, accel_threshold=0.3, max_distance=5.0):
    """Per pedestrian: (step, -1 without onset; distance, NaN without; away there; in the band).  A pedestrian is in the
    band when at some step up to its onset |away - thr| / |thr| or |dist - max| / |max| is below BAND."""
    ped_xy = np.asarray(ped_xy, float)
    T, N, _ = ped_xy.shape
    step, where, away_at, band = np.full(N, -1, np.int32), np.full(N, np.nan), np.full(N, np.nan), np.zeros(N, bool)
    if T < 2 or N == 0:
        return step, where, away_at, band
    d, away, in_range = onset_terms(ego_xy, ped_xy, ped_vel, dt, max_distance)
    with np.errstate(invalid="ignore"):
        hit = in_range & (away > accel_threshold)
        near = (in_range & (np.abs(away - accel_threshold) <= BAND * abs(accel_threshold))) | \
               (np.abs(d - max_distance) <= BAND * abs(max_distance))
    any_hit = hit.any(axis=0)
    first = np.argmax(hit, axis=0)
    cols = np.arange(N)
    step[any_hit] = first[any_hit]
    where[any_hit] = d[first[any_hit], cols[any_hit]]
    away_at[any_hit] = away[first[any_hit], cols[any_hit]]
    upto = np.where(any_hit, first, T - 1)
    band = (near & (np.arange(T)[:, None] <= upto[None, :])).any(axis=0)
    return step, where, away_at, band


def onset_loop(ego_xy, ped_xy, ped_vel=None, dt=0.4, accel_threshold=0.3, max_distance=5.0):
    """The same rule as the reference's shape has it: a Python double loop over (pedestrian, step).  Returns the distances
    of the pedestrians that evade.  (What scripts/fidelity_bench.py times as the host loop.)"""
    ego_xy, ped_xy = np.asarray(ego_xy, float), np.asarray(ped_xy, float)
    T, N, _ = ped_xy.shape
    if T < 2 or N == 0:
        return np.array([])
    vel = gradient(ped_xy, dt) if ped_vel is None else np.asarray(ped_vel, float)
    acc = gradient(vel, dt)
    def evades(t, j):
        """(whether pedestrian j evades at step t, its distance there), one scalar at a time"""
        rx, ry = ped_xy[t, j, 0] - ego_xy[t, 0], ped_xy[t, j, 1] - ego_xy[t, 1]
        d = float(np.sqrt(rx * rx + ry * ry))
        if d < MIN_DIST or d > max_distance:
            return False, d
        return float(acc[t, j, 0] * (rx / d) + acc[t, j, 1] * (ry / d)) > accel_threshold, d

    firsts = (next((d for hit, d in (evades(t, j) for t in range(T)) if hit), None) for j in range(N))
    return np.array([d for d in firsts if d is not None])


def ped_error(ego_xy, ped_xy, truth_xy, interaction_distance=None):
    """Per pedestrian: the error summed over the steps 1 .. T-1 in ascending order, and whether it is kept."""
    ped_xy, truth_xy = np.asarray(ped_xy, float), np.asarray(truth_xy, float)
    T, N, _ = ped_xy.shape
    diff = ped_xy - truth_xy
    err = dist(diff[..., 0], diff[..., 1])
    total = np.zeros(N)
    for t in range(1, T):
        total = total + err[t]
    keep = np.ones(N, bool)
    if interaction_distance is not None and not np.isnan(interaction_distance) and N:
        keep = np.min(distances(ego_xy, truth_xy), axis=0) <= interaction_distance
    return total, keep, err


def record(ego_xy, ped_xy, ped_vel=None, truth_xy=None, dt=0.4, accel_threshold=0.3, max_distance=5.0,
           interaction_distance=None):
    """(ENC_DT record, series [T], onset distance [N], onset step [N], away [N], band [N]) of one encounter"""
    ped_xy = np.asarray(ped_xy, float)
    T, N, _ = ped_xy.shape
    series = separation(ego_xy, ped_xy)
    step, where, away_at, band = onset(ego_xy, ped_xy, ped_vel, dt, accel_threshold, max_distance)
    r = np.zeros((), ENC_DT)
    closest = float(np.min(series))
    r["closest"] = closest
    r["closest_step"] = -1 if (N == 0 or np.isnan(closest)) else int(np.argmax(series == closest))
    r["n_onset"] = int(np.sum(step >= 0))
    if truth_xy is not None:
        total, keep, _ = ped_error(ego_xy, ped_xy, truth_xy, interaction_distance)
        s = 0.0
        for j in range(N):
            if keep[j]:
                s = s + float(total[j])
        r["err_sum"], r["err_count"] = s, (T - 1) * int(np.sum(keep))
    return r, series, where, step, away_at, band


def evaluate(encounters, with_vel=False, truth=None, **kw):
    """The restatement of one fot_fidelity_eval call: (records [n], series [steps], onset distance [sum N], onset step
    [sum N], band [sum N]).  encounters: dictionaries with ego_xy, ped_xy, dt (and ped_vel); truth: one array per encounter."""
    recs, series, where, step, band = [], [], [], [], []
    for i, e in enumerate(encounters):
        r, s, w, st, _, b = record(e["ego_xy"], e["ped_xy"], e["ped_vel"] if with_vel else None,
                                   None if truth is None else truth[i], dt=e["dt"], **kw)
        recs.append(r); series.append(s); where.append(w); step.append(st); band.append(b)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return (np.array(recs, ENC_DT).reshape(len(recs)), cat(series, np.float64), cat(where, np.float64), cat(step, np.int32),
            cat(band, bool))


def ks_statistic(a, b):
    """the two-sample KS statistic of finite 1-D samples: the largest difference of the empirical CDFs.  The true value
    is a multiple of 1 / lcm(n_a, n_b); up to 10000 samples a side the difference of the two rounded quotients is put back
    on that lattice (scipy's exact mode does the same, and takes over above that size without it)."""
    a, b = np.sort(np.asarray(a, float)), np.sort(np.asarray(b, float))
    both = np.concatenate([a, b])
    d = float(np.max(np.abs(np.searchsorted(a, both, side="right") / a.size - np.searchsorted(b, both, side="right") / b.size)))
    if max(a.size, b.size) <= 10000:
        lcm = (a.size // int(np.gcd(a.size, b.size))) * b.size
        d = int(np.round(d * lcm)) * 1.0 / lcm
    return d


# ---- encounters -------------------------------------------------------------------------------------------------------------
def random_encounter(rng, T, N, dt, vel=True):
    """An ego driving straight at 1 .. 4 m/s and N pedestrians that start 0.8 .. 9 m from its path and walk at about
    1.3 m/s under a random acceleration of about 0.8 m/s^2 per step: some evade in range, some never do."""
    t = np.arange(T) * dt
    heading = rng.uniform(0, 2 * np.pi)
    speed = rng.uniform(1.0, 4.0)
    start = rng.uniform(-20.0, 20.0, 2)
    ego = start + np.outer(t, speed * np.array([np.cos(heading), np.sin(heading)]))
    along = rng.uniform(0.0, max(t[-1], dt) * speed, N)
    side = rng.uniform(0.8, 9.0, N) * rng.choice([-1.0, 1.0], N)
    p0 = start + np.outer(along, [np.cos(heading), np.sin(heading)]) + np.outer(side, [-np.sin(heading), np.cos(heading)])
    v0 = rng.normal(0.0, 0.9, (N, 2))
    acc = rng.normal(0.0, 0.8, (T, N, 2))
    v = v0[None] + np.cumsum(acc, axis=0) * dt
    ped = p0[None] + np.cumsum(v, axis=0) * dt
    out = dict(ego_xy=ego, ped_xy=ped, dt=float(dt))
    if vel:
        out["ped_vel"] = v + rng.normal(0.0, 0.02, v.shape)       # a recorded velocity: not the positions' gradient
    return out


def rollout_of(enc):
    """A stand-in roll-out of an encounter from its `drift` [2, N, 2]: the recording plus drift[0] t + drift[1] t^2 (t in
    seconds) -- the recording's first frame, then a path of its own with another acceleration.  Products and sums only:
    the same bits wherever it is formed."""
    ped = np.asarray(enc["ped_xy"], float)
    t = (np.arange(ped.shape[0]) * enc["dt"])[:, None, None]
    return ped + (t * enc["drift"][0][None] + (t * t) * enc["drift"][1][None])


def with_drift(rng, enc, scale=0.25):
    enc["drift"] = rng.normal(0.0, scale, (2, np.shape(enc["ped_xy"])[1], 2))
    return enc


def fuzz(seed, n, t_range=(2, 70), n_range=(0, 12)):
    rng = np.random.default_rng(seed)
    return [random_encounter(rng, int(rng.integers(t_range[0], t_range[1] + 1)), int(rng.integers(n_range[0], n_range[1] + 1)),
                             DTS[int(rng.integers(0, 3))]) for _ in range(n)]


def axis_encounter(px, dt=0.5, py=None):
    """The ego at the origin and one pedestrian on the x axis at px [T] (py [T]: on the y axis instead)"""
    a = np.asarray(px if py is None else py, float)
    ped = np.zeros((len(a), 1, 2))
    ped[:, 0, 0 if py is None else 1] = a
    return dict(ego_xy=np.zeros((len(a), 2)), ped_xy=ped, dt=dt, ped_vel=gradient(ped, dt))


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def load_cases():
    with np.load(GOLDEN, allow_pickle=False) as z:
        fix = {k: z[k] for k in z.files}
    fix["meta"] = json.loads(str(fix["meta"]))
    return fix


def golden_encounters(fix, group):
    """the encounters of a group of the fixture, as dictionaries (with the roll-out's `drift`: rollout_of)"""
    out = []
    for i in range(fix["meta"]["groups"][group]):
        k = f"{group}_{i}_"
        e = dict(ego_xy=fix[k + "ego_xy"], ped_xy=fix[k + "ped_xy"], dt=float(fix[k + "dt"]))
        for opt in ("ped_vel", "drift"):
            if k + opt in fix:
                e[opt] = fix[k + opt]
        out.append(e)
    return out


# ---- the emulation's files (tests/emu/fot_fidelity_emu.cpp) ----------------------------------------------------------------------
def write_emu_case(path, encounters, with_vel=False, truth=None, accel_threshold=0.3, max_distance=5.0,
                   interaction_distance=None, step_off=None, n_ped=None, dt=None, n_enc=None):
    steps = [len(e["ego_xy"]) for e in encounters]
    so = np.concatenate([[0], np.cumsum(steps)]).astype(np.int32) if step_off is None else np.asarray(step_off, np.int32)
    npd = np.array([np.shape(e["ped_xy"])[1] for e in encounters], np.int32) if n_ped is None else np.asarray(n_ped, np.int32)
    dts = np.array([e["dt"] for e in encounters], np.float64) if dt is None else np.asarray(dt, np.float64)
    n = len(encounters) if n_enc is None else n_enc
    flat = lambda arrs: np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in arrs]) if len(arrs) else np.zeros(0)
    with open(path, "wb") as f:
        f.write(struct.pack("<3d", accel_threshold, max_distance, np.nan if interaction_distance is None else interaction_distance))
        f.write(struct.pack("<4i", n, int(with_vel), int(truth is not None), 0))
        f.write(so.tobytes()); f.write(npd.tobytes()); f.write(dts.tobytes())
        f.write(flat([e["ego_xy"] for e in encounters]).tobytes())
        f.write(flat([e["ped_xy"] for e in encounters]).tobytes())
        if with_vel:
            f.write(flat([e["ped_vel"] for e in encounters]).tobytes())
        if truth is not None:
            f.write(flat(truth).tobytes())


def read_emu_out(path):
    """(code, records, series, onset distance, onset step, away)"""
    with open(path, "rb") as f:
        raw = f.read()
    code, n, steps, peds = struct.unpack_from("<4i", raw, 0)
    if code != 0:
        return code, None, None, None, None, None
    o = 16
    rec = np.frombuffer(raw, ENC_DT, n, o); o += 32 * n
    series = np.frombuffer(raw, "<f8", steps, o); o += 8 * steps
    where = np.frombuffer(raw, "<f8", peds, o); o += 8 * peds
    away = np.frombuffer(raw, "<f8", peds, o); o += 8 * peds
    step = np.frombuffer(raw, "<i4", peds, o); o += 4 * peds
    assert o == len(raw)
    return code, rec, series, where, step, away


# ---- designed encounters: the onset where the test puts it -----------------------------------------------------------------------
def designed(T, N, evaders, near_steps, dt=0.4, accel=1.0, gap=3.0):
    """N pedestrians walking along +x under the constant acceleration `accel` (x = accel t^2 / 2, rows 0.01 m apart in y):
    np.gradient of a parabola gives `accel` inside and accel / 2 at both ends, so with accel = 1 `away` exceeds 0.3 at every
    step the ego is in range.  The pedestrians not in `evaders` walk 100 m ahead and are never in range.  The ego stands
    `gap` behind the evaders at the steps of `near_steps` and 20 m behind otherwise: an evader's onset is the first near step.
    ped_vel is a recorded constant velocity (acceleration 0: no onset on that branch)."""
    t = np.arange(T) * dt
    x = 0.5 * accel * t * t
    ped = np.zeros((T, N, 2))
    ped[:, :, 0] = x[:, None] + 100.0
    ped[:, :, 1] = 0.01 * np.arange(N)[None, :]
    for j in evaders:
        ped[:, j, 0] = x
    behind = np.full(T, 20.0)
    behind[list(near_steps)] = gap
    ego = np.stack([x - behind, np.zeros(T)], axis=1)
    vel = np.zeros_like(ped)
    vel[..., 0] = 1.0
    return dict(ego_xy=ego, ped_xy=ped, dt=float(dt), ped_vel=vel)


def edge_encounters():
    """[(name, encounter, expected onsets from positions, expected onsets with ped_vel)], each expectation a dictionary
    {pedestrian: step} or None (whatever the restatement says): the smallest shapes that can go wrong"""
    rng = np.random.default_rng(28)
    out = []
    for T in (1, 2, 3, 63, 64, 65, 129):
        out.append((f"T{T}", random_encounter(rng, T, 3, 0.4), None, None))
    for N in (0, 1, 63, 64, 65, 257):
        out.append((f"N{N}", random_encounter(rng, 5, N, 0.1), None, None))
    out.append(("onset_first_step", designed(9, 2, [1], range(0, 9)), {1: 0}, {}))
    out.append(("onset_last_step", designed(9, 2, [0], [8]), {0: 8}, {}))
    # two steps: both ends apply and there is no interior -- the positions' acceleration is 0 whatever they are, a
    # recorded velocity that gains 1 m/s has 1 / dt at both steps
    for name, near in (("onset_T2_first", [0, 1]), ("onset_T2_last", [1])):
        e = designed(2, 1, [0], near)
        e["ped_vel"][1, :, 0] = 2.0
        out.append((name, e, {}, {0: near[0]}))
    for k in (63, 64, 65):
        out.append((f"onset_step_{k}", designed(70, 3, [0, 2], range(k, 70), dt=0.1), {0: k, 2: k}, {}))
    out.append(("onset_lanes_63_64", designed(6, 257, [63, 64], [3, 4]), {63: 3, 64: 3}, {}))
    out.append(("onset_twice", designed(20, 2, [0], [4, 5, 12, 13]), {0: 4}, {}))
    out.append(("one_step", random_encounter(rng, 1, 4, 0.4), None, None))
    out.append(("long", random_encounter(rng, 2000, 2, 1 / 23.98), None, None))
    return out
