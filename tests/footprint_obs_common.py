"""Shared by the footprint re-verification tests (fot_footprint_recheck, fot_loop_footprint_*): the NumPy restatement of the
three observational geometries and of the heading reconstruction (the same NumPy operations the reference's functions apply,
so that it equals the golden answers bit for bit), the derived tolerance, case builders, and the emulation's file formats
(tests/emu/fot_footprint_obs_emu.cpp)."""
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "footprint_obs", "cases.npz")

DEFAULT_GEOM = dict(vehicle_length=4.5, vehicle_width=2.0, n_circles=3, ped_radius=0.2, ego_radius=1.0)
MOVING_EPS = 1e-4
STEP_DT = np.dtype([("legacy", "<f8"), ("multi", "<f8"), ("rect", "<f8")])
RECORD_F64 = ("legacy_min_dist", "multi_min_dist", "multi_clearance", "rect_min_surface_dist", "rect_clearance")
RECORD_I32 = ("legacy_collision_steps", "multi_violation_steps", "rect_violation_steps", "steps", "steps_with_peds")
RECORD_DT = np.dtype([(n, "<f8") for n in RECORD_F64] + [(n, "<i4") for n in RECORD_I32 + ("_pad",)])
assert STEP_DT.itemsize == 24 and RECORD_DT.itemsize == 64

# ---- the tolerance against the reference / the restatement on identical inputs ---------------------------------------------
# Both sides take the same float64 inputs; they differ in the last bits of cos / sin / atan2 / hypot and in whether a
# product and the sum behind it round once or twice.  A value's chain, with M the largest coordinate magnitude (every
# intermediate is at most 2 M): px - x (1), the two products and their sum of the vehicle frame or the circle centre (3, each
# carrying the <= 1 ulp of cos / sin: 2 more), |.| - half (1), the squares and their sum or hypot (3), the root (1), the
# minimum (0), the clearance's subtraction (1) -- 12 roundings, under 16 on each side, each at most 2^-53 (2 M) = 2^-52 M:
# 2 sides x 16 x 2^-52 M = 32 x 2^-52 M; the bound is twice that.
DIST_ULPS = 64                                    # |got - want| <= 64 * 2^-52 * max(1, M)
# a heading: dx, dy are exact or one rounding each; atan2 of the two libraries within 1 ulp of the true value each, its
# condition number in (dx, dy) is at most 1: under 8 ulp of pi
YAW_TOL = 8 * 2.0 ** -52 * np.pi


def dist_tol(M):
    return DIST_ULPS * 2.0 ** -52 * max(1.0, float(M))


def magnitude(*arrays):
    """the largest finite coordinate magnitude of a case"""
    m = 0.0
    for a in arrays:
        a = np.asarray(a, float)
        if a.size:
            m = max(m, float(np.max(np.abs(a[np.isfinite(a)]), initial=0.0)))
    return m


# ---- the geometry -----------------------------------------------------------------------------------------------------------
def circle_cover(length, width, n):
    """offsets [n] and radius of the n-circle cover of the length x width rectangle"""
    seg = length / n
    return -length / 2 + seg / 2 + seg * np.arange(n), float(np.hypot(seg / 2, width / 2))


def thresholds(geom):
    """(legacy, multi, rect) thresholds of a geometry dictionary"""
    g = dict(DEFAULT_GEOM, **(geom or {}))
    _, radius = circle_cover(g["vehicle_length"], g["vehicle_width"], g["n_circles"])
    legacy = g["legacy_radius"] if "legacy_radius" in g else g["ego_radius"] + g["ped_radius"]
    return legacy, radius + g["ped_radius"], g["ped_radius"]


# ---- the restatement -------------------------------------------------------------------------------------------------------
def step_values(x, y, yaw, peds, geom=None):
    """(legacy, multi, rect) of one pose against its pedestrians [P, 2]; +inf three times without any"""
    g = dict(DEFAULT_GEOM, **(geom or {}))
    peds = np.asarray(peds, dtype=float)
    if peds.size == 0:
        return np.inf, np.inf, np.inf
    peds = peds.reshape(-1, 2)
    offsets, _ = circle_cover(g["vehicle_length"], g["vehicle_width"], g["n_circles"])
    here = np.array([x, y])
    legacy = float(np.min(np.linalg.norm(peds - here, axis=1)))
    heading = np.array([np.cos(yaw), np.sin(yaw)])
    centres = np.array([x, y]) + offsets[:, None] * heading
    multi = float(np.min(np.linalg.norm(peds[None, :, :] - centres[:, None, :], axis=2)))
    c, s = np.cos(yaw), np.sin(yaw)
    turn = np.array([[c, s], [-s, c]])
    local = (peds - np.array([x, y])) @ turn.T
    over_x = np.maximum(np.abs(local[:, 0]) - g["vehicle_length"] / 2, 0.0)
    over_y = np.maximum(np.abs(local[:, 1]) - g["vehicle_width"] / 2, 0.0)
    rect = float(np.min(np.hypot(over_x, over_y)))
    return legacy, multi, rect


def heading_terms(x, y):
    """(dx, dy, moving, raw heading) of a trajectory's positions"""
    dx, dy = np.gradient(np.asarray(x, float)), np.gradient(np.asarray(y, float))
    return dx, dy, np.hypot(dx, dy) > MOVING_EPS, np.arctan2(dy, dx)


def reconstruct_heading(x, y):
    """The heading of every step from the finite differences of its positions: a standing step holds the last moving
    heading, the steps in front of the first moving one take that first heading, all zeros when nothing moves."""
    _, _, moving, raw = heading_terms(x, y)
    if not moving.any():
        return np.zeros_like(raw)
    src = np.maximum.accumulate(np.where(moving, np.arange(len(raw)), -1))
    return raw[np.where(src >= 0, src, int(np.argmax(moving)))]


def series_of(x, y, yaw, ped_off, ped_xy, geom=None):
    """STEP_DT [steps] of one trajectory (ped_off relative to ped_xy)"""
    out = np.zeros(len(x), STEP_DT)
    for i in range(len(x)):
        out[i] = step_values(x[i], y[i], yaw[i], ped_xy[ped_off[i]:ped_off[i + 1]], geom)
    return out


def fold(series, n_peds, geom=None):
    """RECORD_DT record of a trajectory's per-step values; n_peds [steps]: the pedestrians of each step"""
    t_legacy, t_multi, t_rect = thresholds(geom)
    r = np.zeros((), RECORD_DT)
    mins = [float(np.min(series[k])) if len(series) else np.inf for k in ("legacy", "multi", "rect")]
    r["legacy_min_dist"], r["multi_min_dist"], r["rect_min_surface_dist"] = mins
    r["multi_clearance"] = mins[1] - t_multi
    r["rect_clearance"] = mins[2] - t_rect
    r["legacy_collision_steps"] = int(np.sum(series["legacy"] < t_legacy))
    r["multi_violation_steps"] = int(np.sum(series["multi"] < t_multi))
    r["rect_violation_steps"] = int(np.sum(series["rect"] < t_rect))
    r["steps"] = len(series)
    r["steps_with_peds"] = int(np.sum(np.asarray(n_peds) > 0))
    return r


def recheck(case, geom=None, reconstruct=False):
    """(records [n_traj], series [steps], yaw [steps]) of a case dictionary (step_off, xy, yaw, ped_off, ped_xy)"""
    step_off, xy, ped_off, ped_xy = case["step_off"], case["xy"], case["ped_off"], case["ped_xy"]
    yaw = np.array(case["yaw"], float) if not reconstruct else np.zeros(len(xy))
    recs = np.zeros(len(step_off) - 1, RECORD_DT)
    series = np.zeros(len(xy), STEP_DT)
    for t, (lo, hi) in enumerate(zip(step_off[:-1], step_off[1:])):
        if reconstruct:
            yaw[lo:hi] = reconstruct_heading(xy[lo:hi, 0], xy[lo:hi, 1])
        for i in range(lo, hi):
            series[i] = step_values(xy[i, 0], xy[i, 1], yaw[i], ped_xy[ped_off[i]:ped_off[i + 1]], geom)
        recs[t] = fold(series[lo:hi], np.diff(ped_off[lo:hi + 1]), geom)
    return recs, series, yaw


def fold_series(case, series, geom=None):
    """the records of a case from given per-step values (the host's fold of `series`)"""
    step_off, ped_off = case["step_off"], case["ped_off"]
    return np.array([fold(series[lo:hi], np.diff(ped_off[lo:hi + 1]), geom) for lo, hi in zip(step_off[:-1], step_off[1:])],
                    dtype=RECORD_DT)


# ---- comparison ------------------------------------------------------------------------------------------------------------
def assert_close(got, want, tol, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same_inf = np.isinf(got) == np.isinf(want)
    assert same_inf.all() and np.array_equal(got[np.isinf(got)], want[np.isinf(want)]), f"{what}: infinities differ"
    fin = np.isfinite(want)
    diff = float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))
    assert diff <= tol, f"{what}: largest difference {diff:.3e} > {tol:.3e}"
    return diff


def assert_records_close(got, want, tol, what):
    worst = 0.0
    for k in RECORD_F64:
        worst = max(worst, assert_close(got[k], want[k], tol, f"{what} {k}"))
    for k in RECORD_I32:
        assert np.array_equal(got[k], want[k]), f"{what} {k}: {got[k]} != {want[k]}"
    return worst


def assert_series_close(got, want, tol, what):
    return max(assert_close(got[k], want[k], tol, f"{what} {k}") for k in STEP_DT.names)


# ---- cases -----------------------------------------------------------------------------------------------------------------
def make_case(trajs):
    """A case dictionary from [(x [n], y [n], yaw [n], [peds_i [P_i, 2] per step])]"""
    step_off = np.concatenate([[0], np.cumsum([len(t[0]) for t in trajs])]).astype(np.int32)
    xy = np.concatenate([np.stack([np.asarray(t[0], float), np.asarray(t[1], float)], axis=1) for t in trajs])
    yaw = np.concatenate([np.asarray(t[2], float) for t in trajs])
    peds = [np.asarray(p, float).reshape(-1, 2) for t in trajs for p in t[3]]
    ped_off = np.concatenate([[0], np.cumsum([len(p) for p in peds])]).astype(np.int32)
    ped_xy = np.concatenate(peds) if peds else np.zeros((0, 2))
    return dict(step_off=step_off, xy=np.ascontiguousarray(xy), yaw=yaw, ped_off=ped_off, ped_xy=np.ascontiguousarray(ped_xy))


def sub_case(case, ts):
    """the trajectories `ts` of a case as a case of their own"""
    out = []
    for t in ts:
        lo, hi = case["step_off"][t], case["step_off"][t + 1]
        out.append((case["xy"][lo:hi, 0], case["xy"][lo:hi, 1], case["yaw"][lo:hi],
                    [case["ped_xy"][case["ped_off"][i]:case["ped_off"][i + 1]] for i in range(lo, hi)]))
    return make_case(out)


def drive(rng, n, speed=0.8, stand=(), start=(0.0, 0.0)):
    """n positions of a gently turning drive; stand: (first, last) step ranges in which the vehicle does not move"""
    heading = np.cumsum(rng.normal(0.0, 0.05, n)) + rng.uniform(-np.pi, np.pi)
    v = np.full(n, speed)
    for lo, hi in stand:
        v[lo:hi + 1] = 0.0
    x = start[0] + np.cumsum(v * np.cos(heading))
    y = start[1] + np.cumsum(v * np.sin(heading))
    return x, y, heading


def crowd_near(rng, x, y, counts, spread=6.0):
    """per step `counts[i]` pedestrians scattered around the pose"""
    return [np.stack([x[i] + rng.uniform(-spread, spread, c), y[i] + rng.uniform(-spread, spread, c)], axis=1)
            for i, c in enumerate(counts)]


def scan_case(seed=11):
    """Standstill across the chunk boundary at 256, lead-ins of 1 and 300 steps, a trajectory that never moves, lengths
    2, 3, 255, 256, 257 and 600 -- no pedestrians: the heading alone."""
    rng = np.random.default_rng(seed)
    trajs = []
    # (drive(): positions i - 1 .. hi coincide for a stand (i, hi), so the central difference is zero on steps i .. hi - 1)
    for n, stand in ((600, ((250, 263),)), (600, ((0, 1),)), (600, ((0, 300),)), (40, ((0, 39),)), (2, ()), (3, ()), (255, ()),
                     (256, ((254, 255),)), (257, ((254, 256),)), (600, ((100, 580),))):
        x, y, heading = drive(rng, n, stand=stand)
        trajs.append((x, y, heading, [np.zeros((0, 2))] * n))
    return make_case(trajs)


# ---- the golden fixture ----------------------------------------------------------------------------------------------------
def load_cases():
    z = np.load(GOLDEN, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def golden_case(fix, name):
    return {k: fix[f"{name}_{k}"] for k in ("step_off", "xy", "yaw", "ped_off", "ped_xy")}


# ---- the emulation's files -------------------------------------------------------------------------------------------------
def write_emu_case(path, case, geom=None, reconstruct=False, chunk=0, n_traj=None):
    g = dict(DEFAULT_GEOM, **(geom or {}))
    legacy = g["legacy_radius"] if "legacy_radius" in g else g["ego_radius"] + g["ped_radius"]
    n = len(case["step_off"]) - 1 if n_traj is None else n_traj
    with open(path, "wb") as f:
        f.write(struct.pack("<4d4i", g["vehicle_length"], g["vehicle_width"], g["ped_radius"], legacy, g["n_circles"], n,
                            0 if reconstruct else 1, chunk))
        f.write(np.ascontiguousarray(case["step_off"], "<i4").tobytes())
        f.write(np.ascontiguousarray(case["xy"], "<f8").tobytes())
        if not reconstruct:
            f.write(np.ascontiguousarray(case["yaw"], "<f8").tobytes())
        f.write(np.ascontiguousarray(case["ped_off"], "<i4").tobytes())
        f.write(np.ascontiguousarray(case["ped_xy"], "<f8").tobytes())


def read_emu_out(path):
    """(code, records, series, yaw, moving, offsets, radius); the arrays None for a refusal"""
    with open(path, "rb") as f:
        raw = f.read()
    code, n, steps, _ = struct.unpack_from("<4i", raw, 0)
    if code != 0:
        return code, None, None, None, None, None, None
    at = 16
    rec = np.frombuffer(raw, RECORD_DT, n, at); at += 64 * n
    series = np.frombuffer(raw, STEP_DT, steps, at); at += 24 * steps
    yaw = np.frombuffer(raw, "<f8", steps, at); at += 8 * steps
    moving = np.frombuffer(raw, np.uint8, steps, at).astype(bool); at += steps
    off = np.frombuffer(raw, "<f8", 8, at); at += 64
    radius = float(np.frombuffer(raw, "<f8", 1, at)[0])
    assert at + 8 == len(raw)
    return 0, rec, series, yaw, moving, off, radius
