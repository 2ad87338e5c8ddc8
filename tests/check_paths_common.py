"""The reference's external-path checks restated in NumPy, and the cases the check-path tests share.

FrenetPlanner._check_paths (frenet_planner.py:891-993), _apply_stop_distance_filter (:307-324), _curvature_feasible
(:995-1033), _path_collision_geometry (:1126-1179), _hits_static (:1181-1198), _hits_dynamic (:1200-1233) and the two
collision entries (:1049-1124), in the reference's operation order: np.hypot for the step length, np.sum(diff**2, axis=2),
np.round(t / dt).astype(int) with clip, and the bounding-box pre-filters with their NaN behaviour (np.min / np.max
propagate a NaN, and a NaN bound fails every comparison).  Independent of oracle/ and of the library; pinned to the
reference's own answers by tests/test_check_paths_common.py (tests/golden/check_paths/cases.npz).

Beside each answer the functions return the smallest relative margin |value - threshold| / |threshold| over every
comparison made on the path up to the deciding rule (every element of a rule, not only up to the first failing one: the
smaller margin).  The box pre-filters carry no margin of their own: a box is the path grown by the radius, so an
obstacle near a box face and able to hit is as near to the radius.  A case with a margin below BAND may be decided
either way by a re-association (sqrt of a sum of squares against np.hypot, the yaw step from products of sin / cos
against arctan2(sin, cos)).

A *path* is a dict of lists t, x, y, yaw, v, a, c, d, s (any may be shorter or longer than x).  A *call* is a dict
cfg / paths / static / dyn / dist / overrides / max_stop: one obstacle set and one set of limits for all its paths.
"""
import json
import math

import numpy as np

FIELDS = ("t", "x", "y", "yaw", "v", "a", "c", "d", "s")
CATEGORIES = ("max_speed_error", "max_accel_error", "max_curvature_error", "max_lat_accel_error", "road_bound_error",
              "collision_error", "ok", "stop_distance_error", "dropped")         # index = FOT_ST_*
SPEED, ACCEL, CURV, LAT, ROAD, COLLISION, OK, STOP, DROPPED = range(9)
BAND = 1e-9
BAND_CAP = 0.005                  # share of cases that may fall inside the band
FUZZ_SEEDS = range(300)

GATE, SLIP_RATIO, SLIP_FLOOR, DYAW_CAP, STOP_SPEED_EPS = 0.5, 1.5, 0.02, 0.1, 0.15

BASE_CFG = dict(max_speed=10.0, max_accel=2.0, max_curvature=1.0, max_lat_accel=3.0, dt=0.125, max_road_width=7.0,
                robot_radius=1.0, obstacle_radius=0.25, chance_epsilon=0.0, collision_margin_inflation=1.0,
                footprint=None)                                                   # footprint: (offsets, radius) or None


def cfg(**kw):
    out = dict(BASE_CFG)
    out.update(kw)
    return out


def multi_circle(length, width, n):
    """EgoFootprint.multi_circle (footprint.py:26-40) as (offsets, radius)."""
    seg = length / n
    return [float(o) for o in -length / 2 + seg / 2 + seg * np.arange(n)], float(math.hypot(seg / 2, width / 2))


def path(**fields):
    return {f: [float(v) for v in fields.get(f, [])] for f in FIELDS}


def call(cfg_, paths, static=None, dyn=None, dist=None, overrides=None, max_stop=None, name=""):
    return dict(cfg=cfg_, paths=list(paths), static=None if static is None else np.asarray(static, float).reshape(-1, 2),
                dyn=None if dyn is None else np.asarray(dyn, float), dist=None if dist is None else np.asarray(dist, float),
                overrides=overrides, max_stop=max_stop, name=name)


class _Margin:
    def __init__(self):
        self.m = math.inf

    def cmp(self, value, thr):
        value = np.asarray(value, float).ravel()
        with np.errstate(invalid="ignore", over="ignore"):
            rel = np.abs(value - thr) / abs(thr)
        rel = rel[np.isfinite(rel)]
        if rel.size:
            self.m = min(self.m, float(rel.min()))


# ------------------------------------------------------------------------------------------------ collision

def _geometry(c, p, inflation=1.0):
    if len(p["x"]) == 0:
        return None
    m = min(len(p["x"]), len(p["t"]))
    pts = np.stack([np.array(p["x"][:m]), np.array(p["y"][:m])], axis=1)
    pt = np.array(p["t"][:m])
    if c["footprint"] is None:
        ego_r = c["robot_radius"]
    else:
        off, ego_r = np.asarray(c["footprint"][0], float), c["footprint"][1]
        yaw = np.array(p["yaw"][:m])
        if len(yaw) < m:
            yaw = np.concatenate([yaw, np.full(m - len(yaw), yaw[-1] if len(yaw) > 0 else 0.0)])
        heading = np.stack([np.cos(yaw), np.sin(yaw)], axis=1)
        pts = (pts[None, :, :] + off[:, None, None] * heading[None, :, :]).reshape(len(off) * m, 2)
        pt = np.tile(pt, len(off))
    r = max(ego_r + c["obstacle_radius"], 1e-6)
    r_dyn = r * inflation
    grow = max(r, r_dyn)
    return pts, pt, np.min(pts, axis=0) - grow, np.max(pts, axis=0) + grow, r ** 2, r_dyn ** 2


def _hits_static(pts, lo, hi, static, sq, mg):
    if static is None or len(static) == 0:
        return False
    mask = (static[:, 0] >= lo[0]) & (static[:, 0] <= hi[0]) & (static[:, 1] >= lo[1]) & (static[:, 1] <= hi[1])
    if not np.any(mask):
        return False
    diff = pts[:, None, :] - static[mask][None, :, :]
    sq_d = np.sum(diff ** 2, axis=2)
    mg.cmp(sq_d, sq)
    return bool(np.any(sq_d <= sq))


def _hits_dynamic(dt, pts, pt, lo, hi, dyn, sq, mg):
    if dyn is None or dyn.size == 0 or dyn.shape[-1] != 2:
        return False
    o_lo, o_hi = np.min(dyn, axis=1), np.max(dyn, axis=1)
    mask = (o_hi[:, 0] >= lo[0]) & (o_lo[:, 0] <= hi[0]) & (o_hi[:, 1] >= lo[1]) & (o_lo[:, 1] <= hi[1])
    if not np.any(mask):
        return False
    cand = dyn[mask]
    rows = np.clip(np.round(pt / dt).astype(int), 0, cand.shape[1] - 1)
    diff = pts[:, None, :] - cand.transpose(1, 0, 2)[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        sq_d = np.sum(diff ** 2, axis=2)
    mg.cmp(sq_d, sq)
    return bool(np.any(sq_d <= sq))


def _free_single(c, p, static, dyn, mg):
    g = _geometry(c, p, c["collision_margin_inflation"])
    if g is None:
        return True
    pts, pt, lo, hi, sq, sq_dyn = g
    if _hits_static(pts, lo, hi, static, sq, mg):
        return False
    return not _hits_dynamic(c["dt"], pts, pt, lo, hi, dyn, sq_dyn, mg)


def _free_distribution(c, p, static, dist, eps, mg):
    g = _geometry(c, p)
    if g is None:
        return True
    pts, pt, lo, hi, sq, _ = g
    if _hits_static(pts, lo, hi, static, sq, mg):
        return False
    if dist is None or dist.size == 0:
        return True
    S = dist.shape[0]
    max_viol = int(np.floor(eps * S))
    viol = sum(_hits_dynamic(c["dt"], pts, pt, lo, hi, dist[k], sq, mg) for k in range(S))
    return viol <= max_viol


def _route(c, p, static, dyn, dist, mg):
    if dist is not None and dist.size > 0:                                       # :1043
        return _free_distribution(c, p, static, dist, c["chance_epsilon"], mg)
    return _free_single(c, p, static, dyn, mg)


def collision_free(c, p, static=None, dyn=None, dist=None):
    """_path_is_collision_free: (free, margin)."""
    mg = _Margin()
    return _route(c, p, static, dyn, dist, mg), mg.m


def collision_free_single(c, p, static=None, dyn=None):
    mg = _Margin()
    return _free_single(c, p, static, dyn, mg), mg.m


def collision_free_distribution(c, p, static=None, dist=None, eps=None):
    mg = _Margin()
    return _free_distribution(c, p, static, dist, c["chance_epsilon"] if eps is None else eps, mg), mg.m


# ------------------------------------------------------------------------------------------------ categories

def _curvature_feasible(c, p, lim_curv, mg):
    v, cc, x, y, yaw, s, d = (p[f] for f in ("v", "c", "x", "y", "yaw", "s", "d"))
    n = min(len(cc), len(v))
    n_geo = min(len(x), len(y), len(yaw), len(s), len(d))
    ok = True
    for i in range(1, n):
        mg.cmp(v[i], GATE)
        if v[i] > GATE:
            mg.cmp(abs(cc[i]), lim_curv)
            if abs(cc[i]) > lim_curv:
                ok = False
        elif i < n_geo:
            dd = abs(d[i] - d[i - 1])
            d_s = abs(s[i] - s[i - 1])
            thr = max(SLIP_RATIO * d_s, SLIP_FLOOR)
            mg.cmp(dd, thr)
            if dd > thr:
                ok = False
            dyaw = abs(np.arctan2(np.sin(yaw[i] - yaw[i - 1]), np.cos(yaw[i] - yaw[i - 1])))
            ds = float(np.hypot(x[i] - x[i - 1], y[i] - y[i - 1]))
            thr = max(lim_curv * ds, DYAW_CAP)
            mg.cmp(dyaw, thr)
            if dyaw > thr:
                ok = False
    return ok


def categorise(c, p, static=None, dyn=None, dist=None, overrides=None, max_stop=None):
    """_check_paths, then _apply_stop_distance_filter when max_stop is given: (FOT_ST_* index, margin)."""
    mg = _Margin()
    if len(p["x"]) == 0 or len(p["x"]) != len(p["t"]):
        return DROPPED, mg.m
    v, a, cc = np.asarray(p["v"], float), np.asarray(p["a"], float), np.asarray(p["c"], float)
    if not (np.all(np.isfinite(v)) and np.all(np.isfinite(a)) and np.all(np.isfinite(cc))):
        return DROPPED, mg.m
    o = overrides or {}
    lim_speed, lim_accel = o.get("max_speed", c["max_speed"]), o.get("max_accel", c["max_accel"])
    lim_curv, lim_lat = o.get("max_curvature", c["max_curvature"]), o.get("max_lat_accel", c["max_lat_accel"])
    if len(p["x"]) >= 2:
        with np.errstate(invalid="ignore", over="ignore"):
            step = np.hypot(np.diff(p["x"]), np.diff(p["y"]))
            limit = max(lim_speed, c["max_speed"]) * c["dt"] * 3.0
            mg.cmp(step, limit)
            if np.max(step) > limit:
                return DROPPED, mg.m
    mg.cmp(v[1:], lim_speed)
    if np.any(v[1:] > lim_speed):
        return SPEED, mg.m
    mg.cmp(np.abs(a[1:]), lim_accel)
    if np.any(np.abs(a[1:]) > lim_accel):
        return ACCEL, mg.m
    if not _curvature_feasible(c, p, lim_curv, mg):
        return CURV, mg.m
    n = min(len(v), len(cc))
    lat = v[1:n] * v[1:n] * np.abs(cc[1:n])
    mg.cmp(lat, lim_lat)
    if np.any(lat > lim_lat):
        return LAT, mg.m
    road = c["max_road_width"] + 1e-9
    d = np.abs(np.asarray(p["d"], float)[1:])
    mg.cmp(d, road)
    if np.any(d > road):
        return ROAD, mg.m
    if not _route(c, p, static, dyn, dist, mg):
        return COLLISION, mg.m
    if max_stop is not None:
        mg.cmp(abs(p["v"][-1]) if len(p["v"]) else math.inf, STOP_SPEED_EPS)
        stops = len(p["v"]) > 0 and abs(p["v"][-1]) <= STOP_SPEED_EPS
        travel = float(p["s"][-1] - p["s"][0]) if len(p["s"]) > 0 else 0.0
        mg.cmp(travel, max_stop + 1e-6)
        if not (stops and travel <= max_stop + 1e-6):
            return STOP, mg.m
    return OK, mg.m


def evaluate(cl):
    """Every path of a call: (categories [n], free [n], margins [n]) -- free is _path_is_collision_free alone."""
    cats, free, marg = [], [], []
    for p in cl["paths"]:
        k, m1 = categorise(cl["cfg"], p, cl["static"], cl["dyn"], cl["dist"], cl["overrides"], cl["max_stop"])
        f, m2 = collision_free(cl["cfg"], p, cl["static"], cl["dyn"], cl["dist"])
        cats.append(k); free.append(f); marg.append(min(m1, m2))
    return np.array(cats, int), np.array(free, bool), np.array(marg, float)


# ------------------------------------------------------------------------------------------------ fixture I/O

def save_calls(fname, calls, expected):
    """calls + the reference's answers -> one .npz (inputs and expected outputs only)."""
    out, meta = {}, []
    for i, (cl, ex) in enumerate(zip(calls, expected)):
        lens = [[len(p[f]) for f in FIELDS] for p in cl["paths"]]
        flat = [v for p in cl["paths"] for f in FIELDS for v in p[f]]
        out[f"k{i}_paths"] = np.array(flat, float)
        for key in ("static", "dyn", "dist"):
            if cl[key] is not None:
                out[f"k{i}_{key}"] = cl[key]
        out[f"k{i}_cat"] = np.array(ex["cat"], np.int8)
        out[f"k{i}_free"] = np.array(ex["free"], np.int8)
        meta.append(dict(name=cl["name"], cfg=cl["cfg"], lens=lens, overrides=cl["overrides"], max_stop=cl["max_stop"]))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(fname, **out)


def load_calls(fname):
    z = np.load(fname, allow_pickle=False)
    calls, expected = [], []
    for i, m in enumerate(json.loads(str(z["meta"]))):
        flat, pos, paths = z[f"k{i}_paths"], 0, []
        for lens in m["lens"]:
            p = {}
            for f, n in zip(FIELDS, lens):
                p[f] = flat[pos:pos + n].tolist()
                pos += n
            paths.append(p)
        c = m["cfg"]
        if c["footprint"] is not None:
            c["footprint"] = (list(c["footprint"][0]), float(c["footprint"][1]))
        arr = {key: (z[f"k{i}_{key}"] if f"k{i}_{key}" in z.files else None) for key in ("static", "dyn", "dist")}
        calls.append(dict(cfg=c, paths=paths, overrides=m["overrides"], max_stop=m["max_stop"], name=m["name"], **arr))
        expected.append(dict(cat=z[f"k{i}_cat"].astype(int), free=z[f"k{i}_free"].astype(bool)))
    return calls, expected


# ------------------------------------------------------------------------------------------------ hand-made classes

DT = 0.125                                   # a power of two: t / dt is exact


def straight(n, step=0.5, v=4.0, y0=0.0, t0=0.0, dt=DT, x0=0.0, **over):
    """A feasible straight path along x: n samples `step` apart."""
    k = np.arange(n)
    f = dict(t=t0 + k * dt, x=x0 + k * step, y=np.full(n, y0), yaw=np.zeros(n), v=np.full(n, v) if np.ndim(v) == 0 else v, a=np.zeros(n),
             c=np.zeros(n), d=np.zeros(n), s=k * step)
    f.update(over)
    return path(**f)


def next_up(v):
    return float(np.nextafter(v, math.inf))


def eps_pairs():
    """(eps, S) whose float64 product rounds just below and just above an integer, and the plain ones."""
    below = above = None
    for S in (20, 63, 64, 7, 50):
        for num in range(1, S):
            for e in (num / S, float(np.nextafter(num / S, 0.0)), next_up(num / S), round(num / S, 2), round(num / S, 3)):
                prod, near = e * S, round(e * S)
                if prod == near or abs(prod - near) > 1e-12 or not 0.0 < e < 1.0:
                    continue
                if prod < near and below is None:
                    below = (e, S)
                if prod > near and above is None:
                    above = (e, S)
    assert below and above
    return [below, above, (0.0, 4), (1.0, 4), (0.1, 20), (0.5, 64), (0.3, 10)]


def class_calls():
    """The classes of tests/test_gpu_check_paths_fuzz.py that have a reference answer, as calls (name, ...)."""
    out = []
    base = cfg()                              # combined radius 1.25: 1.5625 = 0.75^2 + 1.0^2 exactly
    # ---- time index: one pedestrian far away except in one row, where it stands on the path's sample
    far = [500.0, 500.0]

    def ped_rows(T, at):                      # [1, T, 2]: row -> (x, y)
        d = np.tile(np.array(far), (1, T, 1))
        for r, xy in at.items():
            d[0, r] = xy
        return d
    for name, tq, want_row in (("half0", [0.5], 0), ("half1", [1.5], 2), ("half2", [2.5], 2), ("neg", [-3.0], 0),
                               ("offset", [5.0], 5), ("plain", [3.0], 3)):
        for row in range(7):                  # the pedestrian is on the path at `row` only: hit iff row == want_row
            p = straight(1, t=[q * DT for q in tq])
            out.append(call(base, [p], dyn=ped_rows(7, {row: [0.0, 0.0]}), name=f"tindex_{name}_row{row}"))
    p = straight(6, t=np.array([0.0, 0.75, 2.0, 2.25, 5.0, 9.0]) * DT)          # non-uniform: rows 0 1 2 2 5 9
    for row in range(10):
        out.append(call(base, [p], dyn=ped_rows(10, {row: [p["x"][min(row, 5)], 0.0]}), name=f"tindex_nonuniform_row{row}"))
    p = straight(8)
    out.append(call(base, [p], dyn=ped_rows(1, {0: [3.5, 0.0]}), name="tindex_T1"))
    for k in range(8):                        # T = 4 < 8 samples: row 3 serves samples 3..7
        out.append(call(base, [p], dyn=ped_rows(4, {3: [p["x"][k], 0.0]}), name=f"tindex_Tshort_{k}"))
        out.append(call(base, [p], dyn=ped_rows(4, {2: [p["x"][k], 0.0]}), name=f"tindex_Tshort_row2_{k}"))
    out.append(call(base, [p], dyn=ped_rows(12, {r: [3.5, 0.0] for r in range(8, 12)}), name="tindex_Tlong"))
    # ---- radius: an obstacle exactly on the combined radius, and one ulp outside
    p1 = straight(1)
    on, off = [0.75, 1.0], [0.75, next_up(1.0)]
    for nm, xy in (("on", on), ("off", off)):
        out.append(call(base, [p1], static=[xy], name=f"radius_static_{nm}"))
        out.append(call(base, [p1], dyn=np.array([[xy]]), name=f"radius_dyn_{nm}"))
        out.append(call(base, [p1], dist=np.array([[[xy]]]), name=f"radius_dist_{nm}"))
    infl = cfg(collision_margin_inflation=1.2)                                   # 1.25 * 1.2 = 1.5
    for nm, xy in (("in", [0.0, 1.4]), ("out", [0.0, 1.6]), ("nominal", [0.0, 1.2])):
        out.append(call(infl, [p1], dyn=np.array([[xy]]), name=f"inflation_single_{nm}"))
        out.append(call(infl, [p1], dist=np.array([[[xy]]]), name=f"inflation_dist_{nm}"))
        out.append(call(infl, [p1], static=[xy], name=f"inflation_static_{nm}"))
    # ---- chance budget
    p = straight(6)
    for S in (1, 2, 20, 63, 64):              # only sample S-1 hits, at several steps
        d = np.tile(np.array(far), (S, 2, 6, 1))
        d[S - 1, :, :, :] = np.stack([np.array(p["x"]), np.zeros(6)], axis=1)
        out.append(call(base, [p], dist=d, name=f"budget_last_S{S}"))
        out.append(call(cfg(chance_epsilon=1.0 / S), [p], dist=d, name=f"budget_last_forgiven_S{S}"))
    for e, S in eps_pairs():
        k = int(math.floor(e * S))
        for extra in (0, 1):
            if k + extra > S:
                continue
            d = np.tile(np.array(far), (S, 1, 6, 1))
            d[S - (k + extra):, 0, :, :] = np.stack([np.array(p["x"]), np.zeros(6)], axis=1)
            out.append(call(cfg(chance_epsilon=e), [p], dist=d, name=f"budget_eps{e!r}_S{S}_{k}+{extra}"))
    d = np.tile(np.array(far), (4, 1, 6, 1))
    out.append(call(cfg(chance_epsilon=1.0), [p], static=[[1.0, 0.5]], dist=d, name="budget_static_never_forgiven"))
    # ---- footprint
    for n in (1, 3, 8):
        fp = cfg(footprint=multi_circle(4.5, 2.0, n))
        r = fp["footprint"][1] + 0.25
        front, rear = fp["footprint"][0][-1], fp["footprint"][0][0]
        for yaw_name, yaw in (("east", 0.0), ("north", math.pi / 2), ("west", math.pi), ("skew", 0.7)):
            pf = straight(1, yaw=[yaw])
            tip = [(front + 0.9 * r) * math.cos(yaw), (front + 0.9 * r) * math.sin(yaw)]
            tail = [(rear - 0.9 * r) * math.cos(yaw), (rear - 0.9 * r) * math.sin(yaw)]
            side = [-(abs(front) + 1.1 * r) * math.sin(yaw), (abs(front) + 1.1 * r) * math.cos(yaw)]
            for nm, xy in (("tip", tip), ("tail", tail), ("side", side)):
                out.append(call(fp, [pf], static=[xy], name=f"footprint{n}_{yaw_name}_{nm}_static"))
                out.append(call(fp, [pf], dyn=np.array([[xy]]), name=f"footprint{n}_{yaw_name}_{nm}_dyn"))
    fp3 = cfg(footprint=multi_circle(4.5, 2.0, 3))
    held = straight(4, yaw=[math.pi / 2, math.pi / 2])                           # yaw shorter: held
    out.append(call(fp3, [held], static=[[1.5, 2.5]], name="footprint_yaw_held"))
    out.append(call(fp3, [straight(4, yaw=[0.0, 0.0])], static=[[1.5, 2.5]], name="footprint_yaw_held_east"))
    # ---- non-finite obstacles
    p = straight(4)
    for bad_name, bad in (("nan", math.nan), ("pinf", math.inf), ("ninf", -math.inf)):
        trk = np.zeros((1, 9, 2)); trk[0, :, 0] = 1.0                            # stands on the path at every row
        for ax in (0, 1):
            t2 = trk.copy(); t2[0, 8, ax] = bad                                  # a row the path never indexes
            out.append(call(base, [p], dyn=t2, name=f"nonfinite_track_{bad_name}_ax{ax}_unindexed"))
            t3 = trk.copy(); t3[0, :4, ax] = bad                                 # every row it does index
            out.append(call(base, [p], dyn=t3, name=f"nonfinite_track_{bad_name}_ax{ax}_indexed"))
            dd = np.tile(np.array(far), (3, 2, 9, 1))
            dd[1, 1] = trk[0]; dd[1, 1, 8, ax] = bad                             # (sample 1, pedestrian 1) alone is bad
            out.append(call(base, [p], dist=dd, name=f"nonfinite_dist_{bad_name}_ax{ax}"))
            dd2 = dd.copy(); dd2[2, 0] = trk[0]                                  # ... and a clean one hits
            out.append(call(base, [p], dist=dd2, name=f"nonfinite_dist_{bad_name}_ax{ax}_other_hits"))
            out.append(call(base, [p], static=[[1.0, 0.0] if ax else [bad, 0.0], [bad, 0.0] if ax else [500.0, 0.0]],
                            name=f"nonfinite_static_{bad_name}_ax{ax}"))
            out.append(call(base, [p], static=[[bad, 0.0] if ax == 0 else [1.0, bad]], name=f"nonfinite_static_only_{bad_name}_ax{ax}"))
    # ---- categories
    n = 6
    lowv = [4.0, 0.3, 0.3, 0.3, 0.3, 0.3]

    def low(**over):                          # a crawling path: 0.03 m per sample
        f = dict(step=0.03, v=0.3)
        return straight(n, **{**f, **over})
    rules = {                                 # (array, index, value) that make exactly this rule fail
        "dropped_nonfinite": [("a", 2, math.nan)],
        "dropped_step": [("x", 3, 9.0), ("x", 4, 9.5), ("x", 5, 10.0)],
        "speed": [("v", 2, 11.0)],
        "accel": [("a", 3, -2.5)],
        "curv": [("c", 4, 1.5)],
        "lat": [("c", 1, 0.5)],                                                  # 16 * 0.5 = 8 > 3
        "road": [("d", 5, -7.5)],
        "collision": [],
    }
    names = list(rules)
    for i, ra in enumerate(names):
        for rb in names[i:]:
            q = straight(n)
            for f, j, val in rules[ra] + rules[rb]:
                q[f][j] = val
            st = [[1.0, 0.5]] if "collision" in (ra, rb) else None
            out.append(call(base, [q], static=st, name=f"pair_{ra}+{rb}"))
    for f, bad in (("v", 99.0), ("a", 99.0), ("c", 99.0), ("d", 99.0)):          # index 0 is exempt
        vals = list(straight(n)[f]); vals[0] = bad
        out.append(call(base, [straight(n, **{f: vals})], name=f"index0_{f}"))
    # the gate: v exactly 0.5 takes the low-speed rules (a large c is fine), the next float takes the pointwise one
    for nm, vg in (("at", 0.5), ("above", next_up(0.5))):
        out.append(call(base, [low(v=[4.0, vg, vg, vg, vg, vg], c=[0, 2.0, 2.0, 2.0, 2.0, 2.0])], name=f"gate_{nm}_bigc"))
        out.append(call(base, [low(v=[4.0, vg, vg, vg, vg, vg], d=[0, 0, 0.5, 0.5, 0.5, 0.5])], name=f"gate_{nm}_slip"))
    s = [0.0, 0.03, 0.06, 0.09, 0.12, 0.15]
    for nm, dd in (("floor_at", 0.02), ("floor_over", next_up(0.02)), ("floor_big", 0.021)):
        same_s = [0.0] * n                                                       # no progress: the floor decides
        out.append(call(base, [low(v=lowv, s=same_s, d=[0, 0, dd, dd, dd, dd])], name=f"slip_{nm}"))
    wide = [0.0, 0.25, 0.5, 0.75, 1.0, 1.25]                                     # 1.5 * 0.25 = 0.375 exactly
    for nm, dd in (("ratio_at", 0.375), ("ratio_over", next_up(0.375))):
        out.append(call(base, [low(v=lowv, s=wide, x=wide, d=[0, 0, dd, dd, dd, dd])], name=f"slip_{nm}"))
    for nm, y2 in (("pi_small", [3.1, 3.1, -3.1, -3.1, -3.1, -3.1]), ("pi_big", [3.0, 3.0, -3.0, -3.0, -3.0, -3.0]),
                   ("cap_under", [0, 0, 0.099, 0.099, 0.099, 0.099]), ("cap_over", [0, 0, 0.101, 0.101, 0.101, 0.101]),
                   ("neg_over", [0, 0, -0.101, -0.101, -0.101, -0.101])):
        out.append(call(base, [low(v=lowv, yaw=y2)], name=f"yaw_{nm}"))
    for nm, y2 in (("curv_ds_under", 0.24), ("curv_ds_over", 0.26)):             # ds 0.25, max_curvature 1: cap 0.25
        out.append(call(base, [low(v=lowv, s=wide, x=wide, yaw=[0, 0, y2, y2, y2, y2])], name=f"yaw_{nm}"))
        out.append(call(base, [low(v=lowv, s=wide, x=wide, yaw=[0, 0, y2, y2, y2, y2])], overrides=dict(max_curvature=0.5),
                        name=f"yaw_{nm}_override"))
    for key, over in (("max_speed", dict(v=[4, 4, 6.0, 4, 4, 4])), ("max_accel", dict(a=[0, 0, 1.5, 0, 0, 0])),
                      ("max_curvature", dict(c=[0, 0, 0.15, 0, 0, 0])), ("max_lat_accel", dict(c=[0, 0, 0.15, 0, 0, 0]))):
        tight = {"max_speed": 5.0, "max_accel": 1.0, "max_curvature": 0.1, "max_lat_accel": 2.0}[key]
        out.append(call(base, [straight(n, **over)], name=f"override_{key}_none"))
        out.append(call(base, [straight(n, **over)], overrides={key: tight}, name=f"override_{key}_tight"))
    jump = dict(x=[0, 0.5, 1.0, 5.0, 5.5, 6.0])                                  # a 4 m step; 10 * 0.125 * 3 = 3.75
    out.append(call(base, [straight(n, **jump)], name="step_planner_limit"))
    out.append(call(base, [straight(n, **jump)], overrides=dict(max_speed=12.0), name="step_override_above"))   # 4.5
    out.append(call(base, [straight(n, **jump)], overrides=dict(max_speed=2.0), name="step_override_below"))
    out.append(call(base, [straight(n, x=[0, 0.5, 1.0, 4.75, 5.25, 5.75])], name="step_exactly_at_limit"))
    out.append(call(base, [straight(n, step=1.0, v=1.5)], overrides=dict(max_speed=2.0),     # 1 m steps: over 2 * dt * 3,
                    name="step_between_the_override_and_the_planner_limit"))                 # under the planner's 3.75
    out.append(call(base, [straight(n, x=[0, 0.5, math.nan, 1.5, 30.0, 30.5])], name="step_nan_not_dropped"))
    out.append(call(base, [straight(n, x=[0, 0.5, math.nan, 1.5, 2.0, 2.5])], static=[[2.0, 0.0]],
                    name="step_nan_path_never_collides"))
    for f in ("v", "a", "c"):
        for bad_name, bad in (("nan", math.nan), ("inf", math.inf), ("ninf", -math.inf)):
            vals = list(straight(n)[f]); vals[0] = bad                           # index 0 is NOT exempt from this one
            out.append(call(base, [straight(n, **{f: vals})], name=f"nonfinite_{f}_{bad_name}"))
    for nm, dv in (("at", 7.0 + 1e-9), ("over", next_up(7.0 + 1e-9)), ("neg_over", -next_up(7.0 + 1e-9))):
        out.append(call(base, [straight(n, d=[0, 0, dv, 0, 0, 0])], name=f"road_{nm}"))
    stop = straight(n, v=[4, 3, 2, 1, 0.5, 0.15], s=[0, 0.5, 1.0, 1.5, 1.75, 2.0])
    for nm, ms in (("none", None), ("met", 2.0), ("met_with_slack", 2.0 - 1e-6), ("short", 1.9), ("long", 5.0)):
        out.append(call(base, [stop], max_stop=ms, name=f"stop_{nm}"))
    out.append(call(base, [straight(n, v=[4, 3, 2, 1, 0.5, next_up(0.15)], s=stop["s"])], max_stop=5.0, name="stop_still_moving"))
    out.append(call(base, [straight(n, v=[4, 3, 2, 1, 0.5, -0.1], s=stop["s"])], max_stop=5.0, name="stop_negative_v"))
    out.append(call(base, [straight(n, t=[0.0] * 5), path(), straight(n)], name="len_mismatch_and_empty"))
    # ---- ragged arrays: every array shorter and longer than x, the offending sample inside and outside the short one
    m = 12
    bad_at = {"v": 11.0, "a": 3.0, "c": 1.5, "d": 8.0}
    for f in ("v", "a", "c", "d"):
        for ln in (4, 8, m, 16):
            for at in (2, 6, 14):
                if at >= ln:
                    continue
                full = list(straight(16)[f]); full[at] = bad_at[f]
                out.append(call(base, [straight(m, **{f: full[:ln]})], name=f"ragged_{f}_len{ln}_bad{at}"))
    crawl = dict(step=0.03, v=[4.0] + [0.3] * (m - 1))
    for f in ("s", "d", "yaw"):
        for ln in (4, 8, 16):
            for at in (2, 6):
                slip = [0.0] * 16
                for j in range(at, 16):
                    slip[j] = 0.5
                over = {"d": slip, "s": list(np.arange(16) * 0.03), "yaw": [0.0] * 16}
                if f == "yaw":
                    over["d"] = [0.0] * 16; over["yaw"] = slip                   # a 0.5 rad pivot instead of a slip
                over = {k: (vv[:ln] if k == f else vv[:m]) for k, vv in over.items()}
                out.append(call(base, [straight(m, **{**crawl, **over})], name=f"ragged_geo_{f}_len{ln}_bad{at}"))
    short_v = straight(m, **crawl)
    short_v["v"] = short_v["v"][:5]                                              # the low-speed rules stop with v
    short_v["d"] = [0.0] * 8 + [0.5] * 4
    out.append(call(base, [short_v], name="ragged_short_v_no_lowspeed_behind_it"))
    for f, ln in (("v", 0), ("s", 0), ("v", 3), ("s", 3), ("v", 16), ("s", 16)):
        full = straight(16, v=[4, 3, 2, 1, 0.5, 0.1] + [0.1] * 10, s=list(np.linspace(0, 3.0, 16)))
        q = straight(m, v=full["v"][:m], s=full["s"][:m])
        q[f] = full[f][:ln]
        if f == "v" and ln == 3:
            q["v"] = [4.0, 3.0, 0.1]
        out.append(call(base, [q], max_stop=2.5, name=f"ragged_stop_{f}_len{ln}"))
    lat = straight(m, c=[0.0] * 3)
    lat["v"] = [4.0] * 16
    out.append(call(base, [lat], name="ragged_long_v"))
    nf = straight(m)
    nf["a"] = [0.0] * 14 + [math.nan]
    out.append(call(base, [nf], name="ragged_nonfinite_behind_x"))
    return out


# ------------------------------------------------------------------------------------------------ fuzz

def fuzz_configs():
    """The planner configurations the fuzz draws from (a test keeps one library handle per entry)."""
    rng = np.random.default_rng(20261017)
    out = []
    for i in range(12):
        n_circ = (0, 1, 3, 8)[i % 4]
        out.append(cfg(max_speed=float(rng.uniform(4, 12)), max_accel=float(rng.uniform(1, 3)),
                       max_curvature=float(rng.uniform(0.2, 1.0)), max_lat_accel=float(rng.uniform(2, 4)),
                       dt=(0.1, 0.125, 0.2)[i % 3], max_road_width=float(rng.uniform(3, 7)),
                       robot_radius=float(rng.uniform(0.5, 1.5)), obstacle_radius=float(rng.uniform(0.1, 0.5)),
                       chance_epsilon=(0.0, 0.1, 0.25, 0.5)[(i // 3) % 4], collision_margin_inflation=(1.0, 1.2)[i % 2],
                       footprint=multi_circle(float(rng.uniform(3.5, 5.0)), float(rng.uniform(1.6, 2.2)), n_circ)
                       if n_circ else None))
    return out


def fuzz_path(rng, c, lim, kind, n=None):
    """One random-walk path that fails `kind` (or nothing); n samples (2 to 64 when not given)."""
    n = int(rng.integers(2, 65)) if n is None else n
    if n == 0:
        return path()
    dt = c["dt"]
    slow = rng.random() < 0.3
    v0 = rng.uniform(0.0, 0.6) if slow else rng.uniform(0.6, 0.8 * lim["max_speed"])
    a = rng.normal(0, 0.25 * lim["max_accel"], n)
    a = np.clip(a, -0.8 * lim["max_accel"], 0.8 * lim["max_accel"])
    v = np.clip(v0 + np.cumsum(a) * dt, 0.0, 0.8 * min(lim["max_speed"], c["max_speed"]))
    cmax = np.minimum(0.8 * lim["max_curvature"], 0.8 * lim["max_lat_accel"] / np.maximum(v * v, 1e-3))
    curv = np.clip(np.cumsum(rng.normal(0, 0.02, n)), -cmax, cmax)
    ds = v * dt
    yaw = rng.uniform(-math.pi, math.pi) + np.cumsum(curv * ds)
    x = rng.normal(0, 30) + np.cumsum(ds * np.cos(yaw))
    y = rng.normal(0, 30) + np.cumsum(ds * np.sin(yaw))
    s = rng.uniform(0, 50) + np.cumsum(ds)
    d = np.clip(rng.normal(0, 1) + np.cumsum(rng.normal(0, 0.2, n) * ds), -0.8 * c["max_road_width"], 0.8 * c["max_road_width"])
    t = (np.arange(n) + int(rng.choice([0, 0, 3]))) * dt
    if rng.random() < 0.25:
        t = t + rng.uniform(-0.3, 0.3, n) * dt
    j = int(rng.integers(0 if rng.random() < 0.2 else 1, n)) if n > 1 else 0
    if kind == "speed":
        v[j] = lim["max_speed"] * rng.uniform(1.05, 1.5)
    elif kind == "accel":
        a[j] = lim["max_accel"] * rng.uniform(1.05, 1.5) * rng.choice([-1, 1])
    elif kind == "curv":
        if v[j] > GATE:
            curv[j] = lim["max_curvature"] * rng.uniform(1.05, 1.5) * rng.choice([-1, 1])
            v[j] = min(v[j], math.sqrt(0.5 * lim["max_lat_accel"] / abs(curv[j])))
            if v[j] <= GATE:
                d[j:] += 0.5
        elif rng.random() < 0.5:
            d[j:] += rng.uniform(0.1, 0.5)
        else:
            yaw[j:] += rng.uniform(0.3, 3.0)
    elif kind == "lat":
        v[j] = max(v[j], 0.7 * min(lim["max_speed"], c["max_speed"]))
        curv[j] = min(0.9 * lim["max_curvature"], 1.3 * lim["max_lat_accel"] / (v[j] * v[j])) * rng.choice([-1, 1])
    elif kind == "road":
        d[j] = c["max_road_width"] * rng.uniform(1.05, 1.5) * rng.choice([-1, 1])
    elif kind == "dropped":
        r = rng.random()
        if r < 0.4:
            x[j:] += 5.0 * max(lim["max_speed"], c["max_speed"]) * dt
        elif r < 0.8:
            (v, a, curv)[int(rng.integers(3))][j] = (math.nan, math.inf, -math.inf)[int(rng.integers(3))]
        else:
            t = t[:-1]
    elif kind == "stop":
        v[-1] = rng.uniform(0.0, 0.3)
    return path(t=t, x=x, y=y, yaw=yaw, v=v, a=a, c=curv, d=d, s=s)


def fuzz_call(seed):
    """One seeded call: 1 to 8 random-walk paths of 2 to 64 samples against one obstacle set."""
    rng = np.random.default_rng([int(seed), 0xC4EC])
    cfgs = fuzz_configs()
    c = cfgs[int(rng.integers(len(cfgs)))]
    overrides = None
    if rng.random() < 0.4:
        overrides = {k: float(c[k] * rng.uniform(0.6, 1.3)) for k in ("max_speed", "max_accel", "max_curvature", "max_lat_accel")
                     if rng.random() < 0.5} or None
    lim = {k: (overrides or {}).get(k, c[k]) for k in ("max_speed", "max_accel", "max_curvature", "max_lat_accel")}
    kinds = ("ok", "collision", "speed", "accel", "curv", "lat", "road", "dropped", "stop", "ok")
    paths = [fuzz_path(rng, c, lim, kinds[int(rng.integers(len(kinds)))]) for _ in range(int(rng.integers(1, 9)))]
    max_stop = float(rng.uniform(0.5, 6.0)) if rng.random() < 0.3 else None
    r = (c["footprint"][1] if c["footprint"] else c["robot_radius"]) + c["obstacle_radius"]

    def near(p, k):                                       # a point within reach of sample k of path p, or just beyond
        k = min(k, len(p["x"]) - 1)
        ang, dist = rng.uniform(0, 2 * math.pi), r * rng.uniform(0.0, 2.0)
        return [p["x"][k] + dist * math.cos(ang), p["y"][k] + dist * math.sin(ang)]
    static = None
    if rng.random() < 0.5:
        static = np.array([near(paths[int(rng.integers(len(paths)))], int(rng.integers(64))) if rng.random() < 0.3
                           else [rng.normal(0, 60), rng.normal(0, 60)] for _ in range(int(rng.integers(1, 6)))])
    mode = int(rng.integers(3))                           # none, single, distribution
    dyn = dist = None
    if mode:
        S, P = (int(rng.integers(1, 9)) if mode == 2 else 1), int(rng.integers(1, 9))
        T = int(rng.choice([1, 5, 30, 64, 70]))
        tracks = np.empty((S, P, T, 2))
        for si in range(S):
            for pi in range(P):
                p = paths[int(rng.integers(len(paths)))]
                if rng.random() < 0.35:                   # crosses the path near one sample, at that sample's time
                    k = int(rng.integers(len(p["x"])))
                    row = min(max(int(np.round(p["t"][min(k, len(p["t"]) - 1)] / c["dt"])), 0), T - 1)
                    vel = rng.normal(0, 1.0, 2) * c["dt"]
                    tracks[si, pi] = np.array(near(p, k)) + (np.arange(T)[:, None] - row) * vel
                else:
                    tracks[si, pi] = rng.normal(0, 60, 2) + np.cumsum(rng.normal(0, 0.2, (T, 2)), axis=0)
                if rng.random() < 0.03:
                    tracks[si, pi, int(rng.integers(T)), int(rng.integers(2))] = (math.nan, math.inf)[int(rng.integers(2))]
        if mode == 1:
            dyn = tracks[0]
        else:
            dist = tracks
    return call(c, paths, static=static, dyn=dyn, dist=dist, overrides=overrides, max_stop=max_stop, name=f"fuzz{seed}")
