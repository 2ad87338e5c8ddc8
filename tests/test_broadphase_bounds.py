"""The float32 broad phase's bounds (csrc/fot_math.hpp), checked as properties on the host.

Every collision decision of plan() first passes k_cull (an obstacle is kept only inside the float32 box of a time
step grown by cull_margin), the strips of the entry lists (strip_range over 32 bins) and the two float32 thresholds of
k_evaluate's sink (above `thr`: a certain miss, at or below `thr_sure`: a certain hit).  The output is the reference's
only if every one of these is conservative.  tests/emu/fot_bounds.cpp loops the header's own functions; here they meet
float64 ground truth over fixed-seed random inputs and over adversarial pairs placed at R (1 +- k 2^-52) and
R (1 +- 10^-m) -- the sliver of the radius where a bound that is one rounding too tight flips a decision and random
placement (tests/test_gpu_fuzz.py) almost never lands.

Coordinates are instance-local (relative to the ego, as the kernels use them) up to L_MAX = 1000 km, far beyond the
largest box a lattice reaches in practice (FOT_MAX_NT samples x dt x speed: 256 x 0.1 s x 60 m/s is 1.5 km), with the
ego itself up to 2e4 m from the map origin.  The properties are checked up to 1000 km, far beyond any lattice
(<= ~1.5 km); every bound carries a term relative to the coordinates, and none of them is seen to stop holding there.  (Without cull_margin's
relative term P3 fails at tens of kilometres: the fixed 1 mm slack covers the rounding of smaller coordinates.)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SO = os.path.join(EMU_DIR, "_build", "libfot_bounds.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")

L_MAX = 1.0e6                    # largest instance-local coordinate the properties are checked at (m)
R_MIN, R_MAX = 0.1, 6.0          # collision radii (m)
EGOS = ((0.0, 0.0), (1.5e4, -1.2e4), (-2.0e4, 7.5e3))                     # map-frame ego positions
ADV_DELTAS = np.array(sorted({s * k * 2.0 ** -52 for s in (-1, 1) for k in range(1, 65)}
                             | {s * 10.0 ** -m for s in (-1, 1) for m in range(3, 10)}))

f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    srcs = [os.path.join(EMU_DIR, "fot_bounds.cpp")] + [os.path.join(CSRC, f) for f in ("fot_math.hpp", "fot_types.h")]
    srcs.append(os.path.join(ROOT, "include", "fot.h"))
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SO, srcs[0]],
                       check=True)
    L = C.CDLL(SO)
    n = C.c_int64
    L.bnd_cull_margin.argtypes = [n, f64p, f32p, f32p]
    L.bnd_cull_inside.argtypes = [n, f32p, f32p, f32p, f32p, i32p]
    L.bnd_filter_const.argtypes = [n, f64p, f64p, f32p]
    L.bnd_filter_threshold.argtypes = [n, f32p, f32p, f32p, f32p]
    L.bnd_filter_threshold_sure.argtypes = [n, f32p, f32p, f32p, f32p]
    L.bnd_box_thresholds.argtypes = [n, f32p, f32p, f32p, f32p, f32p]
    L.bnd_min_sqdist32_8.argtypes = [n, f32p, f32p, f32p, f32p]
    L.bnd_bin_map.argtypes = [n, f32p, f32p, i32p, f32p, f32p]
    L.bnd_bin_of.argtypes = [n, i32p, f32p, f32p, f32p, f32p, i32p]
    L.bnd_strip_range.argtypes = [n, i32p, f32p, f32p, f32p, f32p, i32p, u32p]
    L.bnd_segment_box.argtypes = [n] + [f64p] * 8 + [f32p]
    L.bnd_box_footprint_slack.argtypes = [C.c_int, f64p]
    L.bnd_box_footprint_slack.restype = C.c_float
    assert L.bnd_cull_bins() == 32 and L.bnd_ent_chunk() == 8
    return L


def _p(a, dtype):
    """ctypes pointer to a C-contiguous array of `dtype` (the array must outlive the call)."""
    assert a.dtype == dtype and a.flags.c_contiguous
    return a.ctypes.data_as({np.float32: f32p, np.float64: f64p, np.int32: i32p, np.uint32: u32p}[dtype])


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# ---- batch wrappers --------------------------------------------------------------------------------------------------

def filter_const(L, sq, sq_min):
    sq, sq_min = _f64(sq), _f64(sq_min)
    out = np.zeros((len(sq), 3), np.float32)
    L.bnd_filter_const(len(sq), _p(sq, np.float64), _p(sq_min, np.float64), _p(out, np.float32))
    return out


def box_thresholds(L, fc, boxes, m):
    fc, boxes, m = _f32(fc), _f32(boxes), _f32(m)
    thr = np.zeros(len(m), np.float32); sure = np.zeros(len(m), np.float32)
    L.bnd_box_thresholds(len(m), _p(fc, np.float32), _p(boxes, np.float32), _p(m, np.float32),
                         _p(thr, np.float32), _p(sure, np.float32))
    return thr, sure


def filter_thresholds(L, fc, px, py):
    fc, px, py = _f32(fc), _f32(px), _f32(py)
    thr = np.zeros(len(px), np.float32); sure = np.zeros(len(px), np.float32)
    L.bnd_filter_threshold(len(px), _p(fc, np.float32), _p(px, np.float32), _p(py, np.float32), _p(thr, np.float32))
    L.bnd_filter_threshold_sure(len(px), _p(fc, np.float32), _p(px, np.float32), _p(py, np.float32),
                                _p(sure, np.float32))
    return thr, sure


def sqdist32(L, fx, fy, cx, cy):
    """fmaf(dy, dy, dx * dx) of k_evaluate's sink, through min_sqdist32_8 (the obstacle in all 8 slots)."""
    fx, fy = _f32(fx), _f32(fy)
    chunks = _f32(np.concatenate([np.repeat(_f32(cx)[:, None], 8, 1), np.repeat(_f32(cy)[:, None], 8, 1)], 1))
    out = np.zeros(len(fx), np.float32)
    L.bnd_min_sqdist32_8(len(fx), _p(chunks, np.float32), _p(fx, np.float32), _p(fy, np.float32), _p(out, np.float32))
    return out


def cull_margin(L, max_sq, boxes):
    max_sq, boxes = _f64(max_sq), _f32(boxes)
    out = np.zeros(len(max_sq), np.float32)
    L.bnd_cull_margin(len(max_sq), _p(max_sq, np.float64), _p(boxes, np.float32), _p(out, np.float32))
    return out


def cull_inside(L, boxes, m, fx, fy):
    boxes, m, fx, fy = _f32(boxes), _f32(m), _f32(fx), _f32(fy)
    out = np.zeros(len(m), np.int32)
    L.bnd_cull_inside(len(m), _p(boxes, np.float32), _p(m, np.float32), _p(fx, np.float32), _p(fy, np.float32),
                      _p(out, np.int32))
    return out.astype(bool)


def segment_box(L, rx, ry, cs, sn, d0, d1, ox, oy):
    a = [_f64(v) for v in (rx, ry, cs, sn, d0, d1, ox, oy)]
    out = np.zeros((len(a[0]), 4), np.float32)
    L.bnd_segment_box(len(a[0]), *[_p(v, np.float64) for v in a], _p(out, np.float32))
    return out


def bin_map(L, boxes, margin):
    boxes, margin = _f32(boxes), _f32(margin)
    n = len(margin)
    axis = np.zeros(n, np.int32); lo = np.zeros(n, np.float32); inv_w = np.zeros(n, np.float32)
    L.bnd_bin_map(n, _p(boxes, np.float32), _p(margin, np.float32), _p(axis, np.int32), _p(lo, np.float32),
                  _p(inv_w, np.float32))
    return axis, lo, inv_w


def bin_of(L, axis, lo, inv_w, x, y):
    axis, lo, inv_w, x, y = np.ascontiguousarray(axis, np.int32), _f32(lo), _f32(inv_w), _f32(x), _f32(y)
    out = np.zeros(len(x), np.int32)
    L.bnd_bin_of(len(x), _p(axis, np.int32), _p(lo, np.float32), _p(inv_w, np.float32), _p(x, np.float32),
                 _p(y, np.float32), _p(out, np.int32))
    return out


def strip_range(L, axis, lo, inv_w, wboxes, margin, starts):
    axis, lo, inv_w = np.ascontiguousarray(axis, np.int32), _f32(lo), _f32(inv_w)
    wboxes, margin, starts = _f32(wboxes), _f32(margin), np.ascontiguousarray(starts, np.int32)
    out = np.zeros(len(margin), np.uint32)
    L.bnd_strip_range(len(margin), _p(axis, np.int32), _p(lo, np.float32), _p(inv_w, np.float32),
                      _p(wboxes, np.float32), _p(margin, np.float32), _p(starts, np.int32), _p(out, np.uint32))
    return out


def footprint_slack(L, offsets):
    o = _f64(list(offsets) + [0.0] * (8 - len(offsets)))
    return L.bnd_box_footprint_slack(len(offsets), _p(o, np.float64))


# ---- inputs ----------------------------------------------------------------------------------------------------------

def sum_sq_unfused(dx, dy):
    """fot_math.hpp within(): (dx*dx) + (dy*dy), two float64 roundings (numpy never contracts)."""
    return dx * dx + dy * dy


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def local_points(rng, n, l_max=L_MAX):
    """Instance-local points of both signs, log-uniform magnitudes 1 cm .. l_max on either axis (so that either axis is
    the longer one) plus a share exactly at the top of the range."""
    mag_x = log_uniform(rng, 1e-2, l_max, n)
    mag_y = log_uniform(rng, 1e-2, l_max, n)
    top = rng.random(n) < 0.1
    mag_x[top] = l_max * rng.uniform(0.9, 1.0, top.sum())
    return mag_x * rng.choice([-1.0, 1.0], n), mag_y * rng.choice([-1.0, 1.0], n)


def pair_deltas(rng, n):
    """Relative distance offsets: the adversarial set (each value as often as the others) and uniform ones."""
    adv = rng.choice(ADV_DELTAS, n)
    uni = rng.uniform(-1e-2, 1e-2, n)
    return np.where(rng.random(n) < 0.75, adv, uni)


def smallest(mask, key, cols):
    """The counterexample with the smallest `key` among `mask`, as a readable dict."""
    idx = np.flatnonzero(mask)
    i = idx[np.argmin(key[idx])]
    return {k: np.asarray(v[i]).tolist() for k, v in cols.items()} | {"count": int(mask.sum())}


def pairs(rng, n, r_point, ego):
    """n (point, obstacle) pairs in the map frame around `ego`: the obstacle at r_point (1 + delta) from the point in a
    random direction.  Returns the float64 map-frame coordinates and the float32 instance-local ones the kernels use."""
    lx, ly = local_points(rng, n)
    delta = pair_deltas(rng, n)
    th = rng.uniform(0, 2 * np.pi, n)
    ox, oy = ego
    px, py = ox + lx, oy + ly
    qx = px + r_point * (1.0 + delta) * np.cos(th)
    qy = py + r_point * (1.0 + delta) * np.sin(th)
    return dict(px=px, py=py, qx=qx, qy=qy, delta=delta,
                fx=_f32(px - ox), fy=_f32(py - oy), cx=_f32(qx - ox), cy=_f32(qy - oy))


def radius_pairs(rng, n, relation):
    """(R_static, R_dyn) with R_static < R_dyn, > or ==."""
    a = log_uniform(rng, R_MIN, R_MAX, n)
    b = log_uniform(rng, R_MIN, R_MAX, n)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    if relation == "equal":
        return a, a.copy()
    return (lo, hi) if relation == "static<dyn" else (hi, lo)


N = 120_000


# ---- P1 / P2: the thresholds of k_evaluate's sink ----------------------------------------------------------------------

@pytest.mark.parametrize("ego", EGOS, ids=["origin", "far1", "far2"])
@pytest.mark.parametrize("relation", ["static<dyn", "static>dyn", "equal"])
def test_thresholds_bound_the_float32_distance(lib, ego, relation):
    """P1: a pair within the larger radius in float64 has a float32 distance <= thr.  P2: a pair whose float32 distance
    is <= thr_sure lies within the SMALLER radius in float64.  Both thresholds are taken at the tightest box that holds
    the point (the point itself, no margin): any box k_cull hands over contains it, and its thresholds are looser."""
    seed = 1000 + 7 * EGOS.index(ego) + ["static<dyn", "static>dyn", "equal"].index(relation)
    rng = np.random.default_rng(seed)
    r_s, r_d = radius_pairs(rng, N, relation)
    sq_s, sq_d = r_s * r_s, r_d * r_d
    sq_max, sq_min = np.maximum(sq_s, sq_d), np.minimum(sq_s, sq_d)
    # the obstacle sits at the boundary of the larger radius (P1's edge), of the smaller one (P2's) or of either kind
    which = rng.integers(0, 3, N)
    r_pt = np.where(which == 0, np.sqrt(sq_max), np.where(which == 1, np.sqrt(sq_min), np.where(rng.random(N) < .5,
                                                                                                r_s, r_d)))
    q = pairs(rng, N, r_pt, ego)
    d64 = sum_sq_unfused(q["px"] - q["qx"], q["py"] - q["qy"])
    d32 = sqdist32(lib, q["fx"], q["fy"], q["cx"], q["cy"])
    fc = filter_const(lib, sq_max, sq_min)
    pbox = np.stack([q["fx"], q["fy"], q["fx"], q["fy"]], 1)
    thr, sure = box_thresholds(lib, fc, pbox, np.zeros(N, np.float32))
    mag = np.abs(q["fx"]).astype(np.float64) + np.abs(q["fy"])
    cols = dict(R_static=r_s, R_dyn=r_d, px=q["px"], py=q["py"], qx=q["qx"], qy=q["qy"], delta=q["delta"],
                d64=d64, d32=d32, thr=thr, thr_sure=sure)
    # every relation places pairs on both sides of both radii
    assert (d64 <= sq_min).sum() > N // 10 and (d64 > sq_max).sum() > N // 10
    bad1 = (d64 <= sq_max) & ~(d32.astype(np.float64) <= thr)
    assert not bad1.any(), f"P1 (miss bound) fails, ego {ego}, {relation}: {smallest(bad1, mag, cols)}"
    bad2 = (d32 <= sure) & ~(d64 <= sq_min)
    assert not bad2.any(), f"P2 (sure bound) fails, ego {ego}, {relation}: {smallest(bad2, mag, cols)}"
    # the band between the thresholds (where the float64 re-check runs) is narrow near the ego: pairs 5 % inside the
    # smaller radius are certain hits there, 5 % outside the larger one certain misses (bounds that are never reached
    # would test nothing)
    near = mag < 1.0
    assert (d32 <= sure)[near & (d64 < 0.95 * sq_min)].all()
    assert (d32 > thr)[near & (d64 > 1.05 * sq_max)].all()


def test_thresholds_hold_for_every_point_of_the_box(lib):
    """box_thresholds() promises its two values for every point of the box grown by m: filter_threshold grows and
    filter_threshold_sure shrinks with |px| + |py|, and the box's bound of |x| + |y| is taken per axis."""
    rng = np.random.default_rng(2024)
    n = 200_000
    cx, cy = local_points(rng, n)
    hw, hh = log_uniform(rng, 1e-3, 300.0, n), log_uniform(rng, 1e-3, 300.0, n)
    boxes = _f32(np.stack([cx - hw, cy - hh, cx + hw, cy + hh], 1))
    m = _f32(log_uniform(rng, 1e-3, 10.0, n))
    r = log_uniform(rng, R_MIN, R_MAX, n)
    fc = filter_const(lib, r * r, (r * rng.uniform(0.3, 1.0, n)) ** 2)
    thr, sure = box_thresholds(lib, fc, boxes, m)
    # points inside the grown box, its corners included
    t = rng.random((n, 2))
    corner = rng.random(n) < 0.3
    t[corner] = np.round(t[corner])
    b64 = boxes.astype(np.float64)
    px = _f32((b64[:, 0] - m) + t[:, 0] * ((b64[:, 2] + m) - (b64[:, 0] - m)))
    py = _f32((b64[:, 1] - m) + t[:, 1] * ((b64[:, 3] + m) - (b64[:, 1] - m)))
    inside = (px >= boxes[:, 0] - m) & (px <= boxes[:, 2] + m) & (py >= boxes[:, 1] - m) & (py <= boxes[:, 3] + m)
    pthr, psure = filter_thresholds(lib, fc, px, py)
    cols = dict(box=list(boxes), m=m, px=px, py=py, thr=thr, point_thr=pthr, thr_sure=sure, point_sure=psure)
    key = np.abs(px).astype(np.float64) + np.abs(py)
    bad = inside & ~(pthr <= thr)
    assert not bad.any(), f"thr of a box is below a point's own: {smallest(bad, key, cols)}"
    bad = inside & ~(psure >= sure)
    assert not bad.any(), f"thr_sure of a box is above a point's own: {smallest(bad, key, cols)}"
    # and the box's values are the point's own at the bound itself
    pt, ps = filter_thresholds(lib, fc, np.maximum(np.abs(boxes[:, 0]), np.abs(boxes[:, 2])) + m,
                               np.maximum(np.abs(boxes[:, 1]), np.abs(boxes[:, 3])) + m)
    np.testing.assert_array_equal(pt, thr)
    np.testing.assert_array_equal(ps, sure)


def test_filter_const_rounds_the_radii_outward(lib):
    """filter_const: sq rounds to nearest (thr's slack covers it), sq_lo lies below the smaller float64 radius, and
    the thresholds at the origin straddle it -- the ordering both bounds are built on."""
    rng = np.random.default_rng(7)
    n = 100_000
    a, b = log_uniform(rng, R_MIN, R_MAX, n), log_uniform(rng, R_MIN, R_MAX, n)
    sq, sq_min = np.maximum(a, b) ** 2, np.minimum(a, b) ** 2
    fc = filter_const(lib, sq, sq_min)
    assert (fc[:, 2].astype(np.float64) < sq_min).all()
    assert (np.abs(fc[:, 0].astype(np.float64) - sq) <= sq * 2.0 ** -24).all()
    np.testing.assert_array_equal(fc[:, 1], _f32(np.sqrt(fc[:, 0]).astype(np.float32) + np.float32(1.0)))
    zeros = np.zeros(n, np.float32)
    thr, sure = filter_thresholds(lib, fc, zeros, zeros)
    assert (thr.astype(np.float64) > sq).all() and (sure.astype(np.float64) < sq_min).all()


# ---- P3: k_cull's box ------------------------------------------------------------------------------------------------

FOOTPRINTS = ((), (0.0,), (-1.0, 0.5, 2.0), (-2.1, -1.5, -0.9, -0.3, 0.3, 0.9, 1.5, 2.1),
              (-3.75, -2.5, -1.25, 0.0, 1.25, 2.5, 3.75, 4.9))


@pytest.mark.parametrize("fp", range(len(FOOTPRINTS)), ids=lambda i: f"circles{len(FOOTPRINTS[i])}")
def test_cull_box_keeps_every_obstacle_within_reach(lib, fp):
    """P3: an obstacle within max(R) of a footprint circle centre of any point on the float64 segment between a box's two
    lateral extremes lies inside the float32 box of that segment (segment_box) grown by cull_margin + the footprint
    slack.  A single segment is the tightest box k_cull builds: merging boxes only grows the box and its margin."""
    offsets = FOOTPRINTS[fp]
    assert len(offsets) <= lib.bnd_max_circles()
    slack = np.float32(footprint_slack(lib, offsets))
    assert slack >= np.float32(max((abs(o) for o in offsets), default=0.0))
    rng = np.random.default_rng(300 + fp)
    n = N
    egos = np.array(EGOS)[rng.integers(0, len(EGOS), n)]
    ox, oy = egos[:, 0], egos[:, 1]
    lx, ly = local_points(rng, n)
    rx, ry = ox + lx, oy + ly
    th = rng.uniform(0, 2 * np.pi, n)
    cs, sn = np.cos(th), np.sin(th)
    d0 = rng.uniform(-8.0, 8.0, n)
    d1 = np.where(rng.random(n) < 0.2, d0, rng.uniform(-8.0, 8.0, n))      # brake-ladder entries: one offset
    box = segment_box(lib, rx, ry, cs, sn, d0, d1, ox, oy)
    # a point of the segment (its ends included), a circle centre off it along the path heading
    t = np.where(rng.random(n) < 0.3, np.round(rng.random(n)), rng.random(n))
    d = d0 + t * (d1 - d0)
    sx, sy = rx - sn * d, ry + cs * d
    if offsets:
        off = np.array(offsets)[rng.integers(0, len(offsets), n)]
        hd = th + rng.uniform(-0.6, 0.6, n)
        sx, sy = sx + off * np.cos(hd), sy + off * np.sin(hd)
    r_s, r_d = radius_pairs(rng, n, ["static<dyn", "static>dyn", "equal"][fp % 3])
    sq_max = np.maximum(r_s, r_d) ** 2
    delta = np.minimum(pair_deltas(rng, n), 0.0) - np.where(rng.random(n) < 0.5, 0.0, 2.0 ** -52)
    phi = np.where(rng.random(n) < 0.5, rng.integers(0, 4, n) * (np.pi / 2) + th, rng.uniform(0, 2 * np.pi, n))
    qx = sx + np.sqrt(sq_max) * (1.0 + delta) * np.cos(phi)
    qy = sy + np.sqrt(sq_max) * (1.0 + delta) * np.sin(phi)
    within = sum_sq_unfused(sx - qx, sy - qy) <= sq_max
    assert within.mean() > 0.5
    m = cull_margin(lib, sq_max, box) + slack
    ins = cull_inside(lib, box, m, _f32(qx - ox), _f32(qy - oy))
    bad = within & ~ins
    key = np.abs(box).max(1).astype(np.float64)
    cols = dict(ego_x=ox, ego_y=oy, rx=rx, ry=ry, heading=th, d0=d0, d1=d1, qx=qx, qy=qy, sq_max=sq_max,
                box=list(box), margin=m, delta=delta)
    assert not bad.any(), f"P3 (cull box) drops an obstacle within reach, circles {offsets}: {smallest(bad, key, cols)}"
    # the margin is tight enough to matter: obstacles 2 cm beyond the reach of a small box are culled
    far = (key < 50.0) & (np.abs(box[:, 2] - box[:, 0]) < 1e-3)
    if far.any():
        gx = box[far, 2] + m[far] + 0.02
        assert not cull_inside(lib, box[far], m[far], gx, box[far, 1]).any()


def test_cull_margin_covers_the_rounding_of_large_boxes(lib):
    """cull_margin's relative term against the float32 rounding the cull test meets, as a bound in its own right: at
    L_MAX the rounding of the obstacle, of the box corner and of b.x0 - m is three half-ulps of the coordinate, far
    above the fixed 1 mm slack."""
    for mag in (1.0, 2.0e3, 1.0e4, L_MAX):
        box = _f32([[mag, -mag, mag, -mag]])
        ulp = float(np.spacing(np.float32(mag)))
        m = float(cull_margin(lib, [0.25], box)[0])
        assert m - 0.5 * 1.000001 - 1e-3 >= 1.5 * ulp, (mag, m, ulp)


# ---- P4: strips ------------------------------------------------------------------------------------------------------

def test_strip_range_holds_every_reachable_entry(lib):
    """P4: for a step box and its entries ordered by bin (bin_map / bin_of, counted and prefixed as k_cull does), the
    chunk range strip_range() gives a tile box contains every entry within max(R) of a point of that tile box --
    entries exactly on the bin edges (lo + j / inv_w, and one float32 ulp either side) included -- and every entry that
    is the float32 rounding of an obstacle placed in float64 within R of a float64 point of one of the tile's segments
    (the rounding the strip margin has to absorb)."""
    rng = np.random.default_rng(4040)
    CB = lib.bnd_cull_bins()
    trials = 3000
    bad = []
    n_checked = n_edge_checked = n_path_checked = 0
    for it in range(trials):
        ox, oy = EGOS[it % len(EGOS)]
        r = float(log_uniform(rng, R_MIN, R_MAX, 1)[0])
        sq = r * r
        # the step box: merged segments of a few profiles around a random local centre (either axis the longer one)
        cx, cy = (v[0] for v in local_points(rng, 1, l_max=[10.0, 2.0e3, L_MAX][it % 3]))
        n_seg = int(rng.integers(1, 7))
        th = rng.uniform(0, 2 * np.pi) + rng.normal(0, 0.05, n_seg)
        along = np.sort(rng.uniform(0, float(log_uniform(rng, 0.5, 200.0, 1)[0]), n_seg))
        rx = ox + cx + along * np.cos(th)
        ry = oy + cy + along * np.sin(th)
        d0, d1 = rng.uniform(-8, 0, n_seg), rng.uniform(0, 8, n_seg)
        segs = segment_box(lib, rx, ry, np.cos(th), np.sin(th), d0, d1, np.full(n_seg, ox), np.full(n_seg, oy))
        step = _f32([[segs[:, 0].min(), segs[:, 1].min(), segs[:, 2].max(), segs[:, 3].max()]])
        mw = cull_margin(lib, [sq], step) + np.float32(0.0)
        axis, lo, inv_w = bin_map(lib, step, mw)
        # entries: random ones in the grown box, and the bin edges along the axis with random cross coordinates
        n_rand = int(rng.integers(0, 200))
        g = step[0].astype(np.float64)
        ex = rng.uniform(g[0] - mw[0], g[2] + mw[0], n_rand)
        ey = rng.uniform(g[1] - mw[0], g[3] + mw[0], n_rand)
        edges = _f32(lo[0] + np.arange(CB + 1, dtype=np.float32) / inv_w[0])
        edges = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))])
        cross_lo, cross_hi = (g[1], g[3]) if axis[0] == 0 else (g[0], g[2])
        cross = rng.uniform(cross_lo - mw[0], cross_hi + mw[0], len(edges))
        # ... and obstacles placed in float64 within R of a float64 point of one segment (what the kernels meet: the
        # entry is the float32 rounding of obstacle - ego, the tile box the float32 hull of the segments' ends)
        n_path = 64
        si = rng.integers(0, n_seg, n_path)
        dq = d0[si] + rng.random(n_path) * (d1[si] - d0[si])
        qx, qy = rx[si] - np.sin(th[si]) * dq, ry[si] + np.cos(th[si]) * dq
        delta = np.minimum(pair_deltas(rng, n_path), 0.0)
        phi = rng.uniform(0, 2 * np.pi, n_path)
        px_, py_ = qx + r * (1.0 + delta) * np.cos(phi), qy + r * (1.0 + delta) * np.sin(phi)
        within64 = sum_sq_unfused(px_ - qx, py_ - qy) <= sq
        n_grid = n_rand + len(edges)
        exy = np.concatenate([np.stack([ex, ey], 1),
                              np.stack([edges, cross], 1) if axis[0] == 0 else np.stack([cross, edges], 1),
                              np.stack([px_ - ox, py_ - oy], 1)])
        exy = _f32(exy)
        n_ent = len(exy)
        bins = bin_of(lib, np.full(n_ent, axis[0]), np.full(n_ent, lo[0]), np.full(n_ent, inv_w[0]), exy[:, 0], exy[:, 1])
        assert ((bins >= 0) & (bins < CB)).all()
        cnt = np.bincount(bins, minlength=CB)
        starts = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        # tiles: each single segment, each run of neighbouring segments, and the whole step box
        spans = [(i, j) for i in range(n_seg) for j in range(i, n_seg)]
        tiles = [segs[i:j + 1] for i, j in spans]
        wbs = _f32([[t[:, 0].min(), t[:, 1].min(), t[:, 2].max(), t[:, 3].max()] for t in tiles])
        nt = len(wbs)
        wm = cull_margin(lib, np.full(nt, sq), wbs)
        rng_ = strip_range(lib, np.full(nt, axis[0]), np.full(nt, lo[0]), np.full(nt, inv_w[0]), wbs, wm,
                           np.repeat(starts[None], nt, 0))
        c_lo, c_hi = (rng_ >> 16).astype(np.int64), (rng_ & 0xFFFF).astype(np.int64)
        e64 = exy.astype(np.float64)
        for w in range(nt):
            b = wbs[w].astype(np.float64)
            gx = np.maximum(np.maximum(b[0] - e64[:, 0], e64[:, 0] - b[2]), 0.0)
            gy = np.maximum(np.maximum(b[1] - e64[:, 1], e64[:, 1] - b[3]), 0.0)
            reach = gx * gx + gy * gy <= sq
            reach[n_grid:] = within64 & (si >= spans[w][0]) & (si <= spans[w][1])
            for j in np.flatnonzero(reach):
                n_checked += 1
                n_edge_checked += n_rand <= j < n_grid
                n_path_checked += j >= n_grid
                first, end = starts[bins[j]], starts[bins[j] + 1]
                if not (c_lo[w] * 8 <= first and end <= c_hi[w] * 8):
                    bad.append(dict(trial=it, tile=w, entry=exy[j].tolist(), bin=int(bins[j]),
                                    bin_entries=(int(first), int(end)), chunks=(int(c_lo[w]), int(c_hi[w])),
                                    tile_box=wbs[w].tolist(), step_box=step[0].tolist(), axis=int(axis[0]),
                                    lo=float(lo[0]), inv_w=float(inv_w[0]), R=r, on_edge=bool(n_rand <= j < n_grid),
                                    from_float64_path_point=bool(j >= n_grid)))
    assert n_checked > 50_000 and n_edge_checked > 5_000 and n_path_checked > 50_000
    if bad:
        worst = min(bad, key=lambda d: abs(d["entry"][0]) + abs(d["entry"][1]))
        pytest.fail(f"P4 (strips): {len(bad)} reachable entries outside their tile's chunk range; smallest: {worst}")


def test_strip_range_of_an_empty_box_is_empty(lib):
    axis, lo, inv_w = np.zeros(1, np.int32), _f32([0.0]), _f32([1.0])
    empty = _f32([[np.inf, np.inf, -np.inf, -np.inf]])
    starts = np.arange(33, dtype=np.int32)[None] * 8
    assert strip_range(lib, axis, lo, inv_w, empty, _f32([1.0]), starts)[0] == 0
