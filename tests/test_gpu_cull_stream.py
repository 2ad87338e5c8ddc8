"""k_cull after the cut of its vector instruction stream: the shapes at which the re-cut code can go wrong.

What changed in k_cull (csrc/fot_kernels.hip cull_group) is index and address arithmetic -- 32-bit byte offsets into
the prediction tensor, the sample index j / P through a host-built reciprocal, the step of a flattened (step, profile)
index without a division, a guess-first segment lookup for the boxes, DPP forms of the wave reductions and of the bin
prefix, the lazy NaN bookkeeping's lane mask built on the scalar side -- and none of it shows in a result unless an
obstacle is kept or dropped wrongly, lands in the wrong bin or carries the wrong sample id.  Every case below therefore
holds

  * the records of the grouped, per-wave and split evaluation paths byte-identical to each other -- the path is exactly
    straight, so "group" and "split-wave" launch the flat kernels (asserted) and "group-noflat" / "split-noflat" the
    lean kernels a bent road runs on the same entry lists,
  * the records equal to the oracle's (oracle.check.assert_record_matches_oracle), and
  * the per-candidate status table (fot_debug_candidates) equal to the oracle's -- the collision statuses are what the
    entry lists decide,

in both dtypes and both tensor layouts ([S][P][T][2] and time-major), on the default lattice, two instances per call
(so the second instance's tensor starts at a non-zero dyn_off).  Obstacle positions are drawn so that the ORACLE ALONE
yields both colliding and free candidates in every instance of every case: test_every_case_decides_something checks
that on the CPU.  The oracle's plans are computed once per case and shared.
"""
import functools

import numpy as np
import pytest

import eps_band
from helpers import TIGHT, assert_flat_as_named, assert_record_matches_oracle, oracle_plan_for_request, set_eval_path
from integrated_path_planning_amd import synthetic as syn
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest
from oracle import oracle as orc
from oracle.check import STATUS_NAMES

WP = (syn.STRAIGHT_WX, syn.STRAIGHT_WY)
KW = syn.CONFIG3_PLANNER
COLLISION, OK = STATUS_NAMES.index("collision_error"), STATUS_NAMES.index("ok")
PATHS = ("group", "wave", "split-wave", "group-noflat", "split-noflat")


def _f32(a):
    """float64 arrays holding float32 values: the oracle and both device dtypes see the same numbers"""
    return np.asarray(a, np.float32).astype(np.float64)


def _points(rng, ego_x, n, inside):
    """n start points.  `inside`: all of them inside the step boxes of the lattice but on its left edge (so the right
    half of the lattice stays free); otherwise two blockers left of the lane centre ahead of the ego, the rest spread
    over the scene, most of it outside the boxes."""
    if inside:
        return np.stack([rng.uniform(ego_x + 4.0, ego_x + 30.0, n), rng.uniform(4.6, 6.9, n)], 1)
    p = np.stack([rng.uniform(ego_x - 10.0, ego_x + 70.0, n), rng.uniform(-22.0, 22.0, n)], 1)
    p[:, 1] += np.where(np.abs(p[:, 1]) < 3.0, 9.0, 0.0)              # (nothing else near the lane: the blockers decide)
    k = min(n, 2)
    p[:k, 0] = ego_x + rng.uniform(9.0, 16.0, k)
    p[:k, 1] = rng.uniform(2.4, 4.0, k)
    return p


def _tracks(rng, p0, S, T):
    """[S][P][T][2]: slow walkers that start at p0, a little sample noise"""
    P = len(p0)
    vel = rng.uniform(-0.15, 0.15, (1, P, 1, 2))
    t = (np.arange(T) * 0.1)[None, None, :, None]
    return p0[None, :, None, :] + vel * t + rng.normal(0.0, 0.02, (S, P, 1, 2))


def scene(seed, n_static=0, S=0, P=0, T=51, inside=False, nan_last=False):
    rng = np.random.default_rng(seed)
    ego = (float(rng.uniform(5.0, 25.0)), float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.03, 0.03)),
           float(rng.uniform(4.0, 6.5)), 0.0)
    n_dyn = P
    pts = _points(rng, ego[0], n_static + n_dyn, inside)
    rng.shuffle(pts[: max(n_static + n_dyn, 1)])                      # blockers: static or dynamic, wherever they fall
    static = _f32(pts[:n_static]) if n_static else None
    dist = None
    if S and P:
        d = _tracks(rng, pts[n_static:], S, T)
        if nan_last:
            # a track that blocks the lane centre -- and is no obstacle at all, for the NaN in its last sample
            d[:, 0, :, 0] = ego[0] + 10.0
            d[:, 0, :, 1] = 0.0
            d = _f32(d)
            d[S - 1, 0, T - 1, 1] = np.nan
        dist = _f32(d) if not nan_last else d
    return PlanRequest(x=ego[0], y=ego[1], yaw=ego[2], v=ego[3], a=ego[4], static=static, dist=dist)


def _split(n):
    """S, P with S * P = n and S the largest divisor of n up to 4"""
    s = max(k for k in (1, 2, 3, 4) if n % k == 0)
    return s, n // s


# name -> the two instances of the case (seed, keyword arguments of scene())
CASES = {}
for _n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):            # lane group 16, STRIDE 64, UNROLL x STRIDE 256
    _s, _p = _split(_n)
    CASES[f"dyn{_n}"] = [(100 + _n, dict(S=1, P=_n)), (200 + _n, dict(S=_s, P=_p))]
    CASES[f"static{_n}"] = [(300 + _n, dict(n_static=_n)), (400 + _n, dict(n_static=_n))]
    if _n > 1:
        _ns = max(1, _n // 3)
        CASES[f"both{_n}"] = [(500 + _n, dict(n_static=_ns, S=1, P=_n - _ns)),
                              (600 + _n, dict(n_static=_n - max(1, _n // 4), S=1, P=max(1, _n // 4)))]
for _t in (1, 2, 3, 5):                                          # rows clamped to T - 1; 51 steps end in a group of 3
    CASES[f"T{_t}"] = [(700 + _t, dict(S=2, P=13, T=_t)), (710 + _t, dict(n_static=3, S=3, P=7, T=_t))]
for _s, _p in ((5, 1), (1, 1), (1, 7), (3, 7), (4, 13), (2, 29), (64, 7), (64, 1)):   # sid = j / P at every remainder
    CASES[f"S{_s}xP{_p}"] = [(800 + 31 * _s + _p, dict(S=_s, P=_p)), (900 + 31 * _s + _p, dict(S=_s, P=_p, n_static=2))]
CASES["inside257dyn"] = [(1001, dict(S=1, P=257, inside=True)), (1002, dict(S=1, P=257, inside=True))]   # > CULL_LIST, > CULL_VER
CASES["inside257static"] = [(1003, dict(n_static=257, inside=True)), (1004, dict(n_static=200, S=1, P=57, inside=True))]
CASES["nan_last"] = [(1005, dict(S=1, P=9, nan_last=True)), (1006, dict(S=3, P=40, n_static=5, nan_last=True))]


@functools.lru_cache(maxsize=None)
def case_requests(name):
    return tuple(scene(seed, **kw) for seed, kw in CASES[name])


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    params, sp = orc.make_params(**KW), orc.Spline(*WP)
    return tuple(oracle_plan_for_request(orc, params, sp, rq, table=True) for rq in case_requests(name))


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_decides_something(name):
    """(CPU) the oracle alone finds colliding AND free candidates in every instance of the case, so a list that keeps
    too little, too much or the wrong sample shows in the status table"""
    for i, want in enumerate(case_oracle(name)):
        st = np.asarray(want.cand_status)
        assert (st == COLLISION).any() and (st == OK).any(), (name, i, np.bincount(st, minlength=8).tolist())
    if name == "nan_last":                                           # ... and the NaN track alone would have blocked the lane
        params, sp = orc.make_params(**KW), orc.Spline(*WP)
        rq = case_requests(name)[0]
        healed = PlanRequest(x=rq.x, y=rq.y, yaw=rq.yaw, v=rq.v, a=rq.a, static=rq.static, dist=np.nan_to_num(rq.dist, nan=0.0))
        other = oracle_plan_for_request(orc, params, sp, healed, table=True)
        assert (np.asarray(other.cand_status) == COLLISION).sum() > (np.asarray(case_oracle(name)[0].cand_status) == COLLISION).sum()


@pytest.fixture(scope="module")
def planner():
    from integrated_path_planning_amd.planner import BatchPlanner
    bp = BatchPlanner(waypoints=WP, **KW)
    yield bp
    bp.close()


def _rec_bytes(rec):
    return bytes(memoryview(rec).cast("B"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_lists_decide_what_the_oracle_decides(planner, name):
    bp = planner
    reqs = list(case_requests(name))
    wants = case_oracle(name)
    any_dyn = any(r.dist is not None for r in reqs)
    for dtype in (np.float32, np.float64):
        for tsp in ((False, True) if any_dyn else (False,)):
            first = None
            for path in PATHS:
                set_eval_path(bp, path)
                label = f"{name} {np.dtype(dtype).name} {'tsp' if tsp else 'spt'} [{path}]"
                res = bp.plan_packed(PackedBatch(reqs, dtype, dyn_layout_tsp=tsp))
                assert bp.last_eval_form() == "lean", label
                assert_flat_as_named(bp, path, True, label)
                recs = [_rec_bytes(res.records[i]) for i in range(len(reqs))]
                if first is None:
                    first = recs
                assert recs == first, f"{label}: records differ from the [{PATHS[0]}] path's"
                for i, want in enumerate(wants):
                    lab = f"{label} inst {i}"
                    assert_record_matches_oracle(res.records[i], want, label=lab)
                    cost, status, keep, nt = bp.candidates(i)
                    np.testing.assert_array_equal(keep, want.cand_keep, err_msg=lab)
                    np.testing.assert_allclose(cost, want.cand_cost, rtol=TIGHT, atol=TIGHT, err_msg=lab)
                    eps_band.check_status_table(bp, i, status, want.cand_status, lab)
    set_eval_path(bp, "auto")
