"""The long road of the long-path tests and what is placed on it.

ONE road for every knot count: a path of n knots is the first n waypoints of it (step lengths uniform in 1 - 4 m, heading a
random walk of sigma 0.05 rad per step -- a map-derived path of hundreds to thousands of waypoints).  Used by
tests/golden/make_golden.py --only long (the reference's answers on it), tests/test_long_paths_cpu.py and
tests/test_gpu_long_paths.py / test_gpu_spline_eval.py, so that all of them speak of the same knots.
"""
import numpy as np

ROAD_SEED = 20260
ROAD_MAX_KNOTS = 4000

# the staging limits of the three plan kernels (csrc/fot_kernels.hip: launch_evaluate, launch_cull, SPLINE_LDS_KNOTS)
EVAL_LDS_KNOTS, CULL_LDS_KNOTS, FRENET_LDS_KNOTS = 28, 64, 512


def road(n):
    """The first n waypoints (wx, wy) of the road."""
    assert 2 <= n <= ROAD_MAX_KNOTS, n
    rng = np.random.default_rng(ROAD_SEED)
    step = rng.uniform(1.0, 4.0, ROAD_MAX_KNOTS)
    heading = np.cumsum(rng.normal(0.0, 0.05, ROAD_MAX_KNOTS))
    return np.cumsum(step * np.cos(heading))[:n].copy(), np.cumsum(step * np.sin(heading))[:n].copy()


def pose_at(sp, s, d=0.0):
    """(x, y, yaw) at arc length s of the oracle spline `sp`, d metres to the left of it."""
    x, y, yaw, _, _ = (float(v[0]) for v in sp.eval(np.array([float(s)])))
    return x - d * np.sin(yaw), y + d * np.cos(yaw), yaw


def to_pose(points, pose, shift=(0.0, 0.0)):
    """Points [..., 2] given in a frame whose origin is the ego heading along +x, moved to `pose` = (x, y, yaw), after
    `shift` is subtracted in the frame itself."""
    p = np.asarray(points, dtype=np.float64) - np.asarray(shift, dtype=np.float64)
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.stack([pose[0] + c * p[..., 0] - s * p[..., 1], pose[1] + s * p[..., 0] + c * p[..., 1]], axis=-1)


def crossing_pedestrians(rng, n_ped, n_samples, T=51, dt=0.1):
    """[S, P, T, 2] in the ego's frame: pedestrians that start 2.5 - 9 m beside the lane, 4 - 28 m ahead, and cross it at walking
    pace, every sample a jittered copy of the same walk."""
    x0 = rng.uniform(4.0, 28.0, n_ped)
    side = rng.choice([-1.0, 1.0], n_ped)
    y0 = side * rng.uniform(2.5, 9.0, n_ped)
    vx = rng.normal(0.0, 0.3, n_ped)
    vy = -side * rng.uniform(0.2, 1.3, n_ped)
    t = np.arange(T) * dt
    base = np.stack([x0[:, None] + vx[:, None] * t, y0[:, None] + vy[:, None] * t], axis=-1)        # [P, T, 2]
    jitter = rng.normal(0.0, 0.15, (n_samples, n_ped, 1, 2)) + rng.normal(0.0, 0.05, (n_samples, n_ped, 1, 2)) * t[:, None]
    return base[None] + jitter


# ------------------------------------------------------------------------------------------------ GPU tests: egos on the road
# planner constants of scenario_01 (tests/golden/make_golden.py SCEN01, which --only long checks this against)
PLANNER = dict(max_speed=10.0, max_accel=2.0, max_curvature=0.2, max_lat_accel=3.0, dt=0.1, d_road_w=0.3,
               max_road_width=2.7, robot_radius=1.0, obstacle_radius=0.2, min_t=4.0, max_t=5.0,
               d_t_s=5.0 / 3.6, k_j=1.0, k_t=1.0, k_d=1.0, k_s_dot=1.0, k_lat=1.0, k_lon=1.0)
EGO_KINDS = ("start", "mid", "near_end", "beyond_end", "prev_s_exact", "prev_s_stale", "standing_tie", "frenet_given")
MID, NEAR_END = 1, 2
_cache = {}


def spline(n):
    """(oracle spline, arc length of its end) of the road's first n waypoints."""
    from oracle import oracle as orc
    if ("sp", n) not in _cache:
        sp = orc.Spline(*road(n))
        _cache["sp", n] = (sp, float(sp.coeffs()[0][-1]))
    return _cache["sp", n]


def egos(n):
    """The eight egos of EGO_KINDS on the path of n knots, each with 12 pedestrians x 4 samples near it and a few static
    points, and what the oracle plans for them: [(PlanRequest, PlanOutput)] (candidate tables for MID and NEAR_END).
    Computed once per knot count and left unchanged."""
    import dataclasses
    from integrated_path_planning_amd.batch import PlanRequest
    from oracle import oracle as orc
    from oracle.check import oracle_plan_for_request
    if ("egos", n) in _cache:
        return _cache["egos", n]
    sp, s_end = spline(n)
    params = orc.make_params(**PLANNER)
    rng = np.random.default_rng([n, 77])
    ex, ey, eyaw = pose_at(sp, s_end)
    at = dict(start=(0.0, 0.3), mid=(0.5 * s_end, -0.5), near_end=(s_end - 1.0, 0.2), prev_s_exact=(0.3 * s_end, 0.4),
              prev_s_stale=(0.7 * s_end, -0.3), standing_tie=(0.25 * s_end, 0.0), frenet_given=(0.4 * s_end, 0.6))
    out = []
    for kind in EGO_KINDS:
        if kind == "beyond_end":                                            # 2 m past the end, 3 m beside the tangent there
            pose = (ex + 2.0 * np.cos(eyaw) - 3.0 * np.sin(eyaw), ey + 2.0 * np.sin(eyaw) + 3.0 * np.cos(eyaw), eyaw)
            s = s_end
        else:
            s, d = at[kind]
            pose = pose_at(sp, s, d)
        obst = dict(dist=to_pose(crossing_pedestrians(rng, 12, 4), pose),
                    static=to_pose([[9.0, 1.6], [17.0, -1.3], [26.0, 0.2], [-5.0, 0.0]], pose))
        rq = PlanRequest(x=pose[0], y=pose[1], yaw=pose[2] + float(rng.normal(0.0, 0.03)), v=float(rng.uniform(3.0, 6.0)),
                         a=float(rng.uniform(-0.5, 0.5)), target_speed=6.0, last_kappa=float(rng.normal(0.0, 0.005)), **obst)
        if kind == "prev_s_exact":
            rq.prev_s = float(s)
        elif kind == "prev_s_stale":
            rq.prev_s = float(s - 25.0)
        elif kind == "standing_tie":                                        # v = 0 on its own previous arc length: the
            rq.v, rq.a, rq.prev_s = 0.0, 0.0, float(s)                      # window's samples 49 and 50 tie
        want = oracle_plan_for_request(orc, params, sp, rq, table=kind in ("mid", "near_end"))
        if kind == "frenet_given":                                          # the oracle's own Frenet state of this ego, handed
            assert want.status != orc.PLAN_C2F_FAILED                       # over as it is: no search, no new_prev_s
            f = [float(v) for v in want.frenet0]
            rq = PlanRequest(*f[:5], last_kappa=f[5], is_frenet=True, target_speed=rq.target_speed, **obst)
            want = dataclasses.replace(want, new_prev_s=float("nan"))
        out.append((rq, want))
    _cache["egos", n] = out
    return out
