"""The cases of tests/test_gpu_frenet_waves.py, and the child process that runs them.

k_frenet_state reads FOT_FRENET_WAVES once per process (`all`: every nearest-point block keeps its four waves to its end;
default: an instance that heads no chain goes on with one wave behind its last block-wide scan), so one child process per
setting runs every case and leaves what it got in a file:

    python3 tests/frenet_waves_common.py OUT.pkl

A case is (planner constants, waypoints, batches of requests[, eval paths]); everything is seeded, so the test and both
children build the same requests.
"""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import long_paths_common as lp  # noqa: E402
from integrated_path_planning_amd import synthetic as syn  # noqa: E402
from integrated_path_planning_amd.batch import PlanRequest, request_from_instance  # noqa: E402

KNOTS = (2, 11, 65, 513)                                         # 513: more than SPLINE_LDS_KNOTS, the path stays in HBM
STRAIGHT = (syn.STRAIGHT_WX, syn.STRAIGHT_WY)
# the largest lattice of the stored goldens (tests/golden/make_golden.py ARC: 29 lateral offsets)
ARC = dict(max_speed=13.9, max_accel=8.0, max_curvature=10.0, dt=0.1, d_road_w=0.5, max_road_width=7.0,
           robot_radius=1.0, min_t=4.0, max_t=5.0, d_t_s=1.39)


_roads = {}


def road_requests(n):
    """long_paths_common's eight egos on the road of n knots (no prev_s at the start, in the middle, near and beyond the
    end; prev_s with the winner inside the window; a stale prev_s below: the winner on the window's UPPER edge, then the
    global scan; a standing ego whose window ties; a given Frenet state) and three more: a stale prev_s above (LOWER
    edge), an ego behind the start of the path (refinement clamped at 0), and one beside the very end (clamped at s_end).
    [(request, the oracle's plan or None)]; computed once per knot count."""
    if n in _roads:
        return _roads[n]
    out = _roads[n] = list(lp.egos(n))
    sp, s_end = lp.spline(n)
    x, y, yaw = lp.pose_at(sp, 0.45 * s_end, 0.3)
    out.append((PlanRequest(x, y, yaw, 4.0, 0.1, target_speed=6.0, prev_s=float(min(s_end, 0.45 * s_end + 25.0))), None))
    x0, y0, yaw0 = lp.pose_at(sp, 0.0)
    out.append((PlanRequest(x0 - 1.5 * np.cos(yaw0) - 0.4 * np.sin(yaw0), y0 - 1.5 * np.sin(yaw0) + 0.4 * np.cos(yaw0), yaw0,
                            3.0, 0.0, target_speed=6.0), None))
    xe, ye, yawe = lp.pose_at(sp, s_end, -0.5)
    out.append((PlanRequest(xe + 0.05 * np.cos(yawe), ye + 0.05 * np.sin(yawe), yawe, 3.0, 0.0, target_speed=6.0,
                            prev_s=float(s_end)), None))
    return out


def chain_requests():
    """a solo instance, the head of a chain, its three members, and a solo one behind them: both paths in one launch"""
    rng = np.random.default_rng(5)
    dyn = np.array([25.0, 0.3]) + rng.normal(0, 5.0, (6, 1, 2)) + np.cumsum(rng.normal(0, 0.1, (6, 51, 2)), axis=1)
    kw = dict(dyn=dyn, static=np.column_stack([rng.uniform(5, 60, 12), rng.uniform(-5, 5, 12)]))
    head = dict(x=12.0, y=0.3, yaw=0.02, v=6.0, a=0.2)
    return [PlanRequest(20.0, 0.6, 0.05, 5.0, 0.2, target_speed=6.0, **kw),
            PlanRequest(**head, target_speed=0.0, prev_s=11.0, **kw),
            PlanRequest(**head, target_speed=4.5, chain_prev_s=True, overrides={"max_accel": 1.5}, **kw),
            PlanRequest(**head, target_speed=3.0, chain_prev_s=True, **kw),
            PlanRequest(**head, target_speed=6.0, chain_prev_s=True, overrides={"max_accel": 2.5}, **kw),
            PlanRequest(31.0, -0.4, 0.0, 4.0, 0.0, target_speed=6.0, prev_s=30.5, **kw)]


def bench_requests(n=5):
    return [request_from_instance(syn.config3_instance(s, S=4, P=8)) for s in range(n)]


def arc_requests():
    rng = np.random.default_rng(9)
    static = np.column_stack([rng.uniform(5, 60, 10), rng.uniform(-6, 6, 10)])
    return [PlanRequest(10.0 + 7.0 * i, 0.5 * i - 1.0, 0.03 * i, 3.0 + 2.0 * i, 0.1, target_speed=5.0 + i, static=static,
                        prev_s=None if i % 2 else 10.0 + 7.0 * i) for i in range(3)] + \
           [PlanRequest(30.0, 0.0, 0.0, 0.0, 0.0, target_speed=0.0, static=static)]          # standing: no brake ladder


def cases():
    """name -> (planner constants, waypoints, [batch of requests, ...], eval paths)"""
    out = {}
    for n in KNOTS:
        reqs = [rq for rq, _ in road_requests(n)]
        # 1, 3 and 5 instances per call (a block first, last and interior), then all of them
        batches = [reqs[:1], reqs[4:7], reqs[6:11], reqs] if n == 11 else [reqs]
        out[f"road_{n}"] = (lp.PLANNER, lp.road(n), batches, ("auto",))
    out["chain"] = (dict(syn.CONFIG2_PLANNER), STRAIGHT, [chain_requests()], ("auto",))
    out["heads_bench"] = (dict(syn.CONFIG3_PLANNER), STRAIGHT, [bench_requests()], ("group", "wave"))
    out["heads_arc"] = (ARC, STRAIGHT, [arc_requests()], ("group", "wave"))
    return out


def run_all():
    from helpers import set_eval_path
    from integrated_path_planning_amd.planner import BatchPlanner
    got = {}
    for name, (kw, wp, batches, paths) in cases().items():
        bp = BatchPlanner(waypoints=wp, **kw)
        runs = []
        for reqs in batches:
            run = {}
            cart = [r for r in reqs if not r.is_frenet and not r.chain_prev_s]
            run["frenet_states"] = [a.tobytes() for a in bp.frenet_states(cart)]
            for path in paths:
                set_eval_path(bp, path)
                res = bp.plan_batch(reqs)
                run[path] = [bytes(memoryview(res.records[i]).cast("B")) for i in range(len(reqs))]
            runs.append(run)
        got[name] = runs
        bp.close()
    return got


if __name__ == "__main__":
    with open(sys.argv[1], "wb") as f:
        pickle.dump(run_all(), f)
