#!/usr/bin/env python3
"""The footprint re-verification study (A-4) on this library, and what it costs.

* ``campaign``: the reference's campaign shape as ONE resident loop -- every crowd of the closed-loop fixture under the
  planner conditions circle, multi_circle (3 circles) and multi_circle5, each slot on its own scenario and footprint, with
  the observational metrics on (``BatchedClosedLoop(..., footprint_obs=True)``): the per-run rows of
  ``observational_footprint_metrics`` -- geometry fixed across conditions -- without a step's pedestrians or egos leaving
  the device.
* ``lockstep``: what the keyword costs.  64 and 256 resident copies of the base episode with 30 pedestrians each, whole
  runs, keep_paths=False, keyword off and on in turn (A B A B ...) after a warm-up of each, medians with every run listed;
  ``--parent-tree DIR`` (a built checkout of the parent commit) adds ``off`` of both trees in alternating child processes.
* ``recheck``: the post-hoc recheck at the reference campaign's size -- 1980 trajectories x 300 steps x 30 pedestrians --
  as one ``fot_footprint_recheck`` call against the NumPy restatement (tests/footprint_obs_common.py) looping on the host
  over the same arrays (``--host-trajectories N``: the host loop over the first N only, its time scaled and marked so), with
  the bytes the call moves.
* ``accuracy``: the golden fixture through the library: the largest differences to the reference's answers.

    python3 scripts/footprint_benchmark.py --out profiles/r27_footprint_obs.json [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONDITIONS = {"circle": None, "multi_circle": 3, "multi_circle5": 5}
N_PEDS = 30

CHILD = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
z = np.load(sys.argv[2], allow_pickle=False)
cfg = json.loads(str(z["meta"]))["config"]
tracks = np.load(sys.argv[5])
n_epi = int(sys.argv[3])
out = []
for k in range(1 + int(sys.argv[4])):                                 # (the first run warms up)
    with BatchedClosedLoop(cfg, [tracks] * n_epi, resident=True) as loop:
        t0 = time.perf_counter()
        hists = loop.run(keep_paths=False)
        out.append((time.perf_counter() - t0) / len(hists[0]) * 1e3)
print(json.dumps(out[1:]))
"""


def crowd_of_30(tracks):
    """the base crowd widened to 30 pedestrians: its own 14 and copies of them 200 m and 400 m aside (they meet nobody)"""
    cols = [tracks]
    while sum(c.shape[1] for c in cols) < N_PEDS:
        cols.append(tracks + np.array([0.0, 200.0 * len(cols)]))
    return np.ascontiguousarray(np.concatenate(cols, axis=1)[:, :N_PEDS])


def condition_config(cfg, condition):
    c = dict(cfg)
    n = CONDITIONS[condition]
    c["ego_footprint"] = "circle" if n is None else "multi_circle"
    if n is not None:
        c["ego_footprint_n_circles"] = n
        c.setdefault("vehicle_length", 4.5)
        c.setdefault("vehicle_width", 2.0)
    return c


def campaign(z, meta):
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    crowds = [n for n in meta["variants"] if n + "_ped_traj" in z.files and meta["variants"][n]["config"].get("ego_footprint", "circle") == "circle"]
    runs = [(crowd, cond) for crowd in crowds for cond in CONDITIONS]
    cfgs = [condition_config(meta["variants"][crowd]["config"], cond) for crowd, cond in runs]
    t0 = time.perf_counter()
    with BatchedClosedLoop(cfgs, [z[crowd + "_ped_traj"] for crowd, _ in runs], resident=True, footprint_obs=True) as loop:
        hists = loop.run(keep_paths=False)
        rows = loop.footprint_metrics()
        reasons = [e.termination_reason for e in loop.episodes]
        scenarios = loop.engine.n_scenarios
    wall = time.perf_counter() - t0
    table = [dict(crowd=crowd, condition=cond, steps=len(h), termination_reason=r, **m)
             for (crowd, cond), h, r, m in zip(runs, hists, reasons, rows)]
    return {"runs": len(runs), "scenarios_on_the_handle": scenarios, "wall_s": wall, "rows": table}


def lockstep(z, cfg, tracks, episodes, repeats, parent_tree, fixture, tmp):
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop

    def one_run(n_epi, on):
        with BatchedClosedLoop(cfg, [tracks] * n_epi, resident=True, footprint_obs=True if on else None) as loop:
            t0 = time.perf_counter()
            hists = loop.run(keep_paths=False)
            if on:
                loop.footprint_metrics()
            wall = time.perf_counter() - t0
            return wall / len(hists[0]) * 1e3, len(hists[0]), loop.ego[0].tobytes()

    out = {}
    for n_epi in episodes:
        ends = [one_run(n_epi, on)[2] for on in (False, True)]
        assert ends[0] == ends[1], "the keyword changes the episodes"
        runs = {False: [], True: []}
        steps = 0
        for _ in range(repeats):
            for on in (False, True):
                ms, steps, _ = one_run(n_epi, on)
                runs[on].append(ms)
        row = {"lock_steps": steps, "pedestrians_per_episode": int(tracks.shape[1])}
        for on, name in ((False, "off"), (True, "on")):
            row[name] = {"median_ms_per_lock_step": float(np.median(runs[on])), "runs": [round(v, 5) for v in runs[on]],
                         "spread_ms": float(max(runs[on]) - min(runs[on]))}
        row["on_minus_off_us_per_lock_step"] = 1e3 * (row["on"]["median_ms_per_lock_step"] - row["off"]["median_ms_per_lock_step"])
        if parent_tree:
            np.save(tmp, tracks)
            sides = {"parent": os.path.abspath(parent_tree), "this": ROOT}
            got = {k: [] for k in sides}
            for _ in range(repeats):                               # parent, this, parent, this ...: one child process each
                for k, tree in sides.items():
                    p = subprocess.run([sys.executable, "-c", CHILD, tree, fixture, str(n_epi), "1", tmp], check=True,
                                       capture_output=True, text=True, timeout=600)
                    got[k] += json.loads(p.stdout.strip().splitlines()[-1])
            row["off_against_parent"] = {k: {"median_ms_per_lock_step": float(np.median(v)), "runs": [round(x, 5) for x in v]}
                                         for k, v in got.items()}
            row["off_against_parent"]["this_minus_parent_ms"] = float(np.median(got["this"]) - np.median(got["parent"]))
            row["off_against_parent"]["parent_spread_ms"] = float(max(got["parent"]) - min(got["parent"]))
        out[str(n_epi)] = row
    return out


def recheck(fc, n_traj, n_steps, host_trajectories, repeats):
    from integrated_path_planning_amd import safety, synthetic as syn
    from integrated_path_planning_amd.planner import BatchPlanner
    rng = np.random.default_rng(27)
    heading = np.cumsum(rng.normal(0.0, 0.02, (n_traj, n_steps)), axis=1) + rng.uniform(-np.pi, np.pi, (n_traj, 1))
    x, y = np.cumsum(0.5 * np.cos(heading), axis=1), np.cumsum(0.5 * np.sin(heading), axis=1)
    steps = n_traj * n_steps
    xy = np.stack([x.reshape(-1), y.reshape(-1)], axis=1)
    ped_xy = (xy[:, None, :] + rng.uniform(-15.0, 15.0, (steps, N_PEDS, 2))).reshape(-1, 2)
    step_off = (np.arange(n_traj + 1) * n_steps).astype(np.int32)
    ped_off = (np.arange(steps + 1) * N_PEDS).astype(np.int32)
    yaw = heading.reshape(-1)
    geom = safety.footprint_geometry()
    out = {"trajectories": n_traj, "steps": n_steps, "pedestrians": N_PEDS}
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        for mode, head in (("stored_yaw", yaw), ("reconstructed_yaw", None)):
            bp.footprint_recheck(geom, step_off, xy, head, ped_off, ped_xy)                   # warm-up
            t = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                rec, _, _ = bp.footprint_recheck(geom, step_off, xy, head, ped_off, ped_xy)
                t.append(time.perf_counter() - t0)
            out[mode] = {"one_call_ms": {"median": float(np.median(t)) * 1e3, "runs": [round(v * 1e3, 3) for v in t]},
                         "bytes_to_device": int(step_off.nbytes + ped_off.nbytes + xy.nbytes + ped_xy.nbytes + (yaw.nbytes if head is not None else 0)),
                         "bytes_to_host": int(rec.nbytes)}
            # the host loop over the same arrays (a part of them, scaled, when asked)
            k = n_traj if host_trajectories <= 0 else min(host_trajectories, n_traj)
            case = dict(step_off=step_off[:k + 1], xy=xy[:k * n_steps], yaw=yaw[:k * n_steps], ped_off=ped_off[:k * n_steps + 1],
                        ped_xy=ped_xy[:k * n_steps * N_PEDS])
            t0 = time.perf_counter()
            want = fc.recheck(case, reconstruct=head is None)[0]
            host = time.perf_counter() - t0
            out[mode]["numpy_host_loop_s"] = {"measured_over_trajectories": k, "measured": host, "scaled_to_all": host * n_traj / k}
            tol = fc.dist_tol(fc.magnitude(xy, ped_xy))
            out[mode]["largest_difference_to_the_host_loop"] = fc.assert_records_close(rec[:k], want, tol, mode)
            out[mode]["bound"] = tol
    return out


def accuracy(fc):
    from integrated_path_planning_amd import safety, synthetic as syn
    from integrated_path_planning_amd.planner import BatchPlanner
    fix = fc.load_cases()
    worst = {"distance": 0.0, "distance_bound_of_that_case": 0.0, "heading": 0.0, "heading_bound": fc.YAW_TOL}
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        for name, info in fix["meta"]["cases"].items():
            case = fc.golden_case(fix, info["inputs"])
            tol = fc.dist_tol(info["M"])
            geom = safety.footprint_geometry(info["geom"])
            _, series, _ = bp.footprint_recheck(geom, case["step_off"], case["xy"], case["yaw"], case["ped_off"], case["ped_xy"],
                                                want_series=True)
            got = np.stack([series["legacy"], series["multi"], series["rect"]], axis=1)
            d = fc.assert_close(got, fix[name + "_series"], tol, name)
            if d > worst["distance"]:
                worst.update(distance=d, distance_bound_of_that_case=tol, distance_case=name)
            if np.all(np.diff(case["step_off"]) >= 2):
                _, _, used = bp.footprint_recheck(geom, case["step_off"], case["xy"], None, case["ped_off"], case["ped_xy"], want_yaw=True)
                worst["heading"] = max(worst["heading"], fc.assert_close(used, fix[name + "_yaw_recon"], fc.YAW_TOL, name))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", nargs="+", default=["campaign", "lockstep", "recheck", "accuracy"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--trajectories", type=int, default=1980)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--host-trajectories", type=int, default=0, help="the host loop over the first N trajectories only (0: all)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import footprint_obs_common as fc
    fixture = os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz")
    z = np.load(fixture, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    result = {"what": "footprint re-verification: the campaign as one loop, the keyword's cost per lock step, the post-hoc "
                      "recheck in one call, the accuracy on the golden fixture", "repeats": args.repeats}
    if "campaign" in args.parts:
        result["campaign"] = campaign(z, meta)
    if "lockstep" in args.parts:
        tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"footprint_bench_tracks_{os.getpid()}.npy")
        result["lockstep"] = lockstep(z, meta["config"], crowd_of_30(z["base_ped_traj"]), args.episodes, args.repeats,
                                      args.parent_tree, fixture, tmp)
        if os.path.exists(tmp):
            os.remove(tmp)
    if "recheck" in args.parts:
        result["recheck"] = recheck(fc, args.trajectories, args.steps, args.host_trajectories, args.repeats)
    if "accuracy" in args.parts:
        result["accuracy"] = accuracy(fc)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
