#!/usr/bin/env python3
"""What the episode summaries of the resident loop cost and what they replace (fot_loop_summary_enable /
fot_loop_summaries, BatchedClosedLoop(resident=True, summaries=True)).  scenario_01's base episode, 64 and 256 copies
advanced together, whole runs, in the manner of scripts/loop_run_bench.py: one process, a warm-up run of each form, then
the forms in turn (A B A B ...), median of --repeats runs each.

* ``off`` / ``on``: ms per lock step of resident=True, keep_paths=False without and with summaries (``on`` includes the
  one aggregate_metrics() call at the end of the run);
* ``campaign``: wall time from the first step to per-episode summaries -- the new path (run(keep_paths=False) +
  aggregate_metrics()) against what the same user does without the feature: run() with the followed paths, then the
  NumPy restatement of the reference's metric code over every EpisodeHistory (tests/summary_common.py), which rebuilds
  every step's record and recomputes its prediction;
* ``--parent-tree DIR``: a built checkout of the parent commit.  ``off`` of this tree and of the parent are then measured
  in alternating child processes (the parent's library has another ABI and cannot share a process with this binding),
  --repeats children each: the off path must launch nothing new, so the two must agree within the spread of the
  parent's own repeats.

    python3 scripts/loop_summary_bench.py --out profiles/r08_loop_summary.json [--parent-tree DIR]
    python3 scripts/loop_summary_bench.py --only on --episodes 64          # one form alone, for a kernel trace
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
z = np.load(sys.argv[2], allow_pickle=False)
cfg = json.loads(str(z["meta"]))["config"]
n_epi = int(sys.argv[3])
out = []
for k in range(1 + int(sys.argv[4])):                                 # (the first run warms up)
    with BatchedClosedLoop(cfg, [z["base_ped_traj"]] * n_epi, resident=True) as loop:
        t0 = time.perf_counter()
        hists = loop.run(keep_paths=False)
        out.append((time.perf_counter() - t0) / len(hists[0]) * 1e3)
print(json.dumps(out[1:]))
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only", choices=["off", "on"], default=None, help="one form alone (for a kernel trace)")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--campaign-repeats", type=int, default=1, help="runs of the host-side restatement (slow)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    fixture = os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz")
    z = np.load(fixture, allow_pickle=False)
    cfg = json.loads(str(z["meta"]))["config"]

    def one_run(n_epi, form):
        with BatchedClosedLoop(cfg, [z["base_ped_traj"]] * n_epi, resident=True, summaries=form == "on") as loop:
            t0 = time.perf_counter()
            hists = loop.run(keep_paths=False)
            agg = loop.aggregate_metrics() if form == "on" else None
            wall = time.perf_counter() - t0
            t1 = time.perf_counter()
            if form == "on":
                loop.aggregate_metrics()
            t_summary = time.perf_counter() - t1
            steps = len(hists[0])
            end = (loop.episodes[0].termination_reason, loop.ego[0].tobytes())
        return wall / steps * 1e3, steps, end, wall, t_summary, agg

    def host_campaign(n_epi):
        """what a user of the parent commit does: every step's records back, the metric code over Python objects"""
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from summary_common import summary_of_history
        with BatchedClosedLoop(cfg, [z["base_ped_traj"]] * n_epi, resident=True) as loop:
            t0 = time.perf_counter()
            hists = loop.run()
            t_run = time.perf_counter() - t0
            agg = [summary_of_history(h, cfg["dt"], 0.4, cfg["pred_len"], cfg.get("num_samples", 1)) for h in hists]
            wall = time.perf_counter() - t0
        return wall, t_run, agg

    forms = [args.only] if args.only else ["off", "on"]
    result = {"what": "episode summaries of the resident loop, whole runs of scenario_01's base episode", "repeats": args.repeats,
              "order": "warm-up of every form, then " + " ".join(forms) + " repeated", "episodes": {}}
    for n_epi in args.episodes:
        ends = {f: one_run(n_epi, f)[2] for f in forms}           # warm-up: code objects, workspace, fresh memory
        runs = {f: [] for f in forms}
        walls = {f: [] for f in forms}
        t_sum, steps, agg_on = [], 0, None
        for _ in range(args.repeats):
            for f in forms:
                ms, steps, end, wall, ts, agg = one_run(n_epi, f)
                runs[f].append(ms)
                walls[f].append(wall)
                assert end == ends[forms[0]], "the forms do not end in the same state"
                if f == "on":
                    t_sum.append(ts)
                    agg_on = agg
        row = {"lock_steps": steps}
        for f in forms:
            row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "runs": [round(v, 5) for v in runs[f]]}
        if len(forms) == 2:
            row["on_over_off"] = row["on"]["median_ms_per_lock_step"] / row["off"]["median_ms_per_lock_step"]
            row["on_minus_off_us_per_lock_step"] = 1e3 * (row["on"]["median_ms_per_lock_step"] - row["off"]["median_ms_per_lock_step"])
            row["summary_call_ms"] = {"median": float(np.median(t_sum)) * 1e3, "runs": [round(v * 1e3, 4) for v in t_sum]}
            camp = [host_campaign(n_epi) for _ in range(args.campaign_repeats)]
            row["campaign_s"] = {
                "new_keep_paths_false_plus_aggregate_metrics": float(np.median(walls["on"])),
                "keep_paths_false_run_alone": float(np.median(walls["off"])),
                "host_run_with_paths_plus_numpy_restatement": float(np.median([c[0] for c in camp])),
                "host_run_with_paths_alone": float(np.median([c[1] for c in camp]))}
            # the two paths give the same numbers
            for a, b in zip(agg_on, camp[0][2]):
                for k in ("ade", "fde", "planning_ade", "planning_fde", "mean_jerk", "rms_jerk", "mean_accel"):
                    assert abs(a[k] - b[k]) <= 1e-10 * abs(b[k]), (k, a[k], b[k])
                for k in ("min_dist", "min_ttc", "max_jerk", "max_accel", "ade_eval_count", "planning_eval_count", "collision_count"):
                    assert a[k] == b[k], (k, a[k], b[k])
            row["campaign_summaries_agree"] = True
        if args.parent_tree and not args.only:
            sides = {"parent": os.path.abspath(args.parent_tree), "this": ROOT}
            got = {k: [] for k in sides}
            for _ in range(args.repeats):                         # parent, this, parent, this ...: one child process each
                for k, tree in sides.items():
                    p = subprocess.run([sys.executable, "-c", CHILD, tree, fixture, str(n_epi), "1"], check=True,
                                       capture_output=True, text=True, timeout=600)
                    got[k] += json.loads(p.stdout.strip().splitlines()[-1])
            row["off_against_parent"] = {
                k: {"median_ms_per_lock_step": float(np.median(v)), "runs": [round(x, 5) for x in v]} for k, v in got.items()}
            pm, tm = np.median(got["parent"]), np.median(got["this"])
            row["off_against_parent"]["this_minus_parent_ms"] = float(tm - pm)
            row["off_against_parent"]["parent_spread_ms"] = float(max(got["parent"]) - min(got["parent"]))
        result["episodes"][str(n_epi)] = row
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
