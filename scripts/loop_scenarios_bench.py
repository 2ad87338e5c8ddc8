#!/usr/bin/env python3
"""What mixing scenarios in one lock step buys: 64 reference episodes split over scenario_01 / scenario_02 / scenario_03
(22 / 21 / 21 copies of the base, walls and turn recordings) as (M) ONE mixed loop on one handle against (S) three
single-scenario loops run one after the other, each form stepwise (one library call per lock step) and resident (whole
runs inside the library).  Whole runs; ms per lock step = wall time until all 64 episodes have ended / lock steps of the
longest episode (what the mixed loop executes).  Order M S M S ... behind one warm-up of each, median of --repeats.
--forms S runs on a tree that predates the mixed loop (the comparison's other side).

    python3 scripts/loop_scenarios_bench.py --out profiles/r07_loop_scenarios.json [--repeats 5] [--forms M S]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPLIT = (("base", 22), ("walls", 21), ("turn", 21))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forms", nargs="+", choices=["M", "S"], default=["M", "S"])
    ap.add_argument("--only", choices=["step", "resident"], default=None, help="one way of stepping alone (for a kernel trace)")
    args = ap.parse_args()
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    variants = json.loads(str(z["meta"]))["variants"]
    cfg = {n: dict(variants[n]["config"]) for n, _ in SPLIT}

    def one_run(form, resident):
        kw = dict(resident=True) if resident else {}
        steps, wall = [], 0.0
        if form == "M":
            names = [n for k in range(22) for n, cnt in SPLIT if k < cnt]         # interleaved
            loops = [([cfg[n] for n in names], [z[n + "_ped_traj"] for n in names])]
        else:
            loops = [(cfg[n], [z[n + "_ped_traj"]] * cnt) for n, cnt in SPLIT]
        for c, tracks in loops:
            with BatchedClosedLoop(c, tracks, **kw) as loop:
                t0 = time.perf_counter()
                loop.run()
                wall += time.perf_counter() - t0
                steps += [int(v) for v in loop.step_counts]
        return wall * 1e3, steps

    ways = [args.only] if args.only else ["step", "resident"]
    result = {"what": "64 episodes over scenario_01/02/03 (22/21/21): M one mixed loop, S three single-scenario loops in "
                      "sequence; ms per lock step = wall of all runs / lock steps of the longest episode",
              "repeats": args.repeats, "order": "warm-up of every form, then " + " ".join(args.forms) + " repeated"}
    for way in ways:
        res = way == "resident"
        ref_steps = None
        for f in args.forms:
            ref_steps = sorted(one_run(f, res)[1])                   # warm-up
        runs = {f: [] for f in args.forms}
        for _ in range(args.repeats):
            for f in args.forms:
                ms, steps = one_run(f, res)
                assert sorted(steps) == ref_steps, "the forms do not run the same episodes"
                runs[f].append(ms / max(steps))
        row = {"lock_steps": max(ref_steps), "episode_steps": sum(ref_steps)}
        for f in args.forms:
            row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "runs": [round(v, 5) for v in runs[f]]}
        if "M" in row and "S" in row:
            row["M_over_S"] = row["M"]["median_ms_per_lock_step"] / row["S"]["median_ms_per_lock_step"]
        result[way] = row
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
