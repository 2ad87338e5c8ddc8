#!/usr/bin/env python3
"""Time per lock step of the closed loop of row f4: (A) one library call per lock step (BatchedClosedLoop's default,
fot_loop_step) against (B) the whole run inside the library (resident=True: fot_loop_set_replay / fot_loop_run), with
and without the followed paths brought back.  The configuration of bench.py's latency.f4_closed_loop[_256]: scenario_01,
the base recording, 64 and 256 copies advanced together, whole runs.  Order A B A B ... in ONE process behind a warm-up
run of each form, median of --repeats runs each; B is only ever compared with the A measured beside it.

    python3 scripts/loop_run_bench.py --out profiles/r06_loop_run.json [--repeats 5] [--episodes 64 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--only", choices=["A", "B", "B_nopaths"], default=None, help="one form alone (for a kernel trace)")
    args = ap.parse_args()
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    cfg = json.loads(str(z["meta"]))["config"]

    def one_run(n_epi, form):
        kw = {} if form == "A" else dict(resident=True)
        with BatchedClosedLoop(cfg, [z["base_ped_traj"]] * n_epi, **kw) as loop:
            t0 = time.perf_counter()
            hists = loop.run(**({"keep_paths": False} if form == "B_nopaths" else {}))
            wall = time.perf_counter() - t0
            steps = len(hists[0])
            end = (loop.episodes[0].termination_reason, loop.ego[0].tobytes())
        return wall / steps * 1e3, steps, end

    forms = [args.only] if args.only else ["A", "B", "B_nopaths"]
    result = {"what": "ms per lock step, whole runs of scenario_01's base episode", "repeats": args.repeats,
              "order": "warm-up of every form, then " + " ".join(forms) + " repeated", "episodes": {}}
    for n_epi in args.episodes:
        ends = {}
        for f in forms:                                           # warm-up: code objects, workspace, fresh memory
            ends[f] = one_run(n_epi, f)[2]
        runs = {f: [] for f in forms}
        steps = 0
        for _ in range(args.repeats):
            for f in forms:
                ms, steps, end = one_run(n_epi, f)
                runs[f].append(ms)
                assert end == ends[forms[0]], "the forms do not end in the same state"
        row = {"lock_steps": steps}
        for f in forms:
            row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "runs": [round(v, 5) for v in runs[f]]}
        if "A" in row and "B" in row:
            row["B_over_A"] = row["B"]["median_ms_per_lock_step"] / row["A"]["median_ms_per_lock_step"]
            row["B_nopaths_over_A"] = row["B_nopaths"]["median_ms_per_lock_step"] / row["A"]["median_ms_per_lock_step"]
        result["episodes"][str(n_epi)] = row
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
