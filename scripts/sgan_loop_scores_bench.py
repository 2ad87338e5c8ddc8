#!/usr/bin/env python3
"""What scoring a resident Social-GAN loop costs (fot_loop_scores_enable), ms per lock step:

(a) the resident sampler loop with the scores OFF against ON, one process, order off on off on ... behind a warm-up run of
    each, median of --repeats; both end in the same state (the mode leaves the step alone);
(b) the OFF path against another build of the library (--parent-lib: the parent commit's libfot.so), in alternating
    processes started before this one touches the GPU, --processes each with --repeats runs; "no regression" is judged
    against the spread of the parent's own repeats;
(c) what the mode replaces: the stepwise loop with prediction_scores=True to the same metrics (run + prediction_metrics()),
    against the resident loop with the scores on (run + prediction_metrics()); the two dictionaries are equal.

64 and 256 episodes x 30 pedestrians x S = 20 samples, the (16, 32, 32, 64, 8, 8) model of scripts/sgan_loop_bench.py with
seeded weights, pooling once per scene, runs of up to 274 lock steps on scenario_01.

    python3 scripts/sgan_loop_scores_bench.py --out profiles/r13_sgan_loop_scores.json [--parent-lib PATH]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
P, S, SEED = 30, 20, 2024
DIMS = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=8, noise_dim=(8,))


class Workload:
    def __init__(self, steps):
        import sgan_common as sc
        from integrated_path_planning_amd.prediction import SganWeights
        z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
        self.cfg = dict(json.loads(str(z["meta"]))["config"], distribution_aware_planning=True)
        tr = z["base_ped_traj"]
        self.track = np.concatenate([tr, tr + np.array([0.7, 9.0]), tr[:, :2] + np.array([-0.5, -9.0])], axis=1)
        assert self.track.shape[1] == P
        a = dict(obs_len=self.cfg["obs_len"], pred_len=self.cfg["pred_len"], num_layers=1, pooling_type="pool_net",
                 pool_every_timestep=False, noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
        self.weights = SganWeights.from_state_dict(a, sc.seeded_state(a, 11, 3.0))
        self.steps = steps

    def run(self, n_epi, form):
        """form: "off" / "on" -- the resident loop without / with the scores; "stepwise" -- prediction_scores=True, stepwise.
        Returns ms per lock step of run(), ms per lock step including prediction_metrics(), the metrics, the end state."""
        from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
        from integrated_path_planning_amd.prediction import SganSampler
        kw = dict(resident=True, prediction_scores=form == "on") if form != "stepwise" else dict(prediction_scores=True)
        src = SganSampler(None, self.weights, S, counter_seed=SEED)
        with BatchedClosedLoop(self.cfg, [self.track] * n_epi, sample_source=src, device_samples=True, **kw) as loop:
            t0 = time.perf_counter()
            if form == "stepwise":
                loop.run(self.steps)
            else:
                loop.run(self.steps, keep_paths=False)
            t1 = time.perf_counter()
            metrics = loop.prediction_metrics() if form != "off" else None
            t2 = time.perf_counter()
            steps = len(loop._steps)
            end = (loop.step_counts.tobytes(), loop.termination.tobytes(), loop.ego.tobytes())
        return (t1 - t0) / steps * 1e3, (t2 - t0) / steps * 1e3, metrics, end, steps


def child(args):
    """(b): the OFF path on the library at --child, nothing else in the process."""
    from integrated_path_planning_amd import _abi
    _abi.LIB_PATH = os.path.abspath(args.child)
    w = Workload(args.steps)
    out = {}
    for n_epi in args.episodes:
        w.run(n_epi, "off")                                          # warm-up: code objects, workspace, fresh memory
        out[str(n_epi)] = [w.run(n_epi, "off")[0] for _ in range(args.repeats)]
    print("CHILD " + json.dumps(out), flush=True)


def same_metrics(a, b):
    def same(x, y):
        return x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))
    return len(a) == len(b) and all(tuple(u) == tuple(v) and all(same(u[k], v[k]) for k in u) for u, v in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=274)
    ap.add_argument("--parent-lib", default=None, help="libfot.so of the parent commit, for (b)")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"what": "ms per lock step of the resident Social-GAN loop: (a) scores off / on, (b) the off path against the "
                      "parent commit's library, (c) the stepwise prediction_scores=True loop it replaces",
              "pedestrians": P, "samples": S, "max_steps": args.steps, "repeats": args.repeats,
              "dims": {k: (list(v) if isinstance(v, tuple) else v) for k, v in DIMS.items()}, "model": "pool_once"}
    # ---- (b) first: fresh processes, started while this one has not touched the GPU
    if args.parent_lib:
        libs = {"parent": os.path.abspath(args.parent_lib), "this": os.path.join(ROOT, "integrated_path_planning_amd", "libfot.so")}
        runs = {k: {str(n): [] for n in args.episodes} for k in libs}
        for _ in range(args.processes):
            for which, path in libs.items():
                cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--repeats", str(args.repeats), "--steps",
                       str(args.steps), "--episodes"] + [str(n) for n in args.episodes]
                out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
                got = json.loads([ln for ln in out.splitlines() if ln.startswith("CHILD ")][-1][6:])
                for n, v in got.items():
                    runs[which][n] += v
        b = {"order": f"{args.processes} processes per library, alternating parent / this, a warm-up and {args.repeats} runs each"}
        for n in args.episodes:
            p, t = runs["parent"][str(n)], runs["this"][str(n)]
            b[str(n)] = {"parent_median": float(np.median(p)), "parent_min": min(p), "parent_max": max(p),
                         "this_median": float(np.median(t)), "this_min": min(t), "this_max": max(t),
                         "this_median_inside_parent_span": bool(min(p) <= np.median(t) <= max(p)),
                         "parent_runs": [round(v, 5) for v in p], "this_runs": [round(v, 5) for v in t]}
            print("(b)", n, json.dumps(b[str(n)]), flush=True)
        result["b_off_path_against_parent"] = b
    else:
        result["b_off_path_against_parent"] = "not measured (--parent-lib not given)"
    # ---- (a) and (c), this process
    w = Workload(args.steps)
    a_out, c_out = {}, {}
    for n_epi in args.episodes:
        ends = {f: w.run(n_epi, f)[3] for f in ("off", "on")}        # warm-up
        assert ends["off"] == ends["on"], "the scores changed the run"
        runs, steps = {"off": [], "on": []}, 0
        for _ in range(args.repeats):
            for f in ("off", "on"):
                ms, _, _, end, steps = w.run(n_epi, f)
                runs[f].append(ms)
                assert end == ends["off"]
        row = {"lock_steps": steps}
        for f in ("off", "on"):
            row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "runs": [round(v, 5) for v in runs[f]]}
        row["on_over_off"] = row["on"]["median_ms_per_lock_step"] / row["off"]["median_ms_per_lock_step"]
        row["on_minus_off_ms"] = row["on"]["median_ms_per_lock_step"] - row["off"]["median_ms_per_lock_step"]
        a_out[str(n_epi)] = row
        print("(a)", n_epi, json.dumps(row), flush=True)
        _, _, want, end, _ = w.run(n_epi, "stepwise")                # warm-up of the stepwise form
        assert end == ends["off"], "the stepwise loop does not end in the same state"
        runs, got = {"stepwise": [], "on": []}, None
        for _ in range(args.repeats):
            for f in ("stepwise", "on"):
                _, ms, m, _, _ = w.run(n_epi, f)
                runs[f].append(ms)
                if f == "on":
                    got = m
        assert same_metrics(got, want), "resident and stepwise metrics differ"
        row = {"lock_steps": steps, "metrics_equal": True, "slot_0": {k: (None if isinstance(v, float) and math.isnan(v) else v)
                                                                   for k, v in got[0].items()}}
        for f in ("stepwise", "on"):
            row[f] = {"median_ms_per_lock_step_with_metrics": float(np.median(runs[f])), "runs": [round(v, 5) for v in runs[f]]}
        row["on_over_stepwise"] = row["on"]["median_ms_per_lock_step_with_metrics"] / row["stepwise"]["median_ms_per_lock_step_with_metrics"]
        c_out[str(n_epi)] = row
        print("(c)", n_epi, json.dumps(row), flush=True)
    result["a_scores_off_against_on"] = a_out
    result["c_stepwise_scores_against_resident_scores"] = c_out
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
