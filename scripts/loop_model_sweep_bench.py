#!/usr/bin/env python3
"""Time per lock step of a campaign cell whose conditions use TWO Social-GAN models: 64 slots = 8 crowds of 30 pedestrians x
the eight conditions of the reference's margin-control experiment (examples/run_da_poc.py CONDITIONS: six on the pooled
'sgan' model, two on the no-pooling 'lstm' one), S = 20 samples, resident, dimension set (16, 32, 32, 64, 8, 8) with seeded
weights, pool_every_timestep = False -- the workload of scripts/loop_crowd_sampler_bench.py with the predictor as a per-slot
axis.

  a  ONE sweep loop of 64 slots, a model per slot (fot_loop_set_sampler_models): every lock step samples 8 scenes x 240 rows
     on each model -- the second model on a side stream -- and gathers them with one k_loop_model_rows launch
  o  (--one-stream) a with FOT_LOOP_MODEL_STREAMS=0: both models one after the other on the loop's stream
  b  what the library offered before for the same episodes: a 48-slot and a 16-slot crowd-shared sweep loop
     (fot_loop_set_sampler_shared), each on a handle with one model, run one after the other; its figure is the SUM of the two
     loops' time per lock step

Order a b [o] a b [o] ... in ONE process behind a warm-up run of each form, median of --repeats whole runs, every run kept.  Every
slot of a must end where its slot of b ends (the same model, crowd id, seed and condition).

    python3 scripts/loop_model_sweep_bench.py --out profiles/r24_model_sweep.json [--repeats 5] [--steps 120]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
P, S, CROWDS, SEED = 30, 20, 8, 2024
DIMS = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=8, noise_dim=(8,))
# (method, distribution_aware_planning, chance_epsilon, collision_margin_inflation): examples/run_da_poc.py CONDITIONS
CONDITIONS = [("sgan", False, 0.0, 1.00), ("sgan", False, 0.0, 1.10), ("sgan", False, 0.0, 1.20), ("sgan", False, 0.0, 1.35),
              ("sgan", False, 0.0, 1.50), ("sgan", True, 0.0, 1.00), ("lstm", False, 0.0, 1.00), ("lstm", True, 0.0, 1.00)]
METHODS = ("sgan", "lstm")                        # model 0: pool net, once per scene; model 1: no pooling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--only", choices=["a", "b"], default=None, help="one form alone, for a profiler run (no comparisons)")
    ap.add_argument("--one-stream", action="store_true", help="a third form o = a with FOT_LOOP_MODEL_STREAMS=0, order a b o")
    args = ap.parse_args()
    import bench
    import sgan_common as sc
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    from integrated_path_planning_amd.prediction import SganSampler, SganWeights
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    base = dict(json.loads(str(z["meta"]))["config"])
    tr = z["base_ped_traj"]
    track = np.concatenate([tr, tr + np.array([0.7, 9.0]), tr[:, :2] + np.array([-0.5, -9.0])], axis=1)
    assert track.shape[1] == P
    crowds = [track + np.array([0.15 * c, 0.1 * (c % 3)]) for c in range(CROWDS)]     # eight crowds, each a little elsewhere
    K = len(CONDITIONS)
    cfgs = [dict(base, distribution_aware_planning=a, chance_epsilon=e, collision_margin_inflation=m) for _, a, e, m in CONDITIONS]
    # slot = crowd * K + condition
    slot_cond = [k for _ in range(CROWDS) for k in range(K)]
    slot_crowd = [c for c in range(CROWDS) for _ in range(K)]
    slot_model = [METHODS.index(CONDITIONS[k][0]) for k in slot_cond]
    weights = []
    for pooling, seed in (("pool_net", 11), (None, 12)):
        a = dict(obs_len=base["obs_len"], pred_len=base["pred_len"], num_layers=1, pooling_type=pooling, pool_every_timestep=False,
                 noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
        weights.append(SganWeights.from_state_dict(a, sc.seeded_state(a, seed, 3.0)))
    forms = (("a", "b", "o") if args.one_stream else ("a", "b")) if args.only is None else (args.only,)

    def run_loop(slots, source, shapes):
        """(seconds, lock steps, per-slot end state, the first step's sampler shapes where asked for) of the loop over `slots`"""
        loop = BatchedClosedLoop([cfgs[slot_cond[e]] for e in slots], [crowds[slot_crowd[e]] for e in slots], sample_source=source,
                                 plan_on_representative_sample=True, device_samples=True, resident=True)
        with loop:
            assert loop._sweep
            first = None
            if shapes:
                loop.run(1)
                first = [list(v) for v in loop.engine.debug_loop_sampler_shapes(2)]
            t0 = time.perf_counter()
            loop.run(args.steps - (1 if shapes else 0))               # (every lock step ends with the host waiting for the device)
            wall = time.perf_counter() - t0
            steps = len(loop._steps) - (1 if shapes else 0)
            end = {e: (int(loop.step_counts[i]), int(loop.termination[i]), loop.ego[i].tobytes()) for i, e in enumerate(slots)}
            return wall, steps, end, first

    def one_run(form, shapes=False):
        """(ms per lock step, lock steps, per-slot end state, sampler shapes)"""
        every = list(range(CROWDS * K))
        if form in ("a", "o"):
            src = SganSampler(None, weights, S, counter_seed=SEED, slot_crowd=slot_crowd, slot_model=slot_model)
            os.environ["FOT_LOOP_MODEL_STREAMS"] = "0" if form == "o" else "1"     # (read by the set call)
            wall, steps, end, first = run_loop(every, src, shapes)
            del os.environ["FOT_LOOP_MODEL_STREAMS"]
            return wall / steps * 1e3, steps, end, first, wall * 1e3
        ms, end, first, steps, total = 0.0, {}, [], [], 0.0
        for m in (0, 1):                                              # one loop per model, one after the other
            slots = [e for e in every if slot_model[e] == m]
            src = SganSampler(None, weights[m], S, counter_seed=SEED, slot_crowd=[slot_crowd[e] for e in slots])
            wall, n, end_m, first_m = run_loop(slots, src, shapes)
            ms += wall / n * 1e3
            total += wall * 1e3
            end.update(end_m)
            steps.append(n)
            first.append(first_m[0] if first_m else None)
        return ms, steps, end, first, total

    result = {"what": "ms per lock step of 64 slots = 8 crowds x 30 pedestrians x the 8 conditions of run_da_poc.py (6 on a pooled "
                      "model, 2 on a no-pooling one), S = 20, resident sweep loops; a = ONE loop, a model per slot "
                      "(fot_loop_set_sampler_models); b = a 48-slot and a 16-slot crowd-shared loop (fot_loop_set_sampler_shared) run "
                      "one after the other, the sum of their times per lock step; o = a with every model on the loop's stream "
                      "(FOT_LOOP_MODEL_STREAMS=0)",
              "pedestrians": P, "samples": S, "crowds": CROWDS, "conditions": [list(c) for c in CONDITIONS], "max_steps": args.steps,
              "dims": {k: (list(v) if isinstance(v, tuple) else v) for k, v in DIMS.items()},
              "models": ["pool_net, once per scene", "no pooling"], "repeats": args.repeats,
              "order": "warm-up of every form, then a b repeated", "kernel_source_hash": bench.kernel_source_hash()}
    ends = {f: one_run(f, shapes=True) for f in forms}                # warm-up: code objects, workspace, fresh memory
    result["sampler_shapes_first_step"] = {f: ends[f][3] for f in forms}
    if args.only is None:
        assert ends["a"][2] == ends["b"][2], "a slot of the one loop does not end where its single-model loop ends"
        assert not args.one_stream or ends["o"][2] == ends["a"][2], "the side stream changes the numbers"
    runs, totals = {f: [] for f in forms}, {f: [] for f in forms}
    for _ in range(args.repeats):
        for f in forms:
            ms, steps, end, _, total = one_run(f)
            runs[f].append(ms)
            totals[f].append(total)
            assert end == ends[f][2], "a form does not repeat its end state"
    for f in forms:
        result[f] = {"lock_steps": ends[f][1], "median_ms_per_lock_step": float(np.median(runs[f])), "min": float(min(runs[f])),
                     "max": float(max(runs[f])), "runs": [round(v, 5) for v in runs[f]],
                     "median_ms_whole_run": float(np.median(totals[f])), "whole_runs_ms": [round(v, 3) for v in totals[f]]}
    if args.only is None:
        result["a_over_b"] = result["a"]["median_ms_per_lock_step"] / result["b"]["median_ms_per_lock_step"]
        result["a_below_b_in_every_repetition"] = bool(all(a < b for a, b in zip(runs["a"], runs["b"])))
        result["a_whole_run_over_b"] = result["a"]["median_ms_whole_run"] / result["b"]["median_ms_whole_run"]
        if args.one_stream:
            result["a_over_o"] = result["a"]["median_ms_per_lock_step"] / result["o"]["median_ms_per_lock_step"]
            result["a_below_o_in_every_repetition"] = bool(all(a < o for a, o in zip(runs["a"], runs["o"])))
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
