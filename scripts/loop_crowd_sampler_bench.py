#!/usr/bin/env python3
"""Time per lock step of a sweep predicted by the in-library Social-GAN sampler: 64 slots = 8 crowds of 30 pedestrians x 8
conditions at S = 20 samples, resident, the (16, 32, 32, 64, 8, 8) model with seeded weights (pooling once per scene) --
the workload of scripts/loop_sweep_bench.py with the sampler in place of the scripted recording.

  a  the sweep loop with the slot-keyed sampler (fot_loop_set_sampler): every slot a scene of its own, 64 scenes x 1920 rows
     through window, noise, encoder, pool net and S decoders every lock step
  b  the shared sampler (fot_loop_set_sampler_shared, slot_crowd[e] = e // 8): 8 scenes x 240 rows, then one gather into the
     step's raw tensor of the 64 episodes
  c  RecordedSamples(slot_col0=...) over b's samples (the slot-keyed sampler recorded over the 8 crowds, crowd c at slot c):
     b without the generator

Order a b c a b c ... in ONE process behind a warm-up run of each form, median of --repeats, every run kept.  b and c plan
against the same samples and must end in the same state; a draws other noise for every condition and ends elsewhere.  The
warm-up runs also record what the first lock step handed to the generator (fot_debug_loop_sampler_shape).

    python3 scripts/loop_crowd_sampler_bench.py --out profiles/r23_crowd_sampler.json [--repeats 5] [--steps 120]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 scripts/loop_crowd_sampler_bench.py --only b --repeats 1   (a run of its own)
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
# (distribution_aware_planning, chance_epsilon, collision_margin_inflation): scripts/loop_sweep_bench.py's
CONDITIONS = [(False, 0.0, 1.0 + 0.1 * i) for i in range(6)] + [(True, 0.0, 1.0), (True, 0.05, 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None, help="one form alone, for a profiler run (no comparisons)")
    args = ap.parse_args()
    import bench
    import sgan_common as sc
    from integrated_path_planning_amd import synthetic as syn
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    from integrated_path_planning_amd.planner import BatchPlanner
    from integrated_path_planning_amd.prediction import RecordedSamples, SganSampler, SganWeights, record_samples
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    base = dict(json.loads(str(z["meta"]))["config"])
    tr = z["base_ped_traj"]
    track = np.concatenate([tr, tr + np.array([0.7, 9.0]), tr[:, :2] + np.array([-0.5, -9.0])], axis=1)
    assert track.shape[1] == P
    crowds = [track + np.array([0.15 * c, 0.1 * (c % 3)]) for c in range(CROWDS)]     # eight crowds, each a little elsewhere
    K = len(CONDITIONS)
    cfgs = [dict(base, distribution_aware_planning=a, chance_epsilon=e, collision_margin_inflation=m) for a, e, m in CONDITIONS]
    aware = dict(base, distribution_aware_planning=True)
    # slot = crowd * K + condition
    slot_cfg = [cfgs[k] for _ in range(CROWDS) for k in range(K)]
    slot_tracks = [crowds[c] for c in range(CROWDS) for _ in range(K)]
    slot_crowd = [c for c in range(CROWDS) for _ in range(K)]
    col0 = [P * c for c in slot_crowd]
    a_model = dict(obs_len=base["obs_len"], pred_len=base["pred_len"], num_layers=1, pooling_type="pool_net", pool_every_timestep=False,
                   noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
    w = SganWeights.from_state_dict(a_model, sc.seeded_state(a_model, 11, 3.0))
    forms = ("a", "b", "c") if args.only is None else (args.only,)
    shared = None
    if "c" in forms:
        with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
            shared = record_samples(aware, crowds, SganSampler(bp, w, S, counter_seed=SEED), args.steps, dtype=np.float32,
                                    device="cuda").samples.clone()    # [steps, S, pred_len, 240, 2]: crowd c drawn as slot c

    def source(form):
        if form == "c":
            return RecordedSamples(shared, slot_col0=col0)
        return SganSampler(None, w, S, counter_seed=SEED, slot_crowd=slot_crowd if form == "b" else None)

    def one_run(form, shape=False):
        """(ms per lock step, lock steps, end state, the first step's sampler shape where asked for)"""
        loop = BatchedClosedLoop(slot_cfg, slot_tracks, sample_source=source(form), plan_on_representative_sample=True,
                                 device_samples=True, resident=True)
        with loop:
            assert loop._sweep
            first = None
            if shape:
                loop.run(1)
                first = list(loop.engine.debug_loop_sampler_shape()) if form != "c" else None
            t0 = time.perf_counter()
            loop.run(args.steps - (1 if shape else 0))                # (every lock step ends with the host waiting for the device)
            wall = time.perf_counter() - t0
            steps = len(loop._steps)
            return wall / (steps - (1 if shape else 0)) * 1e3, steps, (loop.step_counts.tobytes(), loop.termination.tobytes(),
                                                                      loop.ego.tobytes()), first

    result = {"what": "ms per lock step of 64 slots = 8 crowds x 30 pedestrians x 8 conditions, S = 20, resident sweep loop; a = the "
                      "slot-keyed sampler (fot_loop_set_sampler); b = the shared sampler (fot_loop_set_sampler_shared, one sampling "
                      "per crowd); c = RecordedSamples(slot_col0) over b's samples (no generator)",
              "pedestrians": P, "samples": S, "crowds": CROWDS, "conditions": [list(c) for c in CONDITIONS], "max_steps": args.steps,
              "dims": {k: (list(v) if isinstance(v, tuple) else v) for k, v in DIMS.items()}, "pooling": "pool_net, once per scene",
              "repeats": args.repeats, "order": "warm-up of every form, then a b c repeated",
              "kernel_source_hash": bench.kernel_source_hash()}
    ends = {f: one_run(f, shape=True) for f in forms}                 # warm-up: code objects, workspace, fresh memory
    result["sampler_shape_first_step"] = {f: ends[f][3] for f in forms if f != "c"}
    if args.only is None:
        assert ends["b"][2] == ends["c"][2], "the shared sampler and the recording of its samples do not end in the same state"
        result["a_ends_where_b_ends"] = bool(ends["a"][2] == ends["b"][2])
    runs = {f: [] for f in forms}
    for _ in range(args.repeats):
        for f in forms:
            ms, steps, end, _ = one_run(f)
            runs[f].append(ms)
            assert end == ends[f][2], "a form does not repeat its end state"
    for f in forms:
        result[f] = {"lock_steps": ends[f][1], "median_ms_per_lock_step": float(np.median(runs[f])), "min": float(min(runs[f])),
                     "max": float(max(runs[f])), "runs": [round(v, 5) for v in runs[f]]}
    if args.only is None:
        med = {f: result[f]["median_ms_per_lock_step"] for f in forms}
        result["b_over_a"] = med["b"] / med["a"]
        result["b_over_c"] = med["b"] / med["c"]
        result["b_below_a_in_every_repetition"] = bool(all(b < a for a, b in zip(runs["a"], runs["b"])))
        result["b_at_or_above_c_in_every_repetition"] = bool(all(b >= c for b, c in zip(runs["b"], runs["c"])))
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
