#!/usr/bin/env python3
"""Time per lock step of Social-GAN-predicted episodes that plan on the REPRESENTATIVE sample (the reference's default:
distribution_aware_planning unset, num_samples = 20), and of the routes beside it:

  rep_resident    the whole run inside the library, the samples never leaving HBM (resident=True, device_samples=True,
                  plan_on_representative_sample=True)
  rep_step        the one-call step in the same mode (fot_loop_step per lock step)
  host_five_call  the five-call step with the host hand-over: the samples come back to the host, NumPy picks the sample,
                  the chosen tracks go up again -- the only route this configuration had before the mode existed
  dist_resident   for orientation: the distribution-aware resident loop (plans against all 20 samples) at the same sizes

64 and 256 episodes x 30 pedestrians x S = 20 samples, the (16, 32, 32, 64, 8, 8) model with seeded weights and pooling
once per scene, runs of --steps lock steps on scenario_01.  All forms draw the same counter-based noise.  One process per
tree; per size a warm-up run of each form, then the forms alternated --repeats times; the median is reported.  --tree names
the checkout whose package is measured (default: this one); a tree that lacks the mode runs host_five_call and
dist_resident only.  The wall clock around run() ends behind the last step's results in host memory.

    python3 scripts/rep_sample_bench.py --out profiles/r17_rep_sample.json --label this [--tree DIR] [--repeats 5]
                                        [--episodes 64 256] [--steps 30]

With --out, the runs are merged into the file under runs[label] (the file keeps the runs of other labels).
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

P, S, SEED = 30, 20, 2024
DIMS = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=8, noise_dim=(8,))
FORMS = ("rep_resident", "rep_step", "host_five_call", "dist_resident")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--commit", default=None, help="what to record as the tree's commit")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    root = os.path.abspath(args.tree)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import sgan_common as sc
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    from integrated_path_planning_amd.prediction import SganSampler, SganWeights
    has_mode = "plan_on_representative_sample" in inspect.signature(BatchedClosedLoop.__init__).parameters
    forms = [f for f in FORMS if has_mode or not f.startswith("rep_")]
    z = np.load(os.path.join(root, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    base = dict(json.loads(str(z["meta"]))["config"], num_samples=S)
    tr = z["base_ped_traj"]
    track = np.concatenate([tr, tr + np.array([0.7, 9.0]), tr[:, :2] + np.array([-0.5, -9.0])], axis=1)
    assert track.shape[1] == P
    a = dict(obs_len=base["obs_len"], pred_len=base["pred_len"], num_layers=1, pooling_type="pool_net", pool_every_timestep=False,
             noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
    w = SganWeights.from_state_dict(a, sc.seeded_state(a, 11, 3.0))

    def one_run(n_epi, form):
        aware = form == "dist_resident"
        cfg = dict(base, distribution_aware_planning=aware)
        kw = {}
        if form != "host_five_call":
            kw["device_samples"] = True
        if form.endswith("resident"):
            kw["resident"] = True
        if form.startswith("rep_"):
            kw["plan_on_representative_sample"] = True
        src = SganSampler(None, w, S, counter_seed=SEED)
        with BatchedClosedLoop(cfg, [track] * n_epi, sample_source=src, **kw) as loop:
            t0 = time.perf_counter()
            loop.run(args.steps)
            wall = time.perf_counter() - t0
            steps = len(loop._steps)
            end = (loop.step_counts.tobytes(), loop.termination.tobytes(), loop.ego.tobytes())
        return wall / steps * 1e3, steps, end

    result = {}
    for n_epi in args.episodes:
        ends = {f: one_run(n_epi, f)[2] for f in forms}              # warm-up: code objects, workspace, fresh memory
        same = [f for f in forms if f != "dist_resident"]            # the three routes of ONE configuration plan the same steps
        agree = all(ends[f] == ends[same[0]] for f in same)
        runs, steps = {f: [] for f in forms}, 0
        for _ in range(args.repeats):
            for f in forms:
                ms, steps, end = one_run(n_epi, f)
                runs[f].append(ms)
                assert end == ends[f], f"{f}: a repeat ended in another state"
        row = {"lock_steps": steps, "routes_end_in_the_same_state": bool(agree)}
        for f in forms:
            row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "runs": [round(v, 5) for v in runs[f]]}
        if has_mode:
            for f in ("rep_resident", "rep_step"):
                row[f + "_over_host_five_call"] = row[f]["median_ms_per_lock_step"] / row["host_five_call"]["median_ms_per_lock_step"]
            row["rep_resident_minus_dist_resident_ms"] = (row["rep_resident"]["median_ms_per_lock_step"]
                                                          - row["dist_resident"]["median_ms_per_lock_step"])
        result[str(n_epi)] = row
        print(args.label, n_epi, json.dumps(row), flush=True)
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc.setdefault("what", "ms per lock step, Social-GAN-predicted episodes planning on the representative sample "
                               "(rep_resident, rep_step: fot_loop_plan_sample) beside the five-call step with the host "
                               "hand-over (host_five_call) and the distribution-aware resident loop (dist_resident)")
        doc.update(pedestrians=P, samples=S, lock_steps_per_run=args.steps, repeats=args.repeats,
                   dims={k: (list(v) if isinstance(v, tuple) else v) for k, v in DIMS.items()},
                   order="one process per tree; per size a warm-up run of each form, then the forms alternated; medians")
        doc.setdefault("runs", {})[args.label] = {"commit": args.commit, "forms": list(forms), "sizes": result}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
