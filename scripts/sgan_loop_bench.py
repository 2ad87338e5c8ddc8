#!/usr/bin/env python3
"""Time per lock step of Social-GAN-predicted, distribution-aware episodes: (A) the stepwise loop -- one fot_loop_step per
lock step, the window stacked and uploaded by Python, fot_sgan_noise and fot_sgan_sample as calls of their own
(``device_samples=True``) -- against (B) the whole run inside the library (``resident=True`` with the same sampler:
fot_loop_set_sampler).  Both draw the same counter-based noise, so they plan the same steps; B is only ever compared with
the A measured beside it.

64 and 256 episodes x 30 pedestrians x S = 20 samples, the (16, 32, 32, 64, 8, 8) model of scripts/sgan_bench.py with
seeded weights, pooling once per scene and no pooling, runs of up to 274 lock steps on scenario_01 (the base recording's
14 pedestrians, a shifted copy of them and two more).  Order A B A B ... in ONE process behind a warm-up run of each
form, median of --repeats; then one more run of each form with fot_profile_* on for the plan kernels' device time.

    python3 scripts/sgan_loop_bench.py --out profiles/r12_sgan_loop.json [--repeats 5] [--episodes 64 256] [--steps 274]
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
P, S, SEED = 30, 20, 2024
DIMS = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=8, noise_dim=(8,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=274)
    ap.add_argument("--models", nargs="+", default=["pool_once", "none"], choices=["pool_once", "none"])
    args = ap.parse_args()
    import sgan_common as sc
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    from integrated_path_planning_amd.prediction import SganSampler, SganWeights
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    cfg = dict(json.loads(str(z["meta"]))["config"], distribution_aware_planning=True)
    tr = z["base_ped_traj"]
    track = np.concatenate([tr, tr + np.array([0.7, 9.0]), tr[:, :2] + np.array([-0.5, -9.0])], axis=1)
    assert track.shape[1] == P

    def weights(model):
        a = dict(obs_len=cfg["obs_len"], pred_len=cfg["pred_len"], num_layers=1, pooling_type="pool_net" if model == "pool_once" else None,
                 pool_every_timestep=False, noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
        return SganWeights.from_state_dict(a, sc.seeded_state(a, 11, 3.0))

    def one_run(n_epi, w, form, profile=False):
        kw = dict(resident=True) if form == "B" else {}
        src = SganSampler(None, w, S, counter_seed=SEED)
        with BatchedClosedLoop(cfg, [track] * n_epi, sample_source=src, device_samples=True, **kw) as loop:
            if profile:
                loop.engine.profile(True)
            t0 = time.perf_counter()
            loop.run(args.steps)
            wall = time.perf_counter() - t0
            steps = len(loop._steps)
            split = loop.engine.profile_read() if profile else None
            end = (loop.step_counts.tobytes(), loop.termination.tobytes(), loop.ego.tobytes())
        return wall / steps * 1e3, steps, end, split

    result = {"what": "ms per lock step, Social-GAN-predicted distribution-aware episodes; A = stepwise device_samples loop, "
                      "B = resident loop with the same sampler", "pedestrians": P, "samples": S, "max_steps": args.steps,
              "dims": {k: (list(v) if isinstance(v, tuple) else v) for k, v in DIMS.items()}, "repeats": args.repeats,
              "order": "warm-up of both forms, then A B repeated, then one profiled run of each", "runs": {}}
    for model in args.models:
        w = weights(model)
        for n_epi in args.episodes:
            ends = {f: one_run(n_epi, w, f)[2] for f in ("A", "B")}             # warm-up: code objects, workspace, fresh memory
            assert ends["A"] == ends["B"], "the forms do not end in the same state"
            runs, steps = {"A": [], "B": []}, 0
            for _ in range(args.repeats):
                for f in ("A", "B"):
                    ms, steps, end, _ = one_run(n_epi, w, f)
                    runs[f].append(ms)
                    assert end == ends["A"], "the forms do not end in the same state"
            row = {"lock_steps": steps}
            for f in ("A", "B"):
                row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "runs": [round(v, 5) for v in runs[f]],
                          "plan_kernels": one_run(n_epi, w, f, profile=True)[3]}
            row["B_over_A"] = row["B"]["median_ms_per_lock_step"] / row["A"]["median_ms_per_lock_step"]
            result["runs"][f"{model}_{n_epi}"] = row
            print(f"{model}_{n_epi}", json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
