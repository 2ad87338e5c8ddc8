#!/usr/bin/env python3
"""Time per lock step of distribution-aware episodes that predict from a recorded sample tensor: (A) the stepwise loop --
one fot_loop_step per lock step, the step's row of the recording handed over as a device pointer
(``device_samples=True``), the only route without fot_loop_set_samples -- against (B) the whole run inside the library
(``resident=True`` on the same ``prediction.RecordedSamples``).  Beside them (C) the resident loop with the library's own
sampler (fot_loop_set_sampler), which runs the network every step.  The recording is made once per size by that same
counter-seeded sampler through ``record_samples`` (float32, device memory), so all three plan the same steps; A and B
must end in the same state.

64 and 256 episodes x 30 pedestrians x S = 20 samples, pred_len 12, the (16, 32, 32, 64, 8, 8) model of
scripts/sgan_loop_bench.py with pooling once per scene, runs of up to 274 lock steps on scenario_01.  Order A B C A B C
... in ONE process behind a warm-up run of each form, median of --repeats, every run kept.

    python3 scripts/recorded_loop_bench.py --out profiles/r18_recorded_samples.json [--repeats 5] [--episodes 64 256]
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
    args = ap.parse_args()
    import sgan_common as sc
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    from integrated_path_planning_amd.prediction import RecordedSamples, SganSampler, SganWeights, record_samples
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    cfg = dict(json.loads(str(z["meta"]))["config"], distribution_aware_planning=True)
    tr = z["base_ped_traj"]
    track = np.concatenate([tr, tr + np.array([0.7, 9.0]), tr[:, :2] + np.array([-0.5, -9.0])], axis=1)
    assert track.shape[1] == P
    a = dict(obs_len=cfg["obs_len"], pred_len=cfg["pred_len"], num_layers=1, pooling_type="pool_net", pool_every_timestep=False,
             noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
    w = SganWeights.from_state_dict(a, sc.seeded_state(a, 11, 3.0))

    def one_run(n_epi, form, samples):
        if form == "C":
            src, kw = SganSampler(None, w, S, counter_seed=SEED), dict(resident=True)
        else:
            src, kw = RecordedSamples(samples), (dict(resident=True) if form == "B" else {})
        with BatchedClosedLoop(cfg, [track] * n_epi, sample_source=src, device_samples=True, **kw) as loop:
            t0 = time.perf_counter()
            loop.run(args.steps)
            wall = time.perf_counter() - t0
            steps = len(loop._steps)
            end = (loop.step_counts.tobytes(), loop.termination.tobytes(), loop.ego.tobytes())
        return wall / steps * 1e3, steps, end

    result = {"what": "ms per lock step, distribution-aware episodes predicting from a recorded sample tensor; A = stepwise "
                      "device_samples loop on the recording, B = resident loop on the same recording (fot_loop_set_samples), "
                      "C = resident loop with the library's own sampler (fot_loop_set_sampler)",
              "pedestrians": P, "samples": S, "max_steps": args.steps, "recording": "float32, device memory, record_samples of "
              "the counter-seeded SganSampler", "dims": {k: (list(v) if isinstance(v, tuple) else v) for k, v in DIMS.items()},
              "repeats": args.repeats, "order": "warm-up of every form, then A B C repeated", "runs": {}}
    for n_epi in args.episodes:
        tracks = [track] * n_epi
        smp = SganSampler(None, w, S, counter_seed=SEED)
        t0 = time.perf_counter()
        with BatchedClosedLoop(cfg, tracks, sample_source=smp, device_samples=True):          # (binds the sampler to an engine)
            rec = record_samples(cfg, tracks, smp, args.steps, dtype=np.float32, device="cuda")
        t_rec = time.perf_counter() - t0
        samples = rec.samples
        forms = ("A", "B", "C")
        ends = {f: one_run(n_epi, f, samples)[2] for f in forms}      # warm-up: code objects, workspace, fresh memory
        assert ends["A"] == ends["B"], "the stepwise and the resident loop on the recording do not end in the same state"
        runs, steps = {f: [] for f in forms}, 0
        for _ in range(args.repeats):
            for f in forms:
                ms, steps, end = one_run(n_epi, f, samples)
                runs[f].append(ms)
                assert f == "C" or end == ends["A"], "the forms do not end in the same state"
        row = {"lock_steps": steps, "recording_bytes": int(samples.numel() * samples.element_size()),
               "recording_seconds": round(t_rec, 3), "sampler_loop_ends_in_the_same_state": ends["C"] == ends["A"]}
        for f in forms:
            row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "min": float(min(runs[f])), "max": float(max(runs[f])),
                      "runs": [round(v, 5) for v in runs[f]]}
        row["B_over_A"] = row["B"]["median_ms_per_lock_step"] / row["A"]["median_ms_per_lock_step"]
        row["B_median_below_A_min"] = bool(row["B"]["median_ms_per_lock_step"] < row["A"]["min"])
        row["B_median_below_C_median"] = bool(row["B"]["median_ms_per_lock_step"] < row["C"]["median_ms_per_lock_step"])
        result["runs"][f"recorded_{n_epi}"] = row
        print(f"recorded_{n_epi}", json.dumps(row), flush=True)
        del samples, rec
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
