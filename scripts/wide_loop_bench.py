#!/usr/bin/env python3
"""Time per lock step of resident closed loops at sample counts on both sides of 64, on a handle whose sample capacity is
raised (BatchedClosedLoop(sample_capacity=...)): (rec) the resident loop on a recorded sample tensor
(fot_loop_set_samples) and (gan) the resident loop with the library's own Social-GAN sampler (fot_loop_set_sampler), both
distribution-aware, 30 pedestrians per episode, the model of scripts/recorded_loop_bench.py.

S <= 64 runs the kernels of a fresh handle, so its figures are to be held against the same script run on the parent
commit's library on the same box (--capacity 0 builds fresh handles: what the parent can run); S > 64 runs the wide forms
of the score and selection kernels and the plan path's wide evaluation kernels.  Per size: a warm-up run of each form,
then --repeats runs in the order rec gan rec gan ..., median, min, max and every run kept (--forms: one of them only;
--scores: with prediction_scores=True, so that the selection and the score kernels run every step).  --profile adds one run of
each form under fot_profile_enable and stores the per-kernel device time of the kernels the library brackets (the plan
path's: k_cull, the evaluation kernels, ...).  The environment decides FOT_NAN_SCAN (lazy unless "eager"); it is stored.

    python3 scripts/wide_loop_bench.py --out profiles/r34_wide_loop.json --samples 20 64 100 200 [--capacity 254]
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
P, SEED = 30, 2024
DIMS = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=8, noise_dim=(8,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--samples", type=int, nargs="+", default=[20, 64, 100, 200])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--capacity", type=int, default=254, help="0: fresh handles (64)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--forms", nargs="+", default=["rec", "gan"], choices=["rec", "gan"])
    ap.add_argument("--scores", action="store_true", help="prediction_scores=True: the loop also chooses every episode's "
                    "representative sample and scores every step's distribution (the selection and score kernels run)")
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
    cap = args.capacity or None
    src_kw = lambda S: dict(sample_capacity=max(S, 64)) if cap else {}
    loop_kw = dict(sample_capacity=cap) if cap else {}
    run_kw = dict(loop_kw, prediction_scores=True) if args.scores else loop_kw

    def one_run(n_epi, form, S, samples, profile=False):
        src = SganSampler(None, w, S, counter_seed=SEED, **src_kw(S)) if form == "gan" else RecordedSamples(samples, **src_kw(S))
        with BatchedClosedLoop(cfg, [track] * n_epi, sample_source=src, device_samples=True, resident=True, **run_kw) as loop:
            if profile:
                loop.engine.profile(True)
            t0 = time.perf_counter()
            loop.run(args.steps)
            wall = time.perf_counter() - t0
            steps = len(loop._steps)
            prof = {k: v for k, v in loop.engine.profile_read().items() if v["launches"]} if profile else None
        return wall / steps * 1e3, steps, prof

    result = {"what": "ms per lock step of resident distribution-aware loops; rec = on a recorded sample tensor "
                      "(fot_loop_set_samples), gan = with the library's own sampler (fot_loop_set_sampler)",
              "label": args.label, "prediction_scores": bool(args.scores), "pedestrians": P, "max_steps": args.steps, "capacity": cap or 64,
              "FOT_NAN_SCAN": os.environ.get("FOT_NAN_SCAN", "lazy (default)"),
              "recording": "float32, device memory, record_samples of the counter-seeded SganSampler",
              "repeats": args.repeats, "order": "warm-up of every form, then the forms in turn, repeated", "runs": {}}
    for n_epi in args.episodes:
        for S in args.samples:
            tracks = [track] * n_epi
            smp = SganSampler(None, w, S, counter_seed=SEED, **src_kw(S))
            with BatchedClosedLoop(cfg, tracks, sample_source=smp, device_samples=True, **loop_kw):   # (binds the sampler)
                rec = record_samples(cfg, tracks, smp, args.steps, dtype=np.float32, device="cuda")
            samples = rec.samples
            forms = tuple(args.forms)
            for f in forms:
                one_run(n_epi, f, S, samples)                         # warm-up: code objects, workspace, fresh memory
            runs, steps = {f: [] for f in forms}, 0
            for _ in range(args.repeats):
                for f in forms:
                    ms, steps, _ = one_run(n_epi, f, S, samples)
                    runs[f].append(ms)
            row = {"lock_steps": steps}
            for f in forms:
                row[f] = {"median_ms_per_lock_step": float(np.median(runs[f])), "min": float(min(runs[f])), "max": float(max(runs[f])),
                          "runs": [round(v, 5) for v in runs[f]]}
                if args.profile:
                    row[f]["profiled_run"] = one_run(n_epi, f, S, samples, profile=True)[2]
            result["runs"][f"episodes_{n_epi}_S_{S}"] = row
            print(f"episodes_{n_epi}_S_{S}", json.dumps(row), flush=True)
            del samples, rec
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
