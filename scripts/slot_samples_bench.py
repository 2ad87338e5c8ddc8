#!/usr/bin/env python3
"""Time per lock step of a sample-count ablation run as ONE sweep loop with a count per slot (fot_loop_set_slot_samples)
against the same episodes run as one loop per distinct count, one after another -- the only route without per-slot counts.

(a) --mode ablation: 64 slots = 8 crowds x 30 pedestrians x counts {5, 10, 20, 50, 100, 100, 200, 200} on a handle raised to
    200, resident, distribution-aware; form `rec` on a shared device recording of 200 samples (RecordedSamples(slot_col0=,
    slot_samples=)), form `gan` with the shared sampler (SganSampler(slot_crowd=, slot_samples=)).  `separate` is the sum
    over the distinct counts of the ms per lock step of the uniform loop of that count over its slots (a recording cut to
    the count / a sampler of the count).  A warm-up of everything, then --repeats rounds; median, min, max, every run kept.
(b) --mode unchanged: a sweep WITHOUT slot counts (two alternating conditions) at 64 x S = 20 and 256 x S = 64 on a shared
    recording; run once per process against this build and, with --lib, against another build's libfot.so.

    python3 scripts/slot_samples_bench.py --mode ablation --out profiles/r35_slot_samples.json
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
COUNTS = (5, 10, 20, 50, 100, 100, 200, 200)
N_CROWDS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="ablation", choices=["ablation", "unchanged"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--forms", nargs="+", default=["rec", "gan"], choices=["rec", "gan"])
    ap.add_argument("--lib", default=None, help="another build's libfot.so (mode unchanged: the parent commit's)")
    args = ap.parse_args()
    from integrated_path_planning_amd import _abi
    if args.lib:
        _abi.LIB_PATH = os.path.abspath(args.lib)
    import sgan_common as sc
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    from integrated_path_planning_amd.prediction import RecordedSamples, SganSampler, SganWeights, record_samples
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False)
    cfg = dict(json.loads(str(z["meta"]))["config"], distribution_aware_planning=True, chance_epsilon=0.2)
    tr = z["base_ped_traj"]
    track = np.concatenate([tr, tr + np.array([0.7, 9.0]), tr[:, :2] + np.array([-0.5, -9.0])], axis=1)
    assert track.shape[1] == P
    a = dict(obs_len=cfg["obs_len"], pred_len=cfg["pred_len"], num_layers=1, pooling_type="pool_net", pool_every_timestep=False,
             noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
    w = SganWeights.from_state_dict(a, sc.seeded_state(a, 11, 3.0))

    def timed(loop):
        with loop:
            t0 = time.perf_counter()
            loop.run(args.steps)
            return (time.perf_counter() - t0) / len(loop._steps) * 1e3

    def summary(runs):
        return {"median_ms_per_lock_step": float(np.median(runs)), "min": float(min(runs)), "max": float(max(runs)),
                "runs": [round(v, 5) for v in runs]}

    result = {"label": args.label, "mode": args.mode, "pedestrians": P, "max_steps": args.steps, "repeats": args.repeats,
              "library": args.lib or "this build", "FOT_NAN_SCAN": os.environ.get("FOT_NAN_SCAN", "lazy (default)"), "runs": {}}
    if args.mode == "unchanged":
        result["what"] = "ms per lock step of a resident sweep WITHOUT slot counts (two alternating conditions) on a shared device recording"
        cfgs2 = [cfg, dict(cfg, chance_epsilon=0.0)]
        for n_epi, S in ((64, 20), (256, 64)):
            smp = SganSampler(None, w, S, counter_seed=SEED)
            with BatchedClosedLoop(cfg, [track], sample_source=smp, device_samples=True):
                rec = record_samples(cfg, [track], smp, args.steps, dtype=np.float32, device="cuda").samples
            loop = lambda: BatchedClosedLoop([cfgs2[e % 2] for e in range(n_epi)], [track] * n_epi, device_samples=True, resident=True,
                                             sample_source=RecordedSamples(rec, slot_col0=[0] * n_epi))
            timed(loop())
            row = summary([timed(loop()) for _ in range(args.repeats)])
            result["runs"][f"episodes_{n_epi}_S_{S}"] = row
            print(f"episodes_{n_epi}_S_{S}", json.dumps(row), flush=True)
    else:
        result["what"] = ("ms per lock step: `sweep` = 64 slots (8 crowds x the counts) in ONE loop with a count per slot; `separate` = the "
                          "sum over the distinct counts of the uniform loop of that count over its slots, run one after another")
        result["counts"], result["crowds"], result["capacity"] = list(COUNTS), N_CROWDS, max(COUNTS)
        cap = max(COUNTS)
        crowds = [track + np.array([0.05 * c, 0.0]) for c in range(N_CROWDS)]
        slot_crowd = [c for c in range(N_CROWDS) for _ in COUNTS]
        slot_S = [k for _ in range(N_CROWDS) for k in COUNTS]
        tracks = [crowds[c] for c in slot_crowd]
        smp = SganSampler(None, w, cap, counter_seed=SEED, sample_capacity=cap)
        with BatchedClosedLoop(cfg, crowds, sample_source=smp, device_samples=True, sample_capacity=cap):
            rec = record_samples(cfg, crowds, smp, args.steps, dtype=np.float32, device="cuda").samples    # [steps, 200, L, 8 * 30, 2]
        col0 = [P * c for c in slot_crowd]
        kw = dict(device_samples=True, resident=True, sample_capacity=cap)

        def sweep(form):
            src = (RecordedSamples(rec, slot_col0=col0, slot_samples=slot_S, sample_capacity=cap) if form == "rec" else
                   SganSampler(None, w, cap, counter_seed=SEED, slot_crowd=slot_crowd, slot_samples=slot_S, sample_capacity=cap))
            return timed(BatchedClosedLoop(cfg, tracks, sample_source=src, **kw))

        def separate(form):
            total, parts = 0.0, {}
            for k in sorted(set(COUNTS)):
                idx = [e for e, s in enumerate(slot_S) if s == k]
                src = (RecordedSamples(rec[:, :k].contiguous(), slot_col0=[col0[e] for e in idx], sample_capacity=cap) if form == "rec" else
                       SganSampler(None, w, k, counter_seed=SEED, slot_crowd=[slot_crowd[e] for e in idx], sample_capacity=cap))
                parts[k] = timed(BatchedClosedLoop(cfg, [tracks[e] for e in idx], sample_source=src, **kw))
                total += parts[k]
            return total, parts
        for form in args.forms:
            sweep(form), separate(form)                               # warm-up: code objects, workspace, fresh memory
            runs, parts = {"sweep": [], "separate": []}, []
            for _ in range(args.repeats):
                runs["sweep"].append(sweep(form))
                t, p = separate(form)
                runs["separate"].append(t)
                parts.append({str(k): round(v, 5) for k, v in p.items()})
            row = {"sweep": summary(runs["sweep"]), "separate": summary(runs["separate"]), "separate_by_count": parts}
            result["runs"][form] = row
            print(form, json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
