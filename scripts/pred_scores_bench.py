#!/usr/bin/env python3
"""What scoring the sample predictions on the device costs and what it replaces (fot_loop_prediction_scores,
BatchedClosedLoop(prediction_scores=True)).  64 and 256 episodes x 20 samples x 30 pedestrians on scenario_01's
configuration, the pedestrians walking beside the road; the samples come from a device tensor (device_samples=True).
Median of --repeats for each figure:

* ``call_us``: wall time of one fot_prediction_scores call on the resident distribution blocks of all episodes (one
  launch of k_pred_scores and one synchronisation; the kernel's own device time is what a kernel trace of
  ``--only call`` shows);
* ``step_off_ms`` / ``step_on_ms``: the lock step of the device_samples loop without and with scores, in the same process,
  off / on / off / on;
* ``host_ms``: what it replaces per lock step -- the step's distribution copied to the host and scored by the NumPy
  restatement (tests/pred_scores_common.py).

    python3 scripts/pred_scores_bench.py --out profiles/r09_pred_scores.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, P = 20, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", choices=["call"], default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from closed_loop_common import scripted_sample_source
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    from pred_scores_common import origin_terms
    z = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_dist_episodes.npz"), allow_pickle=False)
    cfg = dict(json.loads(str(z["meta"]))["variants"]["s6_eps02"]["config"])
    rng = np.random.default_rng(0)
    t = np.arange(int(cfg["total_time"] / cfg["dt"]) + 64) * cfg["dt"]
    start = np.stack([rng.uniform(0.0, 60.0, P), rng.uniform(12.0, 30.0, P) * rng.choice([-1.0, 1.0], P)], axis=1)
    vel = rng.normal(0.0, 0.6, (P, 2))
    tracks = start[None] + vel[None] * t[:, None, None]
    host_src = scripted_sample_source(S, cfg["pred_len"])
    dev = torch.device("cuda", 0)
    dev_src = lambda last, prev: torch.from_numpy(np.ascontiguousarray(host_src(last, prev))).to(dev)
    stride, E = int(round(0.4 / cfg["dt"])), int(cfg["pred_len"])
    med = lambda v: float(np.median(v))
    result = {"samples": S, "pedestrians": P, "steps": args.steps, "repeats": args.repeats, "episodes": {}}

    def loop(n_epi, on):
        return BatchedClosedLoop(cfg, [tracks] * n_epi, sample_source=dev_src, device_samples=True, prediction_scores=on)

    for n_epi in args.episodes:
        r = {}
        with loop(n_epi, True) as sim:                               # the call alone, on a frame's resident blocks
            for _ in range(3):
                sim.step()
            sel = np.flatnonzero(sim.alive)
            rows = np.minimum(sim.frame + stride * np.arange(1, E + 1), len(tracks) - 1)
            truth = np.ascontiguousarray(sim._ped_all["trajectories"][rows][:, sim._rows_of(sel)].transpose(1, 0, 2))
            call = []
            for _ in range(5 * args.repeats + 3):
                t0 = time.perf_counter()
                sim.engine.loop_prediction_scores(len(sel), stride, E, truth)
                call.append((time.perf_counter() - t0) * 1e6)
            r["call_us"] = med(call[3:])
        if args.only == "call":
            result["episodes"][str(n_epi)] = r
            continue
        off, on = [], []
        for k in range(2 * args.repeats + 2):                        # off / on / off / on; the first pair warms up
            with loop(n_epi, bool(k & 1)) as sim:
                sim.step()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    sim.step()
                ms = (time.perf_counter() - t0) / args.steps * 1e3
                if k >= 2:
                    (on if k & 1 else off).append(ms)
        r.update(step_off_ms=med(off), step_on_ms=med(on), step_off_all=off, step_on_all=on)
        host = []
        with loop(n_epi, False) as sim:                              # what it replaces: the distribution to the host
            for _ in range(3):
                sim.step()
            o32 = sim._steps[-1]["pred_src"][2]
            stale = sim._steps[-1]["pred_src"][3]
            off_p = np.arange(n_epi + 1) * P
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                raw = dev_src(o32[1].astype(np.float64), o32[0].astype(np.float64)).cpu().numpy()
                dist = sim.resampler.process_prediction(raw, anchor_pos=o32[1].astype(np.float64), staleness=stale)
                for e in range(n_epi):
                    origin_terms(dist[:, off_p[e]:off_p[e + 1]], truth[off_p[e]:off_p[e + 1]], stride)
                host.append((time.perf_counter() - t0) * 1e3)
        r["host_ms"] = med(host)
        result["episodes"][str(n_epi)] = r
        print(n_epi, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}, flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
