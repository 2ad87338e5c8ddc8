#!/usr/bin/env python3
"""What one fot_sgan_sample call costs: 256 scenes x 30 pedestrians, S = 20 samples, the (16, 32, 32, 64, 8, 8) model
(embedding, encoder h, decoder h, mlp, bottleneck, noise) with seeded weights, for the four combinations of pooling x
pool_every_timestep; obs, noise and out in device memory.

Per combination: ``ms``, the HIP-event time of one call on the caller's stream after warm-up (events around --calls
calls, divided), median of --repeats; ``gflop``, the operations the model needs for the call counted from the shapes
(one multiply-add = 2; the rearranged first pool layer counted as it is computed); ``tflops`` = gflop / ms and
``share_of_f32_vector_peak`` of the MI355X's 157.3 TFLOP/s (spec) -- a whole-call figure, launch gaps included, not a
kernel's.  There is no baseline: nothing produced this tensor before, and the reference's model does not run there.

    python3 scripts/sgan_bench.py --out profiles/r10_sgan.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SCENES, P, S = 256, 30, 20
DIMS = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=8, noise_dim=(8,))
PEAK_TFLOPS = 157.3


def flops(a, n_scenes, p, s):
    """Floating-point operations of one call, from the shapes."""
    e, he, hd, m, nd = a["embedding_dim"], a["encoder_h_dim"], a["decoder_h_dim"], a["mlp_dim"], a["noise_dim"][0]
    b = a["bottleneck_dim"] if a["pooling_type"] else 0
    n, t, L = n_scenes * p, a["obs_len"], a["pred_len"]
    lstm = lambda h: 2 * 4 * h * (e + h) + 4 * e                   # one cell, its embedding included
    pool = lambda h: n * 2 * 512 * h + n_scenes * p * p * (512 * 4 + 2 * 512 * b)
    mlp = lambda k, o: 2 * (k * m + m * o)
    total = n * t * lstm(he)
    if a["pooling_type"]:
        total += pool(he)
    if nd or a["pooling_type"] or he != hd:
        total += n * mlp(he + b, hd - nd)
    total += s * n * L * (lstm(hd) + 4 * hd)
    if a["pooling_type"] and a["pool_every_timestep"]:
        total += s * (L - 1) * (pool(hd) + n * mlp(hd + b, hd))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import sgan_common as sc
    from integrated_path_planning_amd import _abi, synthetic as syn
    from integrated_path_planning_amd.planner import BatchPlanner
    from integrated_path_planning_amd.prediction import SganWeights

    if not torch.cuda.is_available():
        raise SystemExit("sgan_bench.py measures on the GPU; none found")
    lib = _abi.lib()
    rng = np.random.default_rng(3)
    n = N_SCENES * P
    off = (np.arange(N_SCENES + 1) * P).astype(np.int32)
    start = rng.uniform(-6.0, 6.0, size=(n, 2))
    vel = rng.uniform(-0.6, 0.6, size=(n, 2))
    obs = torch.from_numpy((start[None] + np.cumsum(vel[None] + rng.normal(0, 0.05, (sc.OBS_LEN, n, 2)), axis=0)).astype(np.float32)).cuda()
    results = {}
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        for pooling in (None, "pool_net"):
            for every in (False, True):
                a = dict(obs_len=sc.OBS_LEN, pred_len=sc.PRED_LEN, num_layers=1, pooling_type=pooling, pool_every_timestep=every,
                         noise_mix_type="ped", batch_norm=False, dropout=0.0, **DIMS)
                w = SganWeights.from_state_dict(a, sc.seeded_state(a, 11, 3.0))
                _abi.check(bp._h, lib.fot_sgan_load(bp._h, C.byref(w.desc), w.blob.size, w.blob.ctypes.data))
                noise = torch.randn((S, n, DIMS["noise_dim"][0]), device="cuda", dtype=torch.float32)
                out = torch.empty((S, sc.PRED_LEN, n, 2), device="cuda", dtype=torch.float32)
                stream = torch.cuda.current_stream()
                torch.cuda.synchronize()

                def call():
                    _abi.check(bp._h, lib.fot_sgan_sample(bp._h, N_SCENES, off.ctypes.data, C.c_void_p(obs.data_ptr()), S,
                                                          C.c_void_p(noise.data_ptr()),
                                                          _abi.OUT_DEVICE | _abi.SGAN_OBS_DEVICE | _abi.SGAN_NOISE_DEVICE,
                                                          C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))

                for _ in range(3):
                    call()
                assert torch.isfinite(out).all()
                times = []
                for _ in range(args.repeats):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    for _ in range(args.calls):
                        call()
                    t1.record(stream)
                    t1.synchronize()
                    times.append(t0.elapsed_time(t1) / args.calls)
                ms = float(np.median(times))
                gf = flops(a, N_SCENES, P, S) / 1e9
                key = f"{'pool_net' if pooling else 'none'}{'_every_step' if every and pooling else '_every_step_flag' if every else ''}"
                results[key] = dict(ms=ms, ms_all=[float(t) for t in times], gflop=gf, tflops=gf / ms, 
                                    share_of_f32_vector_peak=gf / ms / PEAK_TFLOPS)
                print(key, json.dumps(results[key]), flush=True)
    doc = dict(workload=dict(scenes=N_SCENES, pedestrians_per_scene=P, samples=S, obs_len=sc.OBS_LEN, pred_len=sc.PRED_LEN,
                             dims={k: (list(v) if isinstance(v, tuple) else v) for k, v in DIMS.items()}),
               method=f"HIP events around {args.calls} calls on the caller's stream after 3 warm-up calls, median of {args.repeats}",
               f32_vector_peak_tflops=PEAK_TFLOPS, lock_step_ms_for_scale=[1.16, 1.21], results=results)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
