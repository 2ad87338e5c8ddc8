"""Measurement: plan calls against prediction distributions of 64, 100 and 200 samples (one MI355X).

256 instances of synthetic.config3_instance(seed, S, P=30) per call, float32 tensors resident in HBM, on a handle whose
sample capacity was raised to 254 (BatchPlanner(sample_capacity=254)): S = 64 runs the kernels a default handle runs,
S = 100 and 200 the wide kernels (eps = 0: k_evaluate*_lean_wide, eps = 0.05: k_evaluate*_wide).  The S = 64 rows are
taken on a default handle as well.  Per row: ms per call (host clock around calls that end in a device synchronise,
profiling off) and, from a second pass with fot_profile_enable, the per-kernel split of fot_profile_read.

    python3 scripts/wide_samples_bench.py --out profiles/rNN_wide_samples.json [--sizes 64 100 200] [--steps 20]

FOT_NAN_SCAN=eager in the environment gives the rows with k_frenet_state's scan blocks flagging the NaN tracks instead
of k_cull's lazy check (S P = 6000 tracks per step are far beyond the 256 tracks the lazy check remembers per group).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from integrated_path_planning_amd import _abi, synthetic as syn  # noqa: E402
from integrated_path_planning_amd.batch import PackedBatch, request_from_instance  # noqa: E402
from integrated_path_planning_amd.planner import BatchPlanner  # noqa: E402

N_INST = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 100, 200])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for S in args.sizes:
        reqs = [request_from_instance(syn.config3_instance(s, S=S, P=30)) for s in range(N_INST)]
        pb = PackedBatch(reqs, obstacle_dtype=np.float32)
        dyn_dev = torch.from_numpy(pb.dyn_xy).to(dev)
        out_dev = torch.zeros(N_INST * _abi.RESULT_BYTES, dtype=torch.uint8, device=dev)
        bstruct = pb.with_device_obstacles(None, dyn_dev.data_ptr())
        stream = torch.cuda.current_stream(dev)
        for eps in (0.0, 0.05):
            for capacity in ((None, 254) if S <= _abi.MAX_SAMPLES else (254,)):
                bp = BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, sample_capacity=capacity,
                                  **dict(syn.CONFIG3_PLANNER, chance_epsilon=eps))

                def run(n):
                    t0 = time.perf_counter()
                    for _ in range(n):
                        bp.plan_packed_device(bstruct, out_dev.data_ptr(), stream.cuda_stream)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / n * 1e3
                run(args.warmup)
                reps = [run(args.steps) for _ in range(3)]
                form, flat = bp.last_eval_form(), bool(bp.set_flat(-1))
                bp.profile(True)
                bp.profile_read(reset=True)
                run(args.steps)
                prof = bp.profile_read(reset=True)
                bp.profile(False)
                recs = (_abi.Result * N_INST).from_buffer_copy(out_dev.cpu().numpy().tobytes())
                row = {"S": S, "P": 30, "instances": N_INST, "eps": eps, "max_viol": int(np.floor(eps * S)),
                       "sample_capacity": bp.sample_capacity, "eval_form": form, "flat_kernel": flat,
                       "ms_per_call": min(reps), "ms_per_call_repeats": reps,
                       "kernel_ms": {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()},
                       "paths_found": int(sum(1 for r in recs if r.best_index >= 0)),
                       "candidates": int(sum(r.n_cand for r in recs)),
                       "collision_error": int(sum(r.stats[_abi.ST_COLLISION] for r in recs))}
                rows.append(row)
                print(json.dumps(row), flush=True)
                bp.close()
        del dyn_dev, out_dev
    doc = {"what": "256 x config3_instance(seed, S, P=30), float32 tensors in HBM, one plan call per step; ms_per_call: best of "
                   "three windows of --steps calls, profiling off; kernel_ms: fot_profile_read over one more window",
           "nan_scan": os.environ.get("FOT_NAN_SCAN", "lazy (default)"), "steps": args.steps, "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
