#!/usr/bin/env python3
"""What mixing scenarios in one plan call buys (GPU box): 256 instances spread over the three scenario settings of
synthetic.SCENARIO_PLANNERS, float32 obstacle distributions resident in HBM, planned
  (a) by three single-scenario handles: three plan calls (one stream each), then one synchronisation;
  (b) by one handle holding the three scenarios: one mixed plan call, then one synchronisation.
Each way: warm-up, then --repeats repeats of --steps steps; prints one JSON line with the median ms per step."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from integrated_path_planning_amd import _abi, synthetic as syn  # noqa: E402
from integrated_path_planning_amd.batch import PackedBatch, request_from_instance  # noqa: E402
from integrated_path_planning_amd.planner import BatchPlanner  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    n = a.instances
    reqs = []
    for i in range(n):
        r = request_from_instance(syn.config3_instance(i))
        r.scenario = i % 3
        reqs.append(r)

    def device_batch(rq):
        pb = PackedBatch(rq, np.float32)
        dyn = torch.from_numpy(pb.dyn_xy).to(dev)
        out = torch.zeros(len(rq) * _abi.RESULT_BYTES, dtype=torch.uint8, device=dev)
        return pb, dyn, out, pb.with_device_obstacles(None, dyn.data_ptr())

    # (a) three handles
    singles = []
    for k, (w, kw) in enumerate(syn.SCENARIO_PLANNERS):
        sub = [r for r in reqs if r.scenario == k]
        for r in sub:
            r.scenario = 0
        singles.append((BatchPlanner(waypoints=w, device=0, **kw), device_batch(sub), torch.cuda.Stream(device=dev)))
        for r in sub:
            r.scenario = k
    # (b) one handle, three scenarios
    (w0, kw0), *rest = syn.SCENARIO_PLANNERS
    mixed = BatchPlanner(waypoints=w0, device=0, **kw0)
    for w, kw in rest:
        mixed.add_scenario(waypoints=w, **kw)
    mb = device_batch(reqs)
    mst = torch.cuda.Stream(device=dev)

    def step_a():
        for bp, (pb, dyn, out, bs), st in singles:
            bp.plan_packed_device(bs, out.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize(dev)

    def step_b():
        pb, dyn, out, bs = mb
        mixed.plan_packed_device(bs, out.data_ptr(), mst.cuda_stream, scenario=pb)
        torch.cuda.synchronize(dev)

    def timed(step):
        for _ in range(a.warmup):
            step()
        reps = []
        for _ in range(a.repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            reps.append((time.perf_counter() - t0) * 1e3 / a.steps)
        return reps

    ra, rb = timed(step_a), timed(step_b)
    # the two ways compute the same records
    mixed_out = mb[2].cpu().numpy().tobytes()
    same = True
    for k, (_, (_, _, out, _), _) in enumerate(singles):
        one_out = out.cpu().numpy().tobytes()
        for j, i in enumerate(i for i in range(n) if reqs[i].scenario == k):
            R = _abi.RESULT_BYTES
            same &= mixed_out[i * R:(i + 1) * R] == one_out[j * R:(j + 1) * R]
    line = {"metric": "scenario mix: ms per step", "instances": n, "scenarios": 3, "steps": a.steps,
            "repeats": a.repeats, "three_handles_ms": float(np.median(ra)), "one_mixed_call_ms": float(np.median(rb)),
            "three_handles_reps": [round(x, 5) for x in ra], "one_mixed_call_reps": [round(x, 5) for x in rb],
            "speedup": float(np.median(ra) / np.median(rb)), "records_equal": bool(same),
            "workload": "config3_instance(seed) x 256 (20 samples x 30 pedestrians x 51 steps, float32, HBM), "
                        "instance i on scenario i mod 3"}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    for bp, _, _ in singles:
        bp.close()
    mixed.close()


if __name__ == "__main__":
    main()
