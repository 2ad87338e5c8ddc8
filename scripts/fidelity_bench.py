#!/usr/bin/env python3
"""What the encounter-fidelity report costs: ``fidelity.fidelity_report`` on a DUT-sized stand-in against the host.

The stand-in: ``--encounters`` (2000) seeded encounters of 30 to 300 steps and 1 to 30 pedestrians at 23.98 fps, each with a
roll-out of its own (tests/fidelity_common.py: random_encounter, rollout_of).  Timed, each a median of ``--repeats`` (5) runs
after one warm-up, every run listed:

* ``gpu_report``: ``fidelity_report(engine, encounters, rollouts)`` whole -- packing the inputs, the two
  ``fot_fidelity_eval`` calls with their copies to and from the device, the pooling and the KS tests on the host;
* ``gpu_library_calls``: the two library calls alone, on inputs already packed;
* ``host_numpy``: the NumPy restatement (vectorised per encounter) producing the same records for both sides;
* ``host_loop``: the reference-shaped form -- a Python double loop over (pedestrian, step) for the onset -- over the first
  ``--loop-encounters`` encounters only, its time scaled to all of them and marked so.

The GPU's dictionary is compared with the host's on the same inputs.  ``--accuracy FILE`` merges what
tests/test_gpu_fidelity.py wrote under FOT_FIDELITY_PROFILE (the largest value difference of the GPU tests).

    python3 scripts/fidelity_bench.py --out profiles/r28_fidelity.json [--accuracy FILE]
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
import fidelity_common as fc  # noqa: E402

DT = 1 / 23.98


def stand_in(n, seed=28):
    rng = np.random.default_rng(seed)
    encs = [fc.with_drift(rng, fc.random_encounter(rng, int(rng.integers(30, 301)), int(rng.integers(1, 31)), DT, vel=False))
            for _ in range(n)]
    return encs, [fc.rollout_of(e) for e in encs]


def timed(fn, repeats):
    fn()                                                            # warm-up: code objects, workspace, fresh memory
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        runs.append(time.perf_counter() - t0)
    return out, {"median_s": float(np.median(runs)), "min_s": min(runs), "max_s": max(runs), "runs_s": runs}


def host_numpy(encs, sims):
    truth = [e["ped_xy"] for e in encs]
    real = fc.evaluate(encs)
    sim = fc.evaluate([dict(e, ped_xy=s) for e, s in zip(encs, sims)], truth=truth)
    return real, sim


def host_loop(encs, sims):
    out = []
    for e, s in zip(encs, sims):
        real_sep, sim_sep = fc.separation(e["ego_xy"], e["ped_xy"]), fc.separation(e["ego_xy"], s)
        real_on = fc.onset_loop(e["ego_xy"], e["ped_xy"], dt=e["dt"])
        sim_on = fc.onset_loop(e["ego_xy"], s, dt=e["dt"])
        err = fc.ped_error(e["ego_xy"], s, e["ped_xy"])[2][1:]
        out.append((float(np.min(real_sep)), float(np.min(sim_sep)), real_on, sim_on, float(np.sum(err)), err.size))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--encounters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-encounters", type=int, default=100)
    ap.add_argument("--accuracy", default=None)
    args = ap.parse_args()

    from integrated_path_planning_amd import batch, fidelity, synthetic as syn
    from integrated_path_planning_amd.planner import BatchPlanner

    encs, sims = stand_in(args.encounters)
    steps = sum(len(e["ego_xy"]) for e in encs)
    peds = sum(e["ped_xy"].shape[1] for e in encs)
    rows = sum(e["ped_xy"].shape[0] * e["ped_xy"].shape[1] for e in encs)
    result = {"stand_in": {"encounters": len(encs), "steps": steps, "pedestrians": peds, "pedestrian_steps": rows, "dt": DT,
                           "bytes_to_device_both_calls": 16 * rows * 3 + 2 * 16 * steps,
                           "bytes_from_device_both_calls": 2 * (8 * steps + 12 * peds + 32 * len(encs))},
              "method": "host clock around calls that end in the library's own stream synchronise; one warm-up, then "
                        f"{args.repeats} runs each, median with min and max; all forms in one process on one MI355X box"}
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as engine:
        report, result["gpu_report"] = timed(lambda: fidelity.fidelity_report(engine, encs, sims), args.repeats)
        ego, rec = [e["ego_xy"] for e in encs], [e["ped_xy"] for e in encs]
        dts = [e["dt"] for e in encs]
        p_real = batch.PackedEncounters(ego, rec, dts)
        p_sim = batch.PackedEncounters(ego, sims, dts, truth_xy=rec)
        _, result["gpu_library_calls"] = timed(lambda: (engine.fidelity_eval(p_real), engine.fidelity_eval(p_sim)), args.repeats)
    (real, sim), result["host_numpy"] = timed(lambda: host_numpy(encs, sims), args.repeats)
    n_loop = min(args.loop_encounters, len(encs))
    share = sum(e["ped_xy"].shape[0] * e["ped_xy"].shape[1] for e in encs[:n_loop]) / rows
    _, loop = timed(lambda: host_loop(encs[:n_loop], sims[:n_loop]), args.repeats)
    loop.update(encounters_timed=n_loop, share_of_pedestrian_steps=share, scaled_to_all_median_s=loop["median_s"] / share,
                note="measured over the first encounters only and scaled by their share of the pedestrian steps")
    result["host_loop"] = loop
    # ---- the same numbers on both sides
    on = lambda ev: [ev[2][ev[3] >= 0]]
    agree = {"closest_real_equal": report["closest_real_raw"] == [float(v) for v in real[0]["closest"]],
             "closest_sim_equal": report["closest_sim_raw"] == [float(v) for v in sim[0]["closest"]],
             "onset_real_equal": bool(np.array_equal(report["onset_real_raw"], on(real)[0])),
             "onset_sim_equal": bool(np.array_equal(report["onset_sim_raw"], on(sim)[0])),
             "rollout_ade_gpu": report["rollout_ade"],
             "rollout_ade_host": float(sim[0]["err_sum"].sum() / sim[0]["err_count"].sum())}
    result["agreement_with_host_numpy"] = agree
    result["report"] = {k: report[k] for k in ("n_encounters", "rollout_ade", "mean_closest_sim", "mean_closest_real", "ks_closest",
                                               "p_closest", "n_onset_sim", "n_onset_real", "ks_onset", "p_onset")}
    g = result["gpu_report"]["median_s"]
    result["speedup_over_host_numpy"] = result["host_numpy"]["median_s"] / g
    result["speedup_over_host_loop_scaled"] = loop["scaled_to_all_median_s"] / g
    if args.accuracy and os.path.exists(args.accuracy):
        with open(args.accuracy) as f:
            result["gpu_test_accuracy"] = json.load(f)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("speedup_over_host_numpy", "speedup_over_host_loop_scaled", "agreement_with_host_numpy")}))
    for k in ("gpu_report", "gpu_library_calls", "host_numpy", "host_loop"):
        print(k, {a: round(b, 4) for a, b in result[k].items() if a.endswith("_s") and not isinstance(b, list)})


if __name__ == "__main__":
    main()
