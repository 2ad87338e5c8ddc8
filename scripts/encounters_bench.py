#!/usr/bin/env python3
"""Cutting encounters out of recorded clips on an MI355X: ``fidelity.extract_encounters(..., cruise='median',
measure_real=True)`` end to end, inputs included, against the route the package offered before for the same numbers -- the
NumPy restatement of the extraction and the boundary conditions (tests/encounters_common.py) plus ``fidelity_batch`` for
the recorded side.

The workload is a DUT-shaped synthetic set: ``--clips`` clips of ``--frames`` frames at 23.98 fps, ``--peds`` pedestrians
that come and go, ``--vehicles`` vehicles that each cross the scene once.  Both routes align the vehicles on the host with
the same code; both are compared on what they return (encounters, closest approaches, cruise speeds, goals, the recorded
side's records).  The file records both times and the bytes sent to the device: one scene per clip on the new route, every
encounter's packed copy on the old one.  ``--accuracy FILE`` merges what tests/test_encounters_cpu.py wrote under
FOT_ENCOUNTERS_PROFILE.

    python3 scripts/encounters_bench.py --out profiles/r29_encounters.json [--accuracy FILE]
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
import encounters_common as ec  # noqa: E402

FPS = 23.98


def stand_in(n_clips, T, A, K, seed=29):
    """clips of T frames: pedestrians present for 8 to 40 s somewhere in the clip, vehicles crossing in 6 to 20 s on their
    own sampling (half the grid's rate), with recorded heading and speed"""
    rng = np.random.default_rng(seed)
    dt = 1.0 / FPS
    clips = []
    for c in range(n_clips):
        times = np.arange(T) * dt
        ped = ec.walkers(rng, T, A, dt, speed=1.3, box=15.0)
        for a in range(A):
            stay = int(rng.integers(int(8 * FPS), int(40 * FPS)))
            t0 = int(rng.integers(0, max(T - stay, 1)))
            ped[:t0, a] = np.nan
            ped[t0 + stay:, a] = np.nan
        Tv = T // 2
        veh_times = np.arange(Tv) * (2 * dt) + 0.3 * dt
        veh = np.full((Tv, K, 2), np.nan)
        psi, vel = np.full((Tv, K), np.nan), np.full((Tv, K), np.nan)
        for k in range(K):
            n = int(rng.integers(int(3 * FPS), int(10 * FPS)))
            a0 = int(rng.integers(0, Tv - n))
            way = rng.uniform(0.0, 2 * np.pi)
            s = np.linspace(-20.0, 20.0, n)
            off = rng.uniform(-8.0, 8.0)
            veh[a0:a0 + n, k] = np.stack([s * np.cos(way) - off * np.sin(way), s * np.sin(way) + off * np.cos(way)], axis=1)
            psi[a0:a0 + n, k] = (way + np.pi) % (2 * np.pi) - np.pi
            vel[a0:a0 + n, k] = 40.0 / (n * 2 * dt)
        clips.append(dict(name=f"clip{c}", times=times, ped_xy=ped, ped_ids=np.arange(A), veh_times=veh_times, veh_xy=veh,
                          veh_ids=np.arange(K), veh_psi=psi, veh_vel=vel))
    return clips


def timed(fns, repeats):
    """the forms in turns, so that whatever else the box is doing falls on all of them alike: one warm-up each (code
    objects, workspace, fresh memory), then `repeats` rounds; per form its last result and its times"""
    outs = [fn() for fn in fns]
    runs = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            outs[i] = fn()
            runs[i].append(time.perf_counter() - t0)
    return outs, [{"median_s": float(np.median(r)), "min_s": min(r), "max_s": max(r), "runs_s": r} for r in runs]


def old_route(engine, fidelity, clips):
    """the restatement's encounters with their boundary conditions, and one fidelity_batch call for the recorded side"""
    encs = ec.extract(clips)
    for e in encs:
        e["cruise"] = ec.cruise_speeds(e["ego_xy"], e["ped_xy"], e["ped_vel"], "median")
        e["far_goals"] = ec.far_goals(e["ped_xy"], e["ped_vel"], 50.0)
    return encs, fidelity.fidelity_batch(engine, encs) if encs else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--peds", type=int, default=150)
    ap.add_argument("--vehicles", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--accuracy", default=None)
    args = ap.parse_args()

    from integrated_path_planning_amd import fidelity, synthetic as syn
    from integrated_path_planning_amd.planner import BatchPlanner

    clips = stand_in(args.clips, args.frames, args.peds, args.vehicles)
    records = [fidelity.RecordedClip(**c) for c in clips]
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as engine:
        (new, (old, old_real), _), (t_new, t_old, t_align) = timed(
            [lambda: fidelity.extract_encounters(engine, records, cruise="median", measure_real=True),
             lambda: old_route(engine, fidelity, clips), lambda: [fidelity.align_vehicles(r) for r in records]], args.repeats)
    cells = sum(e["ped_xy"].shape[0] * e["ped_xy"].shape[1] for e in old)
    steps = sum(e["ped_xy"].shape[0] for e in old)
    same = len(new) == len(old)
    agree = {"encounters_equal": same}
    if same and old:
        agree.update(
            names_equal=[e.clip for e in new] == [e["clip"] for e in old],
            populations_equal=all(np.array_equal(a.ped_ids, b["ped_ids"]) and np.array_equal(a.times, b["times"]) for a, b in zip(new, old)),
            min_separation_equal=all(a.min_separation == b["min_separation"] for a, b in zip(new, old)),
            cruise_equal=all(np.array_equal(a.cruise, b["cruise"]) for a, b in zip(new, old)),
            goals_equal=all(np.array_equal(a.far_goals, b["far_goals"]) for a, b in zip(new, old)),
            recorded_side_equal=all(a.real["record"].tobytes() == r.tobytes() and np.array_equal(a.real["onset_dist"], d, equal_nan=True)
                                    for a, r, d in zip(new, old_real["records"], old_real["onset_dist"])))
    T, A, K = args.frames, args.peds, args.vehicles
    result = {"stand_in": {"clips": args.clips, "frames": T, "pedestrians": A, "vehicles": K, "fps": FPS, "encounters": len(old),
                           "encounter_steps": steps, "pedestrian_steps": cells,
                           "bytes_to_device_new_route": args.clips * (16 * T * A + 16 * K * T) + 16 * steps,
                           "bytes_to_device_old_route": 16 * cells + 16 * steps,
                           "note": "new: one scene per clip, the ego rows and the kept spans' ego rows; old: every encounter's packed copy"},
              "method": "host clock around calls that end in the library's own stream synchronise; one warm-up each, then "
                        f"{args.repeats} rounds with the forms in turns, median with min and max; one process on one MI355X box; "
                        "inputs (alignment, copies to the device) inside the timed region",
              "extract_encounters": t_new, "numpy_restatement_plus_fidelity_batch": t_old, "alignment_alone": t_align,
              "agreement": agree, "speedup": t_old["median_s"] / t_new["median_s"]}
    if args.accuracy and os.path.exists(args.accuracy):
        with open(args.accuracy) as f:
            result["cpu_test_accuracy"] = json.load(f)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("speedup", "agreement")}))
    for k in ("extract_encounters", "numpy_restatement_plus_fidelity_batch", "alignment_alone"):
        print(k, {a: round(b, 4) for a, b in result[k].items() if a.endswith("_s") and not isinstance(b, list)})
    print(result["stand_in"])


if __name__ == "__main__":
    main()
