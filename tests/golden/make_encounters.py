#!/usr/bin/env python3
"""Encounter extraction answers of the REFERENCE (build container only) -- data only.

A few small synthetic clips go through the reference's own ``_split_clip_per_vehicle``, ``align_clip_to_grid``,
``extract_encounters``, ``encounters_from_clips`` and ``encounters_from_clips_multivehicle`` (src/datasets/vci_encounter.py)
and ``_cruise_speeds``, ``cruise_upper_quantile``, ``cruise_freewalk`` and ``_far_goals``
(src/simulation/calibration_harness.py).  ``loguru``, ``pysocialforce`` and, where it is missing, ``pandas`` are stubbed: the
file readers are not run.  Only arrays are written: tests/golden/encounters/<clip>.npz and meta.json.  No reference code is
stored.

The clips are chosen so that the reference ALONE produces every outcome, and the generator asserts it with the reference's
own functions: a span that appears only with ``min_len=1`` is SHORT, one that appears only with an infinite threshold is
FAR, one that appears with neither although its vehicle is present is NO_PEDS.  It also asserts the bridged gap, the
gradient fallback's shorter span, the heading crossing +-pi, and every branch of the boundary conditions."""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root
sys.path.insert(0, HERE)
import encounters_common as ec  # noqa: E402
from make_prediction_scores import save_npz  # noqa: E402


def load_reference(ref):
    lg = types.ModuleType("loguru")

    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None

    lg.logger = _Logger()
    sys.modules["loguru"] = lg
    sys.modules.setdefault("pysocialforce", types.ModuleType("pysocialforce"))
    try:
        import pandas  # noqa: F401
    except ImportError:
        pd = types.ModuleType("pandas")
        pd.DataFrame = object
        sys.modules["pandas"] = pd
    sys.path.insert(0, ref)
    os.chdir(ref)
    from src.datasets import vci_encounter, vci_loader
    from src.simulation import calibration_harness as harness
    return vci_loader, vci_encounter, harness


def line(p0, v, T, dt):
    return np.asarray(p0, float)[None] + np.asarray(v, float)[None] * (np.arange(T) * dt)[:, None]


def clip_single():
    """one slow vehicle with recorded heading (crossing +-pi) and speed, a NaN gap inside its track, recorded pedestrian
    velocities; pedestrians for every branch of the boundary conditions"""
    T, dt = 30, 0.4
    times = np.arange(T) * dt
    veh_times = np.arange(-2, 68) * 0.2 + 0.05                                   # its own sampling, beyond the grid at both ends
    Tv = len(veh_times)
    xy = np.stack([-8.0 + 1.5 * veh_times, 0.3 * np.sin(0.4 * veh_times)], axis=1)
    psi = np.pi - 0.02 * (veh_times - 6.0)                                       # drifts through +pi ...
    psi = (psi + np.pi) % (2 * np.pi) - np.pi                                    # ... stored wrapped: a jump of 2 pi
    vel = 1.5 + 0.05 * np.cos(veh_times)
    xy[20:24] = np.nan                                                           # the gap: bridged
    psi[31] = np.nan
    ped = np.zeros((T, 7, 2))
    ped[:, 0] = line([-6.0, 2.0], [1.4, 0.0], T, dt)                             # beside the vehicle all the way: never free-walking
    ped[:, 1] = line([4.0, -9.0], [0.0, 1.2], T, dt) + 0.05 * np.sin(np.arange(T))[:, None]
    out_and_back = np.concatenate([np.arange(15), np.arange(15)[::-1]]) * 0.4    # returns to its start exactly
    ped[:, 2] = np.array([6.0, 5.0])[None] + np.stack([out_and_back, np.zeros(T)], axis=1)
    ped[:, 3] = [2.0, -4.0]                                                      # never moves: +x goal, floored cruise
    ped[:, 4] = line([10.0, 6.0], [-0.9, -0.3], T, dt)
    ped[:, 5] = line([-3.0, 7.0], [0.5, -0.6], T, dt)
    ped[:12, 5] = np.nan                                                         # arrives late: not part of the encounter
    ped[:, 6] = line([0.0, 30.0], [0.3, 0.0], T, dt)
    pvel = ec.velocities(ped, None, dt)
    pvel[:, 2] = np.gradient(ped[:, 2], dt, axis=0)
    pvel[7, 6, 1] = np.nan                                                       # a NaN velocity under a present position
    return dict(name="single", times=times, ped_xy=ped, ped_ids=np.arange(7) * 2 + 10, veh_times=veh_times, veh_xy=xy[:, None],
                veh_ids=np.array([4]), ped_vel=pvel, veh_psi=psi[:, None], veh_vel=vel[:, None])


def clip_nopsi():
    """one vehicle without heading and speed (gradient fallback), no recorded pedestrian velocities"""
    T, dt = 24, 0.5
    times = 3.0 + np.arange(T) * dt
    veh_times = 4.1 + np.arange(40) * 0.2
    xy = np.stack([-10.0 + 3.0 * (veh_times - 4.0), 1.0 + 0.0 * veh_times], axis=1)
    ped = np.zeros((T, 4, 2))
    ped[:, 0] = line([0.0, -5.0], [0.0, 1.0], T, dt)
    ped[:, 1] = line([3.0, 6.0], [0.2, -1.1], T, dt)
    ped[:, 2] = line([-20.0, 3.0], [1.0, 0.0], T, dt)
    ped[18:, 2] = np.nan                                                         # leaves: its last present frame has a NaN velocity
    ped[:, 3] = line([8.0, 2.0], [-0.7, 0.1], T, dt)
    ped[:6, 3] = np.nan
    return dict(name="nopsi", times=times, ped_xy=ped, ped_ids=np.array([7, 3, 9, 1]), veh_times=veh_times, veh_xy=xy[:, None],
                veh_ids=np.array([0]))


def clip_dut3():
    """three vehicles over one crowd: one encounter, one support shorter than min_len, one far away"""
    T, dt = 40, 1 / 2.5
    times = np.arange(T) * dt
    veh_times = np.arange(80) * 0.2
    Tv = len(veh_times)
    xy = np.full((Tv, 3, 2), np.nan)
    xy[10:70, 0] = np.stack([-12.0 + 2.0 * (veh_times[10:70] - 2.0), np.full(60, -1.0)], axis=1)
    xy[30:37, 1] = np.stack([5.0 + veh_times[30:37], np.full(7, 2.0)], axis=1)   # 1.2 s: three grid frames
    xy[:, 2] = np.stack([-30.0 + 4.0 * veh_times, np.full(Tv, 60.0)], axis=1)
    psi = np.zeros((Tv, 3)) + 0.01 * np.arange(Tv)[:, None]
    vel = np.full((Tv, 3), 2.0)
    ped = np.zeros((T, 5, 2))
    ped[:, 0] = line([-5.0, -6.0], [0.1, 0.9], T, dt)
    ped[:, 1] = line([2.0, 4.0], [0.3, -0.8], T, dt)
    ped[:, 2] = line([6.0, -2.0], [-1.0, 0.0], T, dt)
    ped[:, 3] = line([-2.0, 8.0], [0.6, -0.5], T, dt)
    ped[:, 4] = line([12.0, 0.0], [-1.2, 0.2], T, dt)
    ped[:8, 3] = np.nan
    ped[33:, 4] = np.nan
    return dict(name="dut3", times=times, ped_xy=ped, ped_ids=np.array([21, 22, 25, 27, 30]), veh_times=veh_times, veh_xy=xy,
                veh_ids=np.array([5, 2, 8]), veh_psi=psi, veh_vel=vel)


def clip_nobody():
    """one vehicle whose span no pedestrian lasts through"""
    T, dt = 16, 0.4
    times = np.arange(T) * dt
    veh_times = np.arange(34) * 0.2 - 0.1
    xy = np.stack([veh_times * 2.0, np.zeros(34)], axis=1)
    ped = np.zeros((T, 2, 2))
    ped[:, 0] = line([3.0, 1.0], [0.0, 0.5], T, dt)
    ped[:, 1] = line([5.0, -1.0], [0.0, -0.5], T, dt)
    ped[9:, 0] = np.nan
    ped[:5, 1] = np.nan
    return dict(name="nobody", times=times, ped_xy=ped, ped_ids=np.array([1, 2]), veh_times=veh_times, veh_xy=xy[:, None],
                veh_ids=np.array([0]), veh_psi=np.zeros((34, 1)), veh_vel=np.full((34, 1), 2.0))


def to_reference(loader, clip):
    ped_extra = {}
    if clip.get("ped_vel") is not None:
        ped_extra = {"vx": clip["ped_vel"][..., 0], "vy": clip["ped_vel"][..., 1]}
    veh_extra = {k: clip["veh_" + k] for k in ("psi", "vel") if clip.get("veh_" + k) is not None}
    ped = loader.AgentTracks(times=clip["times"], ids=clip["ped_ids"], positions=clip["ped_xy"], extra=ped_extra)
    veh = loader.AgentTracks(times=clip["veh_times"], ids=clip["veh_ids"], positions=clip["veh_xy"], extra=veh_extra)
    return loader.ClipTracks(clip=clip["name"], dataset="dut", scenario=None, ped=ped, veh=veh, ped_path=None, veh_path=None, fps=2.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    out_dir = ec.GOLDEN_DIR
    loader, venc, harness = load_reference(args.ref)
    clips = [clip_single(), clip_nopsi(), clip_dut3(), clip_nobody()]
    meta = {"clips": [c["name"] for c in clips], "encounters": {}, "statuses": {}, "worst_relative_difference": {}}
    statuses = set()
    all_ref = []
    os.makedirs(out_dir, exist_ok=True)
    worst = {"cruise_median": 0.0, "cruise_q85": 0.0, "cruise_free": 0.0, "goals": 0.0}
    for clip in clips:
        ref_clip = to_reference(loader, clip)
        all_ref.append(ref_clip)
        out = {k: clip[k] for k in ec.CLIP_ARRAYS if clip.get(k) is not None}
        subs = venc._split_clip_per_vehicle(ref_clip)
        aligned = [venc.align_clip_to_grid(s) for s in subs]
        out["ref_ego_xy"] = np.stack([a.ego_xy for a in aligned])
        out["ref_ego_psi"] = np.stack([a.ego_psi for a in aligned])
        out["ref_ego_vel"] = np.stack([a.ego_vel for a in aligned])
        out["ref_ped_vel"] = aligned[0].ped_vel
        out["ref_dt"] = np.float64(aligned[0].dt)
        names, per_vehicle = [], []
        n = 0
        for k, a in enumerate(aligned):
            # the outcome of every candidate span of this vehicle, from the reference's own answers under relaxed gates
            here = np.isfinite(a.ego_xy).all(axis=1) & np.isfinite(a.ego_psi) & np.isfinite(a.ego_vel)
            kept = {float(e.times[0]) for e in venc.extract_encounters(a)}
            any_sep = {float(e.times[0]) for e in venc.extract_encounters(a, min_sep_threshold=np.inf)}
            anything = {float(e.times[0]) for e in venc.extract_encounters(a, min_sep_threshold=np.inf, min_len=1)}
            outcome = []
            for run in venc._contiguous_runs(here):
                t0 = float(a.times[run.start])
                status = "KEPT" if t0 in kept else "FAR" if t0 in any_sep else "SHORT" if t0 in anything else "NO_PEDS"
                if status == "NO_PEDS":                             # (a short span without pedestrians would hide here)
                    assert run.stop - run.start >= 5
                outcome.append([int(run.start), int(run.stop), status])
                statuses.add(status)
            per_vehicle.append(outcome)
            for e in venc.extract_encounters(a):
                key = f"enc{n}_"
                for f in ("times", "ego_xy", "ego_psi", "ego_vel", "ped_xy", "ped_vel", "ped_ids"):
                    out[key + f] = getattr(e, f)
                out[key + "min_separation"] = np.float64(e.min_separation)
                out[key + "cruise_median"] = harness._cruise_speeds(e.ped_vel)
                out[key + "cruise_q85"] = harness.cruise_upper_quantile(e)
                out[key + "cruise_free"] = harness.cruise_freewalk(e)
                out[key + "goals"] = harness._far_goals(e.ped_xy, e.ped_vel)
                # the restatement against the reference: the largest relative difference, expected to be 0
                mine = {"cruise_median": ec.cruise_speeds(e.ego_xy, e.ped_xy, e.ped_vel, "median"),
                        "cruise_q85": ec.cruise_speeds(e.ego_xy, e.ped_xy, e.ped_vel, "quantile", 0.85),
                        "cruise_free": ec.cruise_speeds(e.ego_xy, e.ped_xy, e.ped_vel, "freewalk", 0.5, 8.0),
                        "goals": ec.far_goals(e.ped_xy, e.ped_vel)}
                for name, got in mine.items():
                    want = out[key + name]
                    worst[name] = max(worst[name], ec.relative_difference(got, want))
                names.append(e.clip)
                n += 1
        meta["encounters"][clip["name"]] = names
        meta["statuses"][clip["name"]] = per_vehicle
        save_npz(os.path.join(out_dir, clip["name"] + ".npz"), out)
    meta["worst_relative_difference"] = worst
    # ---- the order over clips, and the single-vehicle contract
    meta["multivehicle"] = [e.clip for e in venc.encounters_from_clips_multivehicle(all_ref)]
    meta["single_vehicle_only"] = [e.clip for e in venc.encounters_from_clips(all_ref)]
    assert meta["multivehicle"] == sum((meta["encounters"][c] for c in meta["clips"]), [])
    # ---- every outcome and branch occurs, by the reference alone
    assert statuses == {"KEPT", "SHORT", "NO_PEDS", "FAR"}, statuses
    single, nopsi = (np.load(os.path.join(out_dir, n + ".npz")) for n in ("single", "nopsi"))
    gap_times = single["veh_times"][20:24]
    inside = (single["times"] > gap_times[0]) & (single["times"] < gap_times[-1])
    assert inside.any() and np.isfinite(single["ref_ego_xy"][0][inside]).all()                  # the gap is bridged
    assert np.any(np.abs(np.diff(single["enc0_ego_psi"])) > 6.0)                               # the heading crosses +-pi
    pos_ok = np.flatnonzero(np.isfinite(nopsi["ref_ego_xy"][0]).all(axis=1))
    assert nopsi["enc0_times"][0] == nopsi["times"][pos_ok[0] + 1] and nopsi["enc0_times"][-1] == nopsi["times"][pos_ok[-1] - 1]
    goals, start = single["enc0_goals"], single["enc0_ped_xy"][0]
    ids = single["enc0_ped_ids"].tolist()
    head = (goals - start) / 50.0
    net = single["enc0_ped_xy"][-1] - start
    j_back, j_still, j_beside = ids.index(14), ids.index(16), ids.index(10)
    assert np.hypot(*net[j_back]) < 1e-3 and np.hypot(*single["enc0_ped_vel"][0, j_back]) > 1e-3      # first velocity used
    assert np.hypot(*net[j_still]) < 1e-3 and np.allclose(head[j_still], [1.0, 0.0])                  # the +x fallback
    assert single["enc0_cruise_median"][j_still] == 1e-3                                              # floored
    d_beside = np.hypot(*(single["enc0_ped_xy"][:, j_beside] - single["enc0_ego_xy"]).T)
    assert d_beside.max() <= 8.0                                                                      # freewalk falls back
    assert 20 not in ids and 22 not in ids                                                          # late arrival; NaN velocity
    assert "ped_vel" not in nopsi.files and len(meta["encounters"]["dut3"]) == 1 and meta["encounters"]["dut3"][0] == "dut3#v5"
    with open(os.path.join(out_dir, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    size = sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir))
    print(out_dir, size, "bytes;", meta["statuses"], worst)


if __name__ == "__main__":
    main()
