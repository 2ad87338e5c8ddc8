#!/usr/bin/env python3
"""Footprint re-verification of the REFERENCE (build container only) -- data only.

Trajectories -- synthetic drives among scattered pedestrians, and the reference's own ego histories of `base`, `rnd3`,
`walls` and `turn` (tests/golden/closed_loop/reference_cv_episodes.npz) paired with pedestrian rows chosen here and stored
explicitly -- go through the reference's own functions:
  * ``observational_footprint_metrics`` (examples/run_footprint_benchmark.py) on histories built from ``SimpleNamespace``;
  * ``recheck`` (examples/recheck_footprint.py) on ``trajectory.npz`` files written to a temporary directory, once with the
    stored ``ego_yaw`` and once without it (the heading reconstructed);
  * ``reconstruct_yaw``;
  * ``EgoFootprint.multi_circle`` for 1, 3, 5 and 8 circles;
  * per step, the three minima as ``recheck`` forms them, from ``circle_centers``, ``world_to_vehicle_frame`` and
    ``rectangle_surface_distance``.
The modules' geometry constants are set per case (vehicle 4.5 m x 2.0 m, pedestrian radius 0.2 m, ego radius 1.0 m unless
the case says otherwise).  No reference code is stored.

The threshold cases put one pedestrian in front of a pose at the origin with yaw = 0, where every operation is exact: the
reference's value is exactly the threshold, one ulp below it and one ulp above it, per geometry.  For the centre and the
circle cover the pedestrian's coordinate IS the value (found by a nextafter walk from the threshold); for the rectangle
|py| - W/2 cannot reach every neighbour of 0.2, so the pedestrian stays and the pedestrian radius -- the threshold itself --
walks.  The moving cases: y = [0, 1, 0], x = [0, 0, 2 v] with v = 1e-4 and its two neighbours: step 1 has dx = v exactly
and dy = 0.

The generator asserts (a condition, not a measurement): outside the threshold cases every per-step value lies at least
1e-9 from its threshold and every hypot(dx, dy) at least 1e-9 from 1e-4.
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types
from pathlib import Path
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root
sys.path.insert(0, HERE)
import footprint_obs_common as fc  # noqa: E402
from make_prediction_scores import save_npz  # noqa: E402

MARGIN = 1e-9
EPISODES = ("base", "rnd3", "walls", "turn")
NEAREST = 4                                                    # pedestrian rows kept per step of a reference episode
RECHECK_COLS = ("legacy_min_dist", "legacy_collision_steps", "multi_min_dist", "multi_clearance", "multi_collision_steps",
                "rect_min_surface_dist", "rect_clearance", "rect_collision_steps")
OBS_COLS = ("legacy_min_dist", "multi_clearance", "multi_violation_steps", "rect_clearance", "rect_violation_steps")


def load_reference(ref):
    lg = types.ModuleType("loguru")

    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None

    lg.logger = _Logger()
    sys.modules["loguru"] = lg
    sys.modules.setdefault("pysocialforce", types.ModuleType("pysocialforce"))
    sys.path.insert(0, ref)
    os.chdir(ref)
    mods = []
    for name in ("recheck_footprint", "run_footprint_benchmark"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref, "examples", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    from src.core import footprint as fp
    return mods[0], mods[1], fp


def set_geometry(rf, rb, fp, geom):
    g = dict(fc.DEFAULT_GEOM, **geom)
    cover = fp.EgoFootprint.multi_circle(g["vehicle_length"], g["vehicle_width"], g["n_circles"])
    rf.VEHICLE_LENGTH, rf.VEHICLE_WIDTH, rf.PED_RADIUS, rf.EGO_RADIUS = g["vehicle_length"], g["vehicle_width"], g["ped_radius"], g["ego_radius"]
    rf.N_CIRCLES, rf.FOOTPRINT = g["n_circles"], cover
    rb.VEHICLE_LENGTH, rb.VEHICLE_WIDTH, rb.PED_RADIUS, rb.OBS_FOOTPRINT = g["vehicle_length"], g["vehicle_width"], g["ped_radius"], cover
    return g, cover


def reference_answers(rf, rb, fp, case, geom, tmp, tag, exempt=False):
    """Everything the reference says about a case, as arrays; asserts the margins unless exempt."""
    g, cover = set_geometry(rf, rb, fp, geom)
    t_legacy, t_multi, t_rect = g["ego_radius"] + g["ped_radius"], cover.radius + g["ped_radius"], g["ped_radius"]
    step_off, xy, yaw, ped_off, ped_xy = (case[k] for k in ("step_off", "xy", "yaw", "ped_off", "ped_xy"))
    steps, n_traj = len(xy), len(step_off) - 1
    series, yaw_recon, moving = np.zeros((steps, 3)), np.full(steps, np.nan), np.zeros(steps, bool)
    rows_stored, rows_recon, obs = np.zeros((n_traj, 8)), np.full((n_traj, 8), np.nan), np.zeros((n_traj, 5))
    rf.REPO = Path(tmp)
    for t, (lo, hi) in enumerate(zip(step_off[:-1], step_off[1:])):
        peds = [ped_xy[ped_off[i]:ped_off[i + 1]].copy() for i in range(lo, hi)]
        for i in range(lo, hi):                                     # the steps' own minima, the reference's functions
            p = peds[i - lo]
            if len(p) == 0:
                series[i] = np.inf
                continue
            centres = cover.circle_centers(xy[i, 0], xy[i, 1], yaw[i])
            local = fp.world_to_vehicle_frame(p, xy[i, 0], xy[i, 1], yaw[i])
            series[i] = (np.min(np.linalg.norm(p - np.array([xy[i, 0], xy[i, 1]]), axis=1)),
                         np.min(np.linalg.norm(p[None, :, :] - centres[:, None, :], axis=2)),
                         np.min(fp.rectangle_surface_distance(local, g["vehicle_length"], g["vehicle_width"])))
        history = [SimpleNamespace(ego_state=SimpleNamespace(x=xy[i, 0], y=xy[i, 1], yaw=yaw[i]),
                                   ped_state=SimpleNamespace(positions=peds[i - lo])) for i in range(lo, hi)]
        m = rb.observational_footprint_metrics(history)
        obs[t] = [m[k] for k in OBS_COLS]
        obj = np.empty(hi - lo, dtype=object)
        for i, p in enumerate(peds):
            obj[i] = p
        for with_yaw, rows in ((True, rows_stored), (False, rows_recon)):
            if not with_yaw and hi - lo < 2:
                continue
            d = Path(tmp) / "output" / f"{tag}_{t}_{int(with_yaw)}"
            d.mkdir(parents=True, exist_ok=True)
            kw = dict(ego_x=xy[lo:hi, 0], ego_y=xy[lo:hi, 1], ped_positions=obj, min_distances=series[lo:hi, 0])
            if with_yaw:
                kw["ego_yaw"] = yaw[lo:hi]
            np.savez(d / "trajectory.npz", **kw)
            r = rf.recheck(d / "trajectory.npz")
            assert r["steps"] == hi - lo and r["yaw_source"] == ("stored" if with_yaw else "reconstructed")
            if with_yaw and np.isfinite(series[lo:hi, 0]).all():
                assert r["stored_vs_recomputed_maxdiff"] == 0.0
            rows[t] = [r[k] for k in RECHECK_COLS]
        if hi - lo >= 2:
            yaw_recon[lo:hi] = rf.reconstruct_yaw(xy[lo:hi, 0], xy[lo:hi, 1])
            dx, dy = np.gradient(xy[lo:hi, 0]), np.gradient(xy[lo:hi, 1])
            speed = np.hypot(dx, dy)
            moving[lo:hi] = speed > 1e-4
            if not exempt:
                assert np.min(np.abs(speed - 1e-4)) >= MARGIN, (tag, t, float(np.min(np.abs(speed - 1e-4))))
    if not exempt:
        fin = np.isfinite(series[:, 0])
        for col, thr in enumerate((t_legacy, t_multi, t_rect)):
            gap = float(np.min(np.abs(series[fin, col] - thr), initial=np.inf))
            assert gap >= MARGIN, (tag, col, gap)
    return {"series": series, "recheck_stored": rows_stored, "recheck_recon": rows_recon, "obs": obs,
            "yaw_recon": yaw_recon, "moving": moving}


def synthetic(rng):
    trajs = []
    for n, counts, start, stand in ((2, [3, 0], (0.0, 0.0), ()), (3, [1, 12, 5], (5.0, -3.0), ()),
                                    (40, None, (90.0, -80.0), ((10, 14),)), (25, None, (-60.0, 40.0), ((0, 3), (20, 24))),
                                    (7, [0] * 7, (1.0, 1.0), ()), (6, None, (0.0, 0.0), ((0, 5),))):
        x, y, heading = fc.drive(rng, n, stand=stand, start=start)
        counts = rng.integers(0, 13, n) if counts is None else counts
        trajs.append((x, y, heading, fc.crowd_near(rng, x, y, counts)))
    return fc.make_case(trajs)


def episode_case(ep, name):
    """The reference's ego history of an episode with, per step, the NEAREST pedestrians of the replayed frame this
    generator pairs it with: frame warm-up + k + 1 of the recording (clamped to its last frame) for lock step k."""
    cfg = ep["meta"]["variants"][name]["config"]
    ego, tracks = ep[name + "_ego"], ep[name + "_ped_traj"]
    warm = int(cfg["obs_len"] * 0.4 / cfg["dt"])
    peds = []
    for k in range(len(ego)):
        row = tracks[min(warm + k + 1, len(tracks) - 1)]
        near = np.argsort(np.linalg.norm(row - ego[k, :2], axis=1), kind="stable")[:NEAREST]
        peds.append(row[np.sort(near)])
    return fc.make_case([(ego[:, 0], ego[:, 1], ego[:, 2], peds)])


def one_step(px, py):
    return fc.make_case([([0.0], [0.0], [0.0], [np.array([[px, py]])])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    out_path = fc.GOLDEN
    with np.load(os.path.join(HERE, "closed_loop", "reference_cv_episodes.npz"), allow_pickle=False) as z:
        ep = {k: z[k] for k in z.files}
    ep["meta"] = json.loads(str(ep["meta"]))
    rf, rb, fp = load_reference(args.ref)
    rng = np.random.default_rng(20250427)
    cases, geoms, exempt = {}, {}, set()
    cases["synth"] = synthetic(rng)
    geoms["synth"] = {}
    for n in (1, 5, 8):
        cases[f"synth_n{n}"] = cases["synth"]
        geoms[f"synth_n{n}"] = {"n_circles": n}
    cases["synth_wide"] = cases["synth"]
    geoms["synth_wide"] = {"vehicle_length": 5.3, "vehicle_width": 2.4, "n_circles": 4, "ped_radius": 0.35, "ego_radius": 1.3}
    for name in EPISODES:
        cases["ep_" + name] = episode_case(ep, name)
        geoms["ep_" + name] = {}
    # ---- the threshold cases: value == threshold, one ulp below it, one ulp above it
    t_legacy, t_multi, t_rect = fc.thresholds({})
    off3, _ = fc.circle_cover(4.5, 2.0, 3)
    for side, step in (("at", None), ("below", -np.inf), ("above", np.inf)):
        v = t_legacy if step is None else np.nextafter(t_legacy, step)
        cases[f"thr_legacy_{side}"], geoms[f"thr_legacy_{side}"] = one_step(v, 0.0), {}
        v = t_multi if step is None else np.nextafter(t_multi, step)
        cases[f"thr_multi_{side}"], geoms[f"thr_multi_{side}"] = one_step(float(off3[-1]), v), {}
        val = abs(1.2) - 2.0 / 2                                     # the rectangle's value of the pedestrian (0, 1.2)
        radius = val if step is None else np.nextafter(val, -step)   # (the threshold walks the other way)
        cases[f"thr_rect_{side}"], geoms[f"thr_rect_{side}"] = one_step(0.0, 1.2), {"ped_radius": float(radius)}
    for side, step in (("at", None), ("below", -np.inf), ("above", np.inf)):
        v = 1e-4 if step is None else float(np.nextafter(1e-4, step))
        cases[f"moving_{side}"] = fc.make_case([([0.0, 0.0, 2 * v], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [np.zeros((0, 2))] * 3)])
        geoms[f"moving_{side}"] = {}
    exempt = {k for k in cases if k.startswith(("thr_", "moving_"))}

    out, meta = {}, {"cases": {}, "recheck_cols": list(RECHECK_COLS), "obs_cols": list(OBS_COLS), "margin": MARGIN,
                     "episodes": list(EPISODES), "nearest": NEAREST, "cover": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in cases.items():
            ans = reference_answers(rf, rb, fp, case, geoms[name], tmp, name, exempt=name in exempt)
            shared = name.startswith("synth_")                      # (the inputs of `synth` again: not stored twice)
            if not shared:
                for k, v in case.items():
                    out[f"{name}_{k}"] = v
            for k, v in ans.items():
                out[f"{name}_{k}"] = v
            meta["cases"][name] = {"geom": geoms[name], "inputs": "synth" if shared else name, "exempt": name in exempt,
                                   "M": fc.magnitude(case["xy"], case["ped_xy"])}
    for n in (1, 3, 5, 8):
        c = fp.EgoFootprint.multi_circle(4.5, 2.0, n)
        meta["cover"][str(n)] = {"offsets": [float(v) for v in c.offsets], "radius": float(c.radius)}
    # ---- what the threshold cases are for, asserted on the reference's own answers
    for g in ("legacy", "multi", "rect"):
        col = {"legacy": 1, "multi": 4, "rect": 7}[g]
        counts = [int(out[f"thr_{g}_{side}_recheck_stored"][0, col]) for side in ("at", "below", "above")]
        assert counts == [0, 1, 0], (g, counts)
        k = {"legacy": 0, "multi": 1, "rect": 2}[g]
        thr = fc.thresholds(geoms[f"thr_{g}_at"])[k]
        assert out[f"thr_{g}_at_series"][0, k] == thr
        for side, way in (("below", -np.inf), ("above", np.inf)):
            thr = fc.thresholds(geoms[f"thr_{g}_{side}"])[k]
            assert np.nextafter(thr, way) == out[f"thr_{g}_{side}_series"][0, k], (g, side)
    assert [bool(out[f"moving_{s}_moving"][1]) for s in ("at", "below", "above")] == [False, False, True]
    assert out["moving_above_yaw_recon"][1] == 0.0 and out["moving_at_yaw_recon"][1] != 0.0
    # the episodes are not idle: some violate, all keep their margin
    meta["episode_counts"] = {n: [int(v) for v in out[f"ep_{n}_recheck_stored"][0, [1, 4, 7]]] for n in EPISODES}
    assert any(sum(v) > 0 for v in meta["episode_counts"].values()), meta["episode_counts"]
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    save_npz(out_path, out)
    print(out_path, os.path.getsize(out_path), "bytes;", meta["episode_counts"])


if __name__ == "__main__":
    main()
