#!/usr/bin/env python3
"""Crowds of 33, 64, 65 and 257 pedestrians through the REFERENCE simulator (build container only) -- SURVEY 8(f4).

The recordings of tests/loop_crowds_common.py (``slot_tracks()``: rebuilt from the seed there, not stored) replayed
through the reference's own ReplayPedestrianSource on scenario_01 (method cv), ``IntegratedSimulator.run(n_steps)`` for
n_dense + 15 steps -- long enough for the summary ring of the resident loop to wrap.  Recorded per step what
make_closed_loop_episode.py records (same key layout, variants ``p33`` ...), plus ``<name>_summary``:
``calculate_aggregate_metrics`` of the run in make_closed_loop_summary.py's key order.  Data only.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_closed_loop_episode import STATES  # noqa: E402
from make_closed_loop_summary import INT_KEYS, KEYS  # noqa: E402


def run_slot(job):
    P, steps, ref = job
    import loop_crowds_common as lc
    lg = types.ModuleType("loguru")

    class _Logger:
        def __getattr__(self, n):
            return lambda *a, **k: None

    lg.logger = _Logger()
    sys.modules["loguru"] = lg
    sys.modules["pysocialforce"] = types.ModuleType("pysocialforce")
    sys.path.insert(0, ref)
    os.chdir(ref)
    from src.config import SimulationConfig
    import src.simulation.integrated_simulator as simmod
    from src.simulation.replay_source import ReplayPedestrianSource
    from src.core.metrics import calculate_aggregate_metrics

    raw = yaml.safe_load(open(os.path.join(ref, "scenarios", "scenario_01.yaml")))
    cfg = dict(raw)
    cfg.update(ped_initial_states=[], ped_groups=[], sgan_model_path=None, prediction_method="cv", visualization_enabled=False)
    config = SimulationConfig(**cfg)
    sim = simmod.IntegratedSimulator(config)
    traj = lc.slot_tracks()[lc.SLOT_COUNTS.index(P)]
    assert traj.shape[1] == P
    sim.pedestrian_sim = ReplayPedestrianSource(traj, dt=config.dt)
    t0 = time.time()
    sim.warmup()
    sim.run(steps)
    wall = time.time() - t0
    h = sim.history
    n = len(h)
    with tempfile.TemporaryDirectory() as td:
        sim.visualize = lambda *a, **k: None
        try:
            sim.save_results(td)
        except Exception as e:                           # plotting / metrics extras are not part of the fixture
            print("save_results:", type(e).__name__, e)
        z = np.load(os.path.join(td, "trajectory.npz"), allow_pickle=True)
        keys = {k: [str(z[k].dtype), list(z[k].shape)] for k in z.files}
    L = 64
    px = np.full((n, L), np.nan); py = np.full((n, L), np.nan)
    plen = np.zeros(n, np.int32)
    for i, r in enumerate(h):
        if r.planned_path is not None:
            m = len(r.planned_path.x)
            plen[i] = m
            px[i, :m] = r.planned_path.x; py[i, :m] = r.planned_path.y
    pre = f"p{P}_"
    out = {}
    out[pre + "times"] = np.array([r.time for r in h])
    out[pre + "ego"] = np.array([[r.ego_state.x, r.ego_state.y, r.ego_state.yaw, r.ego_state.v, r.ego_state.a,
                                  r.ego_state.jerk] for r in h])
    out[pre + "state"] = np.array([STATES[r.ego_state.state.name] for r in h], dtype=np.int32)
    out[pre + "metrics"] = np.array([[r.metrics.get("min_distance", np.inf), r.metrics.get("ttc", np.inf),
                                      r.metrics.get("clearance", np.inf), r.metrics.get("clearance_ahead", np.inf),
                                      float(r.metrics.get("collision", False)),
                                      r.metrics.get("n_collision_rejected", -1)] for r in h])
    out[pre + "planned_cost"] = np.array([r.planned_path.cost if r.planned_path is not None else np.inf for r in h])
    out[pre + "planned_len"] = plen
    out[pre + "planned_x"] = px
    out[pre + "planned_y"] = py
    out[pre + "pred_shape"] = np.array([list(r.predicted_trajectories.shape) if r.predicted_trajectories is not None
                                        else [0, 0, 0] for r in h], dtype=np.int32)
    out[pre + "pred_first"] = np.array([r.predicted_trajectories[0, :3].ravel() if r.predicted_trajectories is not None
                                        else np.full(6, np.nan) for r in h])
    m = calculate_aggregate_metrics(h, config.dt, prediction_dt=sim.observer.sgan_dt, prediction_steps=config.pred_len)
    assert set(m) == set(KEYS), sorted(set(m) ^ set(KEYS))
    out[pre + "summary"] = np.array([float(m[k]) for k in KEYS])
    resolved = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(config).items()}
    resolved = {k: v for k, v in resolved.items() if isinstance(v, (int, float, str, bool, list)) or v is None}
    info = dict(steps=n, termination=sim.termination_reason, npz_keys=keys, config=resolved, n_peds=int(P),
                n_frames=int(len(traj)), ego_radius=float(sim.ego_radius), ped_radius=float(sim.ped_radius),
                sgan_dt=float(sim.observer.sgan_dt), pred_len=int(config.pred_len), scenario="scenario_01",
                reference_seconds=round(wall, 1))
    return f"p{P}", out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference simulator")
    ap.add_argument("--steps", type=int, required=True, help="lock steps: the resampler's n_dense + 15")
    ap.add_argument("--jobs", type=int, default=1)
    args = ap.parse_args()
    import loop_crowds_common as lc
    jobs = [(P, args.steps, args.ref) for P in lc.REFERENCE_SLOTS]
    out, meta = {}, {"keys": list(KEYS), "int_keys": list(INT_KEYS), "variants": {}, "states": STATES, "steps": args.steps,
                     "track_seed": lc.TRACK_SEED}
    with ProcessPoolExecutor(max_workers=max(1, args.jobs)) as pool:
        for name, arrays, info in pool.map(run_slot, jobs):
            out.update(arrays)
            meta["variants"][name] = info
            s = dict(zip(KEYS, arrays[name + "_summary"]))
            print(name, info["steps"], info["termination"], f"{info['reference_seconds']} s",
                  f"ade {s['ade']:.3e} ({int(s['ade_eval_count'])})",
                  f"planning_ade {s['planning_ade']:.3e} ({int(s['planning_eval_count'])})", flush=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "closed_loop", "reference_crowd_episodes.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
