#!/usr/bin/env python3
"""Per-episode summary metrics of the REFERENCE simulator (build container only) -- SURVEY 8(f4), aggregate metrics.

``calculate_aggregate_metrics`` (src/core/metrics.py:272-320) of whole reference episodes, what the reference writes as
one row of metrics_summary.csv:

* the thirteen variants of make_closed_loop_episode.py (same scripts, same runs), for ``base`` also of the prefixes
  history[:60] and history[:100] -- what a run stopped there holds;
* new variants whose pedestrians are NOT constant-velocity (lateral weave A sin(wt + phi), A 0.3 - 0.8 m, period 3 - 6 s,
  and a speed modulation), seeds fixed here, with their tracks and resolved configurations: on straight scripted tracks
  the constant-velocity predictor's error is float32 rounding noise (base: ade 3e-06), on these it is centimetres to
  decimetres.  ``weave_short`` has a recording that ends before the episode does (the last frame is held).

The generator asserts that every new variant has ade_eval_count > 0 and ade > 1e-2 m.  Data only.
"""
import argparse
import json
import os
import sys
import types
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_closed_loop_episode import VARIANTS  # noqa: E402

PREFIXES = {"base": (60, 100)}
# weave: seed of the pedestrians' script; n_frames: recorded frames (None: the whole episode and more)
WEAVE_VARIANTS = {
    "weave0": dict(scenario="scenario_01", speed=1.0, dy=0.0, weave=21),
    "weave1": dict(scenario="scenario_02", speed=1.0, dy=0.0, weave=42),
    "weave2": dict(scenario="scenario_03", speed=1.0, dy=0.0, weave=23),
    "weave3": dict(scenario="scenario_01", speed=0.9, dy=0.6, weave=24),
    "weave_short": dict(scenario="scenario_01", speed=1.0, dy=-0.4, weave=35, n_frames=110),
}
# the order of the values in <name>_summary
KEYS = ("min_dist", "collision_count", "min_ttc", "max_jerk", "mean_jerk", "rms_jerk", "max_accel", "mean_accel", "ade",
        "fde", "ade_per_agent", "fde_per_agent", "pred_samples", "ade_eval_count", "planning_ade", "planning_fde",
        "planning_eval_count", "nll", "nll_eval_count")
INT_KEYS = ("collision_count", "pred_samples", "ade_eval_count", "planning_eval_count", "nll_eval_count")


def scripted_tracks(var, peds0, n_frames, dt):
    """[n_frames, P, 2]: straight lines (make_closed_loop_episode.py's script), or the weave on top of them."""
    peds = peds0.copy()
    peds[:, 2:4] *= var["speed"]
    peds[:, 1] += var["dy"]
    if "jitter_seed" in var and len(peds):
        rng = np.random.default_rng(var["jitter_seed"])
        peds[:, 0:2] += rng.normal(0.0, 0.7, (len(peds), 2)) + rng.uniform(-1.5, 1.5, 2)
        ang = rng.normal(0.0, 0.15, len(peds))
        vx, vy = peds[:, 2].copy(), peds[:, 3].copy()
        sc = rng.uniform(0.7, 1.4, len(peds))
        peds[:, 2] = sc * (np.cos(ang) * vx - np.sin(ang) * vy)
        peds[:, 3] = sc * (np.sin(ang) * vx + np.cos(ang) * vy)
    t = np.arange(n_frames) * dt
    if "weave" not in var:
        return peds[None, :, 0:2] + peds[None, :, 2:4] * t[:, None, None]
    rng = np.random.default_rng(var["weave"])
    P = len(peds)
    amp, period, phi = rng.uniform(0.3, 0.8, P), rng.uniform(3.0, 6.0, P), rng.uniform(0.0, 2.0 * np.pi, P)
    mod, mod_period = rng.uniform(0.0, 0.3, P), rng.uniform(4.0, 8.0, P)
    speed = np.hypot(peds[:, 2], peds[:, 3])
    normal = np.stack([-peds[:, 3], peds[:, 2]], axis=1) / np.maximum(speed, 1e-9)[:, None]
    # distance walked under the speed v (1 + mod sin(2 pi t / T)): t + mod T / (2 pi) (1 - cos(2 pi t / T))
    w_mod = 2.0 * np.pi / mod_period
    s = t[:, None] + (mod / w_mod)[None, :] * (1.0 - np.cos(w_mod[None, :] * t[:, None]))
    lateral = amp[None, :] * np.sin((2.0 * np.pi / period)[None, :] * t[:, None] + phi[None, :])
    return (peds[None, :, 0:2] + peds[None, :, 2:4] * s[:, :, None] + normal[None, :, :] * lateral[:, :, None])


def run_variant(job):
    name, var, ref = job
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

    raw = yaml.safe_load(open(os.path.join(ref, "scenarios", var["scenario"] + ".yaml")))
    peds0 = np.array(raw["ped_initial_states"], dtype=float)
    cfg = dict(raw)
    cfg.update(ped_initial_states=[], ped_groups=[], sgan_model_path=None, prediction_method="cv", visualization_enabled=False)
    cfg.update(var.get("cfg", {}))
    config = SimulationConfig(**cfg)
    sim = simmod.IntegratedSimulator(config)
    n_frames = var.get("n_frames") or int(config.total_time / config.dt) + 64
    traj = scripted_tracks(var, peds0, n_frames, config.dt)
    sim.pedestrian_sim = ReplayPedestrianSource(traj, dt=config.dt)
    sim.warmup()
    sim.run()
    h = sim.history

    def summary(hist):
        m = calculate_aggregate_metrics(hist, config.dt, prediction_dt=sim.observer.sgan_dt, prediction_steps=config.pred_len)
        assert set(m) == set(KEYS), sorted(set(m) ^ set(KEYS))
        for k in INT_KEYS:
            assert isinstance(m[k], (int, np.integer)), (k, type(m[k]))
        return np.array([float(m[k]) for k in KEYS])

    out = {name + "_summary": summary(h)}
    for n in PREFIXES.get(name, ()):
        assert n < len(h)
        out[f"{name}_summary_{n}"] = summary(h[:n])
    resolved = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(config).items()}
    resolved = {k: v for k, v in resolved.items() if isinstance(v, (int, float, str, bool, list)) or v is None}
    info = dict(steps=len(h), termination=sim.termination_reason, sgan_dt=float(sim.observer.sgan_dt),
                pred_len=int(config.pred_len), scenario=var["scenario"])
    if "weave" in var:
        out[name + "_ped_traj"] = traj
        info.update(config=resolved, ego_radius=float(sim.ego_radius), ped_radius=float(sim.ped_radius), n_frames=int(n_frames))
        s = dict(zip(KEYS, out[name + "_summary"]))
        assert s["ade_eval_count"] > 0 and s["ade"] > 1e-2, (name, s)
    return name, out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference simulator")
    ap.add_argument("--jobs", type=int, default=1)
    args = ap.parse_args()
    jobs = [(n, v, args.ref) for n, v in list(VARIANTS.items()) + list(WEAVE_VARIANTS.items())]
    out, meta = {}, {"keys": list(KEYS), "int_keys": list(INT_KEYS), "variants": {}, "weave": list(WEAVE_VARIANTS),
                     "prefixes": {k: list(v) for k, v in PREFIXES.items()}}
    with ProcessPoolExecutor(max_workers=max(1, args.jobs)) as pool:
        for name, arrays, info in pool.map(run_variant, jobs):
            out.update(arrays)
            meta["variants"][name] = info
            s = dict(zip(KEYS, arrays[name + "_summary"]))
            print(name, info["steps"], info["termination"], f"ade {s['ade']:.3e} ({int(s['ade_eval_count'])})",
                  f"planning_ade {s['planning_ade']:.3e} ({int(s['planning_eval_count'])})", flush=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "closed_loop", "reference_summary_episodes.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
