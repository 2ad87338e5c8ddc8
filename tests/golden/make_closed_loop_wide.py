#!/usr/bin/env python3
"""Distribution-aware closed-loop episodes of the REFERENCE simulator against distributions of MORE THAN 64 samples
(build container only).

As make_closed_loop_distribution.py: IntegratedSimulator.run() on scenario_01 with `distribution_aware_planning`, the one
Social-GAN forward pass replaced by a scripted sample generator (tests/wide_loop_common.py::wide_raw_sample, whose fan
stays narrow at large S) that still runs through the reference's own process_prediction, predict_single_best, prepend
logic, planner and fail-safe loop; pedestrians are replayed scripted tracks (ReplayPedestrianSource).  Two variants:

  s100_eps01   S = 100, chance_epsilon = 0.01: a budget of floor(0.01 * 100) = exactly ONE colliding sample
  s130_eps0    S = 130, chance_epsilon = 0: robust, no sample may collide

The reference walks the samples in Python, so total_time is shortened until a variant runs in minutes.  The generator
ASSERTS that the budget decides something: every variant has a step with n_collision_rejected > 0 and a state escalation,
and the eps = 0.01 variant has a step whose selected path differs from what the same planner selects on the same inputs
with eps = 0 (every plan() call of that variant is made twice: first with eps = 0 on a copy of the planner's running
state, then for real).  Data only.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: wide_loop_common
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root
STATES = {"NORMAL": 0, "CAUTION": 1, "EMERGENCY": 2}
VARIANTS = {"s100_eps01": dict(n_samples=100, chance_epsilon=0.01, speed=1.0, dy=0.0, total_time=9.0),
            "s130_eps0": dict(n_samples=130, chance_epsilon=0.0, speed=1.15, dy=0.5, total_time=9.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default=None, help="one variant (a trial run: nothing is written)")
    ap.add_argument("--total-time", type=float, default=None, help="override the variants' total_time (trial runs)")
    args = ap.parse_args()
    lg = types.ModuleType("loguru")

    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None

    lg.logger = _Logger()
    sys.modules["loguru"] = lg
    sys.modules["pysocialforce"] = types.ModuleType("pysocialforce")
    from wide_loop_common import wide_raw_sample
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    from src.config import SimulationConfig
    import src.simulation.integrated_simulator as simmod
    from src.simulation.replay_source import ReplayPedestrianSource

    out, meta = {}, {"variants": {}, "states": STATES}
    for name, var in VARIANTS.items():
        if args.only and name != args.only:
            continue
        t_start = time.time()
        raw = yaml.safe_load(open(os.path.join(args.ref, "scenarios", "scenario_01.yaml")))
        peds0 = np.array(raw["ped_initial_states"], dtype=float)
        cfg = dict(raw)
        cfg.update(ped_initial_states=[], ped_groups=[], sgan_model_path=None, prediction_method="cv",
                   visualization_enabled=False, chance_epsilon=var["chance_epsilon"],
                   total_time=args.total_time if args.total_time else var["total_time"])
        config = SimulationConfig(**cfg)
        sim = simmod.IntegratedSimulator(config)
        S = var["n_samples"]
        sim.distribution_aware_planning = True
        pr = sim.predictor
        pr.num_samples = S
        calls = {"k": 0}

        def scripted_predict(obs_traj, obs_traj_rel, seq_start_end, staleness=0.0, pr=pr, calls=calls, S=S):
            k = calls["k"] % S
            calls["k"] += 1
            obs = obs_traj.cpu().numpy().astype(np.float64)      # the observer's float32 tensors, widened
            raw_k = wide_raw_sample(obs[-1], obs[-2], k, S, pr.pred_len, pr.sgan_dt)
            return pr.process_prediction(raw_k, anchor_pos=obs[-1], staleness=staleness)

        pr.predict = scripted_predict
        # the eps > 0 variant: what would eps = 0 have selected on the same inputs?  Asked first, on the planner's running
        # state (the nearest-point window and the last curvature), which is put back before the real call.
        planner = sim.planner
        differs = {"steps": 0, "calls": 0}
        if var["chance_epsilon"] > 0.0:
            real_plan = planner.plan

            def plan_twice(*a, planner=planner, real_plan=real_plan, differs=differs, **kw):
                keep_kappa = planner._last_kappa
                had_prev = hasattr(planner.converter, "_prev_s")
                keep_prev = getattr(planner.converter, "_prev_s", None)
                eps = planner.chance_epsilon
                planner.chance_epsilon = 0.0
                robust = real_plan(*a, **kw)
                planner.chance_epsilon = eps
                planner._last_kappa = keep_kappa
                if had_prev:
                    planner.converter._prev_s = keep_prev
                elif hasattr(planner.converter, "_prev_s"):
                    del planner.converter._prev_s
                chosen = real_plan(*a, **kw)
                differs["calls"] += 1
                if chosen is not None and (robust is None or len(robust.x) != len(chosen.x) or
                                           not np.array_equal(np.asarray(robust.x), np.asarray(chosen.x)) or
                                           not np.array_equal(np.asarray(robust.y), np.asarray(chosen.y))):
                    differs["steps"] += 1
                return chosen

            planner.plan = plan_twice
        peds = peds0.copy()
        peds[:, 2:4] *= var["speed"]
        peds[:, 1] += var["dy"]
        n_frames = int(config.total_time / config.dt) + 64
        t = np.arange(n_frames) * config.dt
        traj = peds[None, :, 0:2] + peds[None, :, 2:4] * t[:, None, None]
        sim.pedestrian_sim = ReplayPedestrianSource(traj, dt=config.dt)
        sim.warmup()
        sim.run()
        h = sim.history
        n = len(h)
        L = 64
        px = np.full((n, L), np.nan); py = np.full((n, L), np.nan)
        plen = np.zeros(n, np.int32)
        for i, r in enumerate(h):
            if r.planned_path is not None:
                m = len(r.planned_path.x)
                plen[i] = m
                px[i, :m] = r.planned_path.x; py[i, :m] = r.planned_path.y
        pre = f"{name}_"
        out[pre + "ped_traj"] = traj
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
        resolved = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(config).items()}
        resolved = {k: v for k, v in resolved.items() if isinstance(v, (int, float, str, bool, list)) or v is None}
        resolved["distribution_aware_planning"] = True
        resolved["num_samples"] = S
        n_rejected = int((out[pre + "metrics"][:, 5] > 0).sum())
        n_escalations = int((np.diff(out[pre + "state"]) > 0).sum())
        meta["variants"][name] = dict(steps=n, termination=sim.termination_reason, config=resolved,
                                      ego_radius=float(sim.ego_radius), ped_radius=float(sim.ped_radius),
                                      n_static_points=int(len(sim.static_obstacle_points)), predict_calls=calls["k"],
                                      steps_with_rejections=n_rejected, state_escalations=n_escalations,
                                      budget_decided_calls=differs["steps"], **var)
        print(name, n, "steps,", sim.termination_reason, "states", np.bincount(out[pre + "state"], minlength=3).tolist(),
              "no path", int((plen == 0).sum()), "predict calls", calls["k"], "steps with rejections", n_rejected,
              "escalations", n_escalations, "plan calls the budget decided", differs["steps"], "of", differs["calls"],
              f"({time.time() - t_start:.0f} s)", flush=True)
        # otherwise the budget never decides and the fixture proves nothing: move the pedestrians (speed, dy) until it does
        assert n_rejected > 0, f"{name}: no step with n_collision_rejected > 0"
        assert n_escalations > 0, f"{name}: no state escalation"
        if var["chance_epsilon"] > 0.0:
            assert differs["steps"] > 0, f"{name}: the budget of one sample never changed the selected path"
    if args.only or args.total_time:
        print("trial run: nothing written")
        return
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "closed_loop", "reference_wide_episodes.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
