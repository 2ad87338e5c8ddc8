#!/usr/bin/env python3
"""Prediction scores of the REFERENCE (build container only): best-of-N ADE / FDE and KDE-NLL -- data only.

(a) Unit origins: hand-made histories of exactly stride * E + 1 entries, so that only origin 0 is eligible, passed to the
    reference's ``_standard_ade_fde_details`` and ``_kde_nll_details`` (src/core/metrics.py:31-176) with small
    ``prediction_dt`` / ``prediction_steps``.  Inputs (dense samples [S, P, T, 2], truth [P, E, 2]) and the reference's
    answers are stored.  The classes are the smallest shapes at which a scoring kernel can go wrong (UNITS below).
(b) Whole episodes: the three distribution episodes of make_closed_loop_distribution.py run again, and two more on
    weaving tracks (make_closed_loop_summary.py's script) so that the truth does not lie inside the sample fan; the
    reference's own ``calculate_aggregate_metrics`` dictionary of each is stored with the tracks and the configuration.

The generator asserts: nll_eval_count > 0 in every episode but s4_eps0 -- that reference run ends in a collision after 45
steps, before the first 48-step horizon completes, so its dictionary is the reference's NaN / 0 answer, kept as the
"nothing counted" case --; ade_per_agent < ade strictly in at least one; floored and
un-floored log p both occur.  meta["nll_atol"]: sqrt(2) 1e-12 (the distance of the loop's predictions from the
reference's, tests/summary_common.py) times the largest |d log p / d q| = |q - g| / b^2 over the un-floored entries of
everything stored -- the absolute tolerance of ``nll`` against these answers.
"""
import argparse
import io
import json
import math
import os
import sys
import types
import zipfile
from types import SimpleNamespace

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: closed_loop_common, pred_scores_common
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root
sys.path.insert(0, HERE)
from make_closed_loop_distribution import VARIANTS as DIST_VARIANTS  # noqa: E402
from make_closed_loop_summary import scripted_tracks  # noqa: E402

WEAVE_VARIANTS = {"weave_s5": dict(n_samples=5, chance_epsilon=0.2, speed=1.0, dy=0.0, weave=21),
                  "weave_s4": dict(n_samples=4, chance_epsilon=0.0, speed=0.9, dy=0.6, weave=24)}
NO_HORIZON = ("s4_eps0",)         # the reference episode collides after 45 steps, before a 48-step horizon completes
KEYS = ("ade", "fde", "ade_per_agent", "fde_per_agent", "pred_samples", "ade_eval_count", "nll", "nll_eval_count")
DT = 0.1


def fan(rng, S, P, T, spread, centre=0.0):
    """Random-walk tracks with S samples scattered around them."""
    base = centre + rng.uniform(-20.0, 20.0, (1, P, 1, 2)) + np.cumsum(rng.normal(0.0, 0.15, (1, P, T, 2)), axis=2)
    return base + rng.normal(0.0, spread, (S, P, T, 2))


def truth_near(rng, dense, stride, E, noise):
    idx = stride * np.arange(1, E + 1) - 1
    return dense.mean(axis=0)[:, idx] + rng.normal(0.0, noise, (dense.shape[1], E, 2))


def units():
    """name -> (dense, truth, stride)"""
    rng = np.random.default_rng(20240607)
    out = {}

    def plain(name, S, P, E, stride, T=None, spread=0.3, noise=0.4, centre=0.0):
        T = stride * E if T is None else T
        d = fan(rng, S, P, T, spread, centre)
        out[name] = (d, truth_near(rng, d, stride, E, noise), stride)

    plain("s1", 1, 3, 2, 4)                                       # no NLL, per-agent == scene
    plain("s2", 2, 3, 2, 4)
    plain("s64", 64, 3, 2, 4)
    plain("p1", 4, 1, 2, 4)
    plain("p33", 4, 33, 2, 4)
    plain("p65", 3, 65, 2, 4)                                     # more than one wave of pedestrians
    plain("p300_e1", 2, 300, 1, 1)                                # more pedestrians than lanes of a workgroup
    plain("p90_e12", 2, 90, 12, 1)                                # 1080 (p, j) pairs: more than one LDS tile
    plain("e1_stride1", 4, 3, 1, 1)
    plain("e12_stride4", 4, 3, 12, 4, T=48)
    plain("tail", 5, 7, 3, 3, T=12)                               # a dense track longer than the horizon
    plain("offset100", 8, 3, 2, 4, spread=0.02, noise=0.03, centre=100.0)      # a one-pass variance loses these
    d = fan(rng, 1, 3, 8, 0.0)
    d = np.repeat(d, 4, axis=0)
    out["identical_s4"] = (d, truth_near(rng, d, 4, 2, 0.4), 4)   # the NLL is skipped
    d = d.copy()
    d[2, 1, 7, 0] += 0.25                                         # ... identical on every (p, j) but one
    out["identical_but_one"] = (d, truth_near(rng, d, 4, 2, 0.1), 4)
    d = fan(rng, 6, 4, 8, 0.5)
    d[:, :2] = d[:1, :2] + rng.normal(0.0, 1e-3, (6, 2, 8, 2))    # two pedestrians under the bandwidth floor
    out["bw_floor_mixed"] = (d, truth_near(rng, d, 4, 2, 0.05), 4)
    d = fan(rng, 6, 4, 8, 0.03)
    t = truth_near(rng, d, 4, 2, 0.02)
    t[:2] += (3.0, -4.0)                                          # metres away from tight samples: log p at the floor
    out["logp_floor_mixed"] = (d, t, 4)
    base = fan(rng, 1, 2, 8, 0.0)[0]                              # scene-level and per-agent picks differ
    d = np.stack([base, base])
    d[0, 1] += (0.9, 0.0)
    d[1, 0] += (0.0, 0.7)
    out["picks_differ"] = (d, base[:, [3, 7]].copy(), 4)
    base = fan(rng, 1, 1, 8, 0.0)[0]                              # minADE and minFDE choose different samples
    d = np.stack([base, base])
    d[0, 0, 7] += (1.0, 0.0)
    d[1, 0, 3] += (1.2, 0.0)
    d[1, 0, 7] += (0.0, 0.5)
    out["ade_fde_differ"] = (d, base[:, [3, 7]].copy(), 4)
    return out


def reference_unit(metrics, dense, truth, stride):
    E = truth.shape[1]
    L = stride * E + 1
    hist = [SimpleNamespace(predicted_distribution=None, predicted_trajectories=None,
                            ped_state=SimpleNamespace(positions=np.zeros((dense.shape[1], 2)))) for _ in range(L)]
    hist[0].predicted_distribution = dense
    for j in range(1, E + 1):
        hist[stride * j].ped_state.positions = truth[:, j - 1]
    a = metrics._standard_ade_fde_details(hist, DT, stride * DT, E)
    n = metrics._kde_nll_details(hist, DT, stride * DT, E)
    return dict(zip(KEYS, [float(a[0]), float(a[1]), float(a[2]), float(a[3]), int(a[4]), int(a[5]), float(n[0]), int(n[1])]))


def log_p_survey(dense, truth, stride):
    """(floored entries, un-floored entries, largest |q - g| / b^2 over the un-floored ones) of one origin."""
    from pred_scores_common import LOG_P_FLOOR, log_p_terms
    E = truth.shape[1]
    q = dense[:, :, stride * np.arange(1, E + 1) - 1]
    if q.shape[0] < 2 or not np.any(np.ptp(q, axis=0) > 0):
        return 0, 0, 0.0
    lp, bw = log_p_terms(q, truth)
    free = lp > LOG_P_FLOOR
    slope = (np.abs(q - truth[None]) / bw[None] ** 2).max(axis=(0, 3))
    return int((~free).sum()), int(free.sum()), float(slope[free].max()) if free.any() else 0.0


def run_episode(name, var, ref):
    from closed_loop_common import scripted_raw_sample
    from src.config import SimulationConfig
    import src.simulation.integrated_simulator as simmod
    from src.simulation.replay_source import ReplayPedestrianSource
    from src.core.metrics import calculate_aggregate_metrics

    raw = yaml.safe_load(open(os.path.join(ref, "scenarios", "scenario_01.yaml")))
    peds0 = np.array(raw["ped_initial_states"], dtype=float)
    cfg = dict(raw)
    cfg.update(ped_initial_states=[], ped_groups=[], sgan_model_path=None, prediction_method="cv",
               visualization_enabled=False, chance_epsilon=var["chance_epsilon"])
    config = SimulationConfig(**cfg)
    sim = simmod.IntegratedSimulator(config)
    S = var["n_samples"]
    aware = var.get("aware", True)
    sim.distribution_aware_planning = aware
    pr = sim.predictor
    pr.num_samples = S
    calls = {"k": 0}

    def scripted_predict(obs_traj, obs_traj_rel, seq_start_end, staleness=0.0):
        k = calls["k"] % S
        calls["k"] += 1
        obs = obs_traj.cpu().numpy().astype(np.float64)
        return pr.process_prediction(scripted_raw_sample(obs[-1], obs[-2], k, S, pr.pred_len, pr.sgan_dt),
                                     anchor_pos=obs[-1], staleness=staleness)

    pr.predict = scripted_predict
    n_frames = int(config.total_time / config.dt) + 64
    traj = scripted_tracks(var, peds0, n_frames, config.dt)
    sim.pedestrian_sim = ReplayPedestrianSource(traj, dt=config.dt)
    sim.warmup()
    sim.run()
    h = sim.history
    m = calculate_aggregate_metrics(h, config.dt, prediction_dt=sim.observer.sgan_dt, prediction_steps=config.pred_len)
    stride, E = int(round(sim.observer.sgan_dt / config.dt)), int(config.pred_len)
    floored = free = 0
    slope = 0.0
    for i, r in enumerate(h):
        d = r.predicted_distribution
        if d is None or d.size == 0 or d.shape[2] <= stride * E - 1 or i + stride * E >= len(h):
            continue
        truth = np.stack([h[i + stride * j].ped_state.positions for j in range(1, E + 1)], axis=1)
        a, b, c = log_p_survey(np.asarray(d, np.float64), truth, stride)
        floored, free, slope = floored + a, free + b, max(slope, c)
    resolved = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(config).items()}
    resolved = {k: v for k, v in resolved.items() if isinstance(v, (int, float, str, bool, list)) or v is None}
    resolved["distribution_aware_planning"] = aware
    resolved["num_samples"] = S
    info = dict(steps=len(h), termination=sim.termination_reason, config=resolved, sgan_dt=float(sim.observer.sgan_dt),
                pred_len=E, reference={k: (int(m[k]) if k in ("pred_samples", "ade_eval_count", "nll_eval_count")
                                           else float(m[k])) for k in KEYS},
                log_p_floored=floored, log_p_free=free, nll_slope=slope,
                **{k: v for k, v in var.items() if k != "weave"})
    return traj, info


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    lg = types.ModuleType("loguru")

    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None

    lg.logger = _Logger()
    sys.modules["loguru"] = lg
    sys.modules["pysocialforce"] = types.ModuleType("pysocialforce")
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    from src.core import metrics

    out, meta = {}, {"keys": list(KEYS), "units": {}, "episodes": {}}
    slope = 0.0
    floored = free = 0
    for name, (dense, truth, stride) in units().items():
        ref = reference_unit(metrics, dense, truth, stride)
        a, b, c = log_p_survey(dense, truth, stride)
        floored, free, slope = floored + a, free + b, max(slope, c)
        out[f"u_{name}_dense"], out[f"u_{name}_truth"] = dense, truth
        meta["units"][name] = dict(stride=stride, reference=ref, log_p_floored=a, log_p_free=b)
        print(name, dense.shape, "E", truth.shape[1], "stride", stride, {k: (round(v, 6) if isinstance(v, float) else v)
                                                                         for k, v in ref.items()}, "floored", a, "free", b)
    u = meta["units"]
    assert u["s1"]["reference"]["nll_eval_count"] == 0 and u["s1"]["reference"]["ade"] == u["s1"]["reference"]["ade_per_agent"]
    assert u["identical_s4"]["reference"]["nll_eval_count"] == 0 and u["identical_but_one"]["reference"]["nll_eval_count"] == 6
    assert u["picks_differ"]["reference"]["ade_per_agent"] < u["picks_differ"]["reference"]["ade"]
    d, t, s_ = units()["ade_fde_differ"]
    disp = np.linalg.norm(d[:, :, [3, 7]] - t[None], axis=3)
    assert np.argmin(disp.mean(axis=(1, 2))) != np.argmin(disp[:, :, -1].mean(axis=1))
    assert u["logp_floor_mixed"]["log_p_floored"] > 0 and u["logp_floor_mixed"]["log_p_free"] > 0
    d, t, s_ = units()["bw_floor_mixed"]
    sd = d[:, :, [3, 7]].std(axis=0, ddof=1) * 6 ** (-1.0 / 6.0)
    assert (sd < 0.05).any() and (sd > 0.05).any()

    for name, var in list(DIST_VARIANTS.items()) + list(WEAVE_VARIANTS.items()):
        traj, info = run_episode(name, var, args.ref)
        out[f"{name}_ped_traj"] = traj
        meta["episodes"][name] = info
        r = info["reference"]
        print(name, info["steps"], info["termination"], {k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items()},
              "floored", info["log_p_floored"], "free", info["log_p_free"], "slope", round(info["nll_slope"], 3), flush=True)
        if name in NO_HORIZON:                                      # (ends before stride * E + 1 steps: nothing counts)
            assert info["steps"] <= int(round(info["sgan_dt"] / DT)) * info["pred_len"] and r["ade_eval_count"] == 0, name
        else:
            assert r["nll_eval_count"] > 0, name
        slope = max(slope, info["nll_slope"])
    eps = meta["episodes"].values()
    assert any(e["reference"]["ade_per_agent"] < e["reference"]["ade"] for e in eps)
    assert sum(e["log_p_floored"] for e in eps) > 0 and sum(e["log_p_free"] for e in eps) > 0
    meta["nll_slope"] = slope
    meta["nll_atol"] = math.sqrt(2.0) * 1e-12 * slope
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "prediction_scores", "cases.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    save_npz(path, out)
    print(f"nll_atol {meta['nll_atol']:.3e}; {os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
