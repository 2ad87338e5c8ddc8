#!/usr/bin/env python3
"""Open-loop prediction evaluation of the REFERENCE (build container only) -- data only.

A synthetic scene (tests/openloop_common.synthetic_scene: 30 frames, 8 ids entering and leaving) goes through the
reference's own open-loop path without its file loader: ``extract_fixed_windows`` on a ``SceneTrajectories`` built from
the array, then per window ``evaluate_window`` of examples/run_openloop_prediction.py (``ReplayPedestrianSource``,
``PedestrianObserver``, ``TrajectoryPredictor``) and ``calculate_aggregate_metrics``, and ``evaluate_scene``'s fold -- for
the constant-velocity predictor and for two generators filled from tests/sgan_common.seeded_state (no pooling: 'lstm';
pool net at every step: 'sgan').  The generators' noise is drawn here and handed over through ``user_noise``; it is stored
with the reference's raw samples (float32 as the predictor ran them, float64 from a second run of the same generator), the
per-window metrics and the scene result.  No reference code is stored.

The generator asserts, on the reference alone: at least three distinct populations; consecutive windows that differ in
population; ade_per_agent < ade somewhere; nll_eval_count > 0; floored and un-floored log p both occur; no predicted
coordinate track within a factor 10 of np.allclose's boundary in process_prediction's constant-fill rule; evaluate_scene's
own result equals the fold of the stored per-window metrics bit for bit.  meta["nll_slope"]: the largest |d log p / d q| =
|q - g| / b^2 over the un-floored entries; meta["nll_atol"] = sqrt(2) 1e-12 times it (make_prediction_scores.py's rule).
"""
import argparse
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root
sys.path.insert(0, HERE)
import openloop_common as oc  # noqa: E402
import sgan_common as sc  # noqa: E402
from make_golden_sgan import run_reference  # noqa: E402
from make_prediction_scores import log_p_survey, save_npz  # noqa: E402
from prediction_common import bound_ratio  # noqa: E402

METHODS = ("cv", "lstm", "sgan")


class NoiseFed:
    """Stands where TrajectoryPredictor keeps its generator: every forward pass takes the next noise block through
    ``user_noise`` and its absolute output is recorded."""

    def __init__(self, gen, relative_to_abs, torch):
        self.gen, self.relative_to_abs, self.torch = gen, relative_to_abs, torch
        self.queue, self.raw = [], []

    def __call__(self, obs_traj, obs_traj_rel, seq_start_end):
        z = self.torch.as_tensor(self.queue.pop(0))
        rel = self.gen(obs_traj, obs_traj_rel, seq_start_end, user_noise=z)
        self.raw.append(self.relative_to_abs(rel, obs_traj[-1]).cpu().numpy().copy())
        return rel


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
    sys.modules.setdefault("pysocialforce", types.ModuleType("pysocialforce"))
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    import torch
    from src.core.metrics import calculate_aggregate_metrics
    from src.datasets.eth_ucy_loader import SceneTrajectories, extract_fixed_windows
    from src.prediction.sgan_vendor.models import TrajectoryGenerator
    from src.prediction.sgan_vendor.utils import relative_to_abs
    from src.prediction.trajectory_predictor import TrajectoryPredictor
    spec = importlib.util.spec_from_file_location("ref_openloop", os.path.join(args.ref, "examples", "run_openloop_prediction.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    torch.set_num_threads(1)

    obs_len, pred_len, dt, S = oc.OBS_LEN, oc.PRED_LEN, oc.DT, oc.NUM_SAMPLES
    seq_len = obs_len + pred_len
    xy = oc.synthetic_scene()
    F, n_ids = xy.shape[:2]
    scene = SceneTrajectories(frames=np.arange(F) * 10, ped_ids=np.arange(n_ids),
                              by_frame=[{i: xy[t, i].copy() for i in range(n_ids) if not np.isnan(xy[t, i]).any()} for t in range(F)],
                              source="synthetic")
    windows = extract_fixed_windows(scene, seq_len=seq_len, stride=1)
    f0, off, col = oc.reference_windows(xy, seq_len)
    assert len(windows) == len(f0)
    for w, win in enumerate(windows):                               # the table names exactly the reference's windows
        assert np.array_equal(win, xy[f0[w]:f0[w] + seq_len][:, col[off[w]:off[w + 1]]])
    pops = np.diff(off)
    assert len(set(pops.tolist())) >= 3, pops
    assert np.any(pops[1:] != pops[:-1]), pops
    rows = int(off[-1])
    out = {"scene": xy, "win_frame0": f0, "ped_off": off, "row_col": col}
    meta = {"obs_len": obs_len, "pred_len": pred_len, "dt": dt, "num_samples": S, "populations": pops.tolist(), "methods": {},
            "window_keys": list(oc.WINDOW_KEYS), "model_args": {k: {**v, "noise_dim": list(v["noise_dim"])} for k, v in oc.MODEL_ARGS.items()},
            "model_seed": oc.MODEL_SEED, "model_scale": oc.MODEL_SCALE}
    slope = 0.0
    floored = free = 0
    rng = np.random.default_rng(20250219)
    for method in METHODS:
        n_samples = 1 if method == "cv" else S
        pr = TrajectoryPredictor(model_path=None, pred_len=pred_len, num_samples=n_samples, device="cpu", sgan_dt=dt, sim_dt=dt,
                                 plan_horizon=pred_len * dt, method=method)
        fed = noise = None
        if method != "cv":
            a = oc.MODEL_ARGS[method]
            state = sc.seeded_state(a, oc.MODEL_SEED[method], oc.MODEL_SCALE)
            kw = {k: a[k] for k in ("obs_len", "pred_len", "embedding_dim", "encoder_h_dim", "decoder_h_dim", "mlp_dim", "num_layers",
                                    "noise_dim", "noise_type", "noise_mix_type", "pooling_type", "pool_every_timestep", "dropout",
                                    "bottleneck_dim", "batch_norm")}
            gen = TrajectoryGenerator(**kw)
            gen.load_state_dict({k: torch.as_tensor(v).to(torch.int64 if v.dtype == np.int64 else torch.float32) for k, v in state.items()},
                                strict=True)
            gen.eval()
            fed = NoiseFed(gen, relative_to_abs, torch)
            pr.generator = fed
            noise = rng.standard_normal((S, rows, a["noise_dim"][0])).astype(np.float32)

        def feed():
            if fed is not None:
                fed.queue = [noise[s, off[w]:off[w + 1]] for w in range(len(f0)) for s in range(S)]
                fed.raw = []

        feed()
        per_window = np.zeros((len(windows), len(oc.WINDOW_KEYS)))
        tot = dict(ade=0.0, fde=0.0, apa=0.0, fpa=0.0, nll=0.0)
        traj = 0.0
        nll_n = 0
        for w, win in enumerate(windows):
            hist = ev.evaluate_window(win, pr, obs_len, dt)
            m = calculate_aggregate_metrics(hist, dt, dt, pred_len)
            per_window[w] = [m[k] for k in oc.WINDOW_KEYS]
            assert m["ade_eval_count"] == win.shape[1], (method, w, m["ade_eval_count"])
            n = m["ade_eval_count"]
            if n > 0 and not np.isnan(m["ade"]):
                tot["ade"] += m["ade"] * n; tot["fde"] += m["fde"] * n
                tot["apa"] += m["ade_per_agent"] * n; tot["fpa"] += m["fde_per_agent"] * n
                traj += n
            k = m["nll_eval_count"]
            if k > 0 and not np.isnan(m["nll"]):
                tot["nll"] += m["nll"] * k
                nll_n += k
            d = hist[obs_len - 1].predicted_distribution
            assert d.shape == (n_samples, win.shape[1], pred_len, 2), d.shape
            if method != "cv":
                truth = win[obs_len:].transpose(1, 0, 2)
                a_, b_, c_ = log_p_survey(np.asarray(d, np.float64), truth, 1)
                floored, free, slope = floored + a_, free + b_, max(slope, c_)
        mine = {"n_windows": len(windows), "n_trajectories": int(traj), "ade": tot["ade"] / traj, "fde": tot["fde"] / traj,
                "ade_per_agent": tot["apa"] / traj, "fde_per_agent": tot["fpa"] / traj, "nll": tot["nll"] / nll_n if nll_n else float("nan")}
        info = {"num_samples": n_samples}
        if method != "cv":
            raw = np.stack([np.concatenate([fed.raw[w * S + s] for w in range(len(f0))], axis=1) for s in range(S)])
            assert raw.shape == (S, pred_len, rows, 2) and raw.dtype == np.float32
            obs32 = np.concatenate([win[:obs_len] for win in windows], axis=1).astype(np.float32)
            raw64 = run_reference(TrajectoryGenerator, relative_to_abs, torch, oc.MODEL_ARGS[method], state, obs32, off, noise, torch.float64)
            e_ref = float(np.max(np.abs(raw.astype(np.float64) - raw64)))
            # process_prediction's constant fill: every source track [anchor, predictions] far from np.allclose's boundary
            worst = None
            for s in range(S):
                for r in range(rows):
                    for ax in range(2):
                        co = np.concatenate([[float(obs32[-1, r, ax])], raw[s, :, r, ax].astype(np.float64)])
                        for b in (co[0], 0.0):
                            q = bound_ratio(co, b)
                            assert not 0.1 <= q <= 10.0, (method, s, r, ax, q)
                            worst = q if worst is None or abs(math.log(q)) < abs(math.log(worst)) else worst
            steps = np.diff(np.concatenate([np.broadcast_to(obs32[-1].astype(np.float64), (S, 1) + obs32[-1].shape), raw64], axis=1), axis=1)
            info.update(e_ref=e_ref, largest_step=float(np.max(np.linalg.norm(steps, axis=-1))), closest_bound_ratio=float(worst))
            out[f"{method}_noise"], out[f"{method}_raw32"], out[f"{method}_raw64"] = noise, raw, raw64
            assert nll_n > 0, method
            assert np.any(per_window[:, 2] < per_window[:, 0]), method                    # ade_per_agent < ade somewhere
        feed()
        theirs = ev.evaluate_scene([scene], pr, obs_len, pred_len, dt, 1, None)
        for k in oc.RESULT_KEYS:                                    # bit for bit (NaN == NaN)
            assert theirs[k] == mine[k] or (np.isnan(theirs[k]) and np.isnan(mine[k])), (method, k, theirs[k], mine[k])
        out[f"{method}_windows"] = per_window
        info["result"] = {k: (int(theirs[k]) if k.startswith("n_") else float(theirs[k])) for k in oc.RESULT_KEYS}
        meta["methods"][method] = info
        print(method, info, flush=True)
    assert floored > 0 and free > 0, (floored, free)
    meta.update(log_p_floored=floored, log_p_free=free, nll_slope=slope, nll_atol=math.sqrt(2.0) * 1e-12 * slope)
    out["meta"] = np.array(json.dumps(meta))
    path = oc.FIXTURE
    os.makedirs(os.path.dirname(path), exist_ok=True)
    save_npz(path, out)
    print(f"floored {floored} free {free} nll_atol {meta['nll_atol']:.3e}; {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
