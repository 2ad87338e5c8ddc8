#!/usr/bin/env python3
"""Golden vectors for Social-GAN sample generation (fot_sgan_sample); build container only.

Imports the REFERENCE TrajectoryGenerator read-only, fills its state dict from NumPy (tests/sgan_common.seeded_state: the
tests rebuild the weights from the seed, the fixture carries none), and runs forward + relative_to_abs with user_noise once
per sample in float32 and again in float64 (torch.set_default_dtype: the model creates its zero states with the default
dtype).  Writes tests/golden/sgan/cases.npz -- per case the descriptor and seed (meta), obs, ped_off, the noise and the
absolute outputs of both runs; no reference code.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sgan_common as sc  # noqa: E402


def run_reference(TrajectoryGenerator, relative_to_abs, torch, a, state, obs, off, noise, dtype):
    torch.set_default_dtype(dtype)
    try:
        kw = {k: a[k] for k in ("obs_len", "pred_len", "embedding_dim", "encoder_h_dim", "decoder_h_dim", "mlp_dim", "num_layers",
                                "noise_dim", "noise_type", "noise_mix_type", "pooling_type", "pool_every_timestep", "dropout",
                                "bottleneck_dim", "batch_norm")}
        gen = TrajectoryGenerator(**kw)
        gen.load_state_dict({k: torch.as_tensor(v).to(torch.int64 if v.dtype == np.int64 else dtype) for k, v in state.items()},
                            strict=True)
        gen.eval()
        obs_t = torch.as_tensor(obs).to(dtype)
        rel_t = torch.zeros_like(obs_t)
        rel_t[1:] = obs_t[1:] - obs_t[:-1]                            # observer.py:126-135
        scenes = [(int(lo), int(hi)) for lo, hi in zip(off[:-1], off[1:]) if hi > lo]   # (the observer hands over no empty scene)
        kept = [i for i, (lo, hi) in enumerate(zip(off[:-1], off[1:])) if hi > lo]
        sse = torch.as_tensor(scenes, dtype=torch.int64)
        out = []
        with torch.no_grad():
            for s in range(noise.shape[0]):
                z = torch.as_tensor(noise[s]).to(dtype)
                if a["noise_mix_type"] == "global":
                    z = z[kept]
                rel = gen(obs_t, rel_t, sse, user_noise=z if a["noise_dim"][0] else None)
                out.append(relative_to_abs(rel, obs_t[-1]).numpy())
        return np.stack(out, axis=0)
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import torch
    from src.prediction.sgan_vendor.models import TrajectoryGenerator
    from src.prediction.sgan_vendor.utils import relative_to_abs

    torch.set_num_threads(1)
    out, meta = {}, {}
    for name, (dims, pooling, every, mix, bn, scenes, S, scale) in sc.CASES.items():
        a = sc.case_args(name)
        seed = sc.case_seed(name)
        state = sc.seeded_state(a, seed, scale)
        obs, off, noise = sc.case_inputs(name)
        r32 = run_reference(TrajectoryGenerator, relative_to_abs, torch, a, state, obs, off, noise, torch.float32)
        r64 = run_reference(TrajectoryGenerator, relative_to_abs, torch, a, state, obs, off, noise, torch.float64)
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == (S, sc.PRED_LEN, int(off[-1]), 2)
        steps = np.diff(np.concatenate([np.broadcast_to(obs[-1].astype(np.float64), (S, 1) + obs[-1].shape), r64], axis=1), axis=1)
        move = float(np.max(np.linalg.norm(steps, axis=-1)))
        e_ref = float(np.max(np.abs(r32 - r64)))
        print(f"{name:26s} largest step {move:6.3f} m   e_ref {e_ref:.3e}   bound {sc.accuracy_bound(r32, r64):.3e}")
        assert 0.3 <= move <= 2.0, f"{name}: the trajectories must move 0.3 .. 2 m per step, got {move}"
        assert np.isfinite(r64).all() and e_ref > 0.0
        meta[name] = dict(args={**a, "noise_dim": list(a["noise_dim"])}, seed=seed, scale=scale, scenes=scenes, S=S,
                          largest_step=move, e_ref=e_ref)
        for k, v in (("obs", obs), ("ped_off", off), ("noise", noise), ("out32", r32), ("out64", r64)):
            out[f"{name}/{k}"] = v
    out["meta"] = np.asarray(json.dumps(meta))
    os.makedirs(os.path.dirname(sc.FIXTURE), exist_ok=True)
    np.savez_compressed(sc.FIXTURE, **out)
    print("wrote", sc.FIXTURE, os.path.getsize(sc.FIXTURE), "bytes")
    assert os.path.getsize(sc.FIXTURE) < 1_000_000


if __name__ == "__main__":
    main()
