#!/usr/bin/env python3
"""Golden vectors for Social-GAN sample generation (fot_sgan_sample); build container only.

Imports the REFERENCE TrajectoryGenerator read-only, fills its state dict from NumPy (tests/sgan_common.seeded_state: the
tests rebuild the weights from the seed, the fixture carries none), and runs forward + relative_to_abs with user_noise once
per sample in float32 and again in float64 (torch.set_default_dtype: the model creates its zero states with the default
dtype).  Writes tests/golden/sgan/cases.npz -- per case the descriptor and seed (meta), obs, ped_off, the noise and the
absolute outputs of both runs; no reference code.

    make_golden_sgan.py [--only cases]   sgan_common.CASES      -> tests/golden/sgan/cases.npz (the default)
    make_golden_sgan.py --only edges     sgan_common.EDGE_CASES -> tests/golden/sgan/edges.npz
    make_golden_sgan.py --only edges --probe    nothing is written: per edge case, the largest step at each weight scale
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


SCALES = (1.5, 2.0, 2.5, 3.0)


def run_case(ref, name, scale):
    """(arrays of the case, its meta entry) at a weight scale; the reference alone is held to the conditions."""
    TrajectoryGenerator, relative_to_abs, torch = ref
    c = sc.case(name)
    a = sc.case_args(name)
    seed = sc.case_seed(name)
    state = sc.seeded_state(a, seed, scale)
    obs, off, noise = sc.case_inputs(name)
    r32 = run_reference(TrajectoryGenerator, relative_to_abs, torch, a, state, obs, off, noise, torch.float32)
    r64 = run_reference(TrajectoryGenerator, relative_to_abs, torch, a, state, obs, off, noise, torch.float64)
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == (c["S"], a["pred_len"], int(off[-1]), 2)
    steps = np.diff(np.concatenate([np.broadcast_to(obs[-1].astype(np.float64), (c["S"], 1) + obs[-1].shape), r64], axis=1), axis=1)
    move = float(np.max(np.linalg.norm(steps, axis=-1)))
    e_ref = float(np.max(np.abs(r32 - r64)))
    print(f"{name:26s} scale {scale:3.1f} largest step {move:6.3f} m   e_ref {e_ref:.3e}   bound {sc.accuracy_bound(r32, r64):.3e}",
          flush=True)
    meta = dict(args={**a, "noise_dim": list(a["noise_dim"])}, seed=seed, scale=scale, scenes=c["scenes"], S=c["S"],
                largest_step=move, e_ref=e_ref)
    arrays = {f"{name}/{k}": v for k, v in (("obs", obs), ("ped_off", off), ("noise", noise), ("out32", r32), ("out64", r64))}
    why = []
    if not np.isfinite(r64).all():
        why.append("the float64 output is not finite")
    if not e_ref > 0.0:
        why.append(f"e_ref must be positive, got {e_ref}")
    if not 0.3 <= move <= 2.0:
        why.append(f"the trajectories must move 0.3 .. 2 m per step, got {move}")
    return arrays, meta, why


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", choices=("cases", "edges"), default="cases")
    ap.add_argument("--probe", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import torch
    from src.prediction.sgan_vendor.models import TrajectoryGenerator
    from src.prediction.sgan_vendor.utils import relative_to_abs

    torch.set_num_threads(1)
    ref = (TrajectoryGenerator, relative_to_abs, torch)
    table, path = (sc.CASES, sc.FIXTURE) if args.only == "cases" else (sc.EDGE_CASES, sc.EDGE_FIXTURE)
    if args.probe:
        for name in table:
            print(name, "->", [s for s in SCALES if not run_case(ref, name, s)[2]], flush=True)
        return
    out, meta = {}, {}
    for name in table:
        arrays, meta[name], why = run_case(ref, name, sc.case_scale(name))
        assert not why, f"{name}: " + "; ".join(why)
        out.update(arrays)
    out["meta"] = np.asarray(json.dumps(meta))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
