#!/usr/bin/env python3
"""What one fot_openloop_eval call costs against the same evaluation composed by hand from the entries the library had
before it.  A synthetic scene of 2000 windows of 5 to 40 pedestrians (obs_len 8, pred_len 12, dt 0.4), S = 20, three
configurations: constant velocity; a generator without pooling; a generator that pools once per scene (both of the
released checkpoints' dimensions, seeded weights).

* ``call_ms``: ``evaluate_open_loop`` on the window table -- the scene goes to the device, every chunk is gathered, predicted,
  resampled and scored there, one wait;
* ``composed_ms``: per chunk of the same windows, in Python: the window cut from the host scene, ``SganSampler.sample``
  (counter noise of the same seed, window ids as slots) or ``PredictionResampler.predict_cv``,
  ``PredictionResampler.resample_device`` on the chunk, the chunk's tensor rearranged into per-window blocks by one
  ``index_select``, ``BatchPlanner.prediction_scores`` with the truth from host memory, each with its own host
  synchronisation; then the reference's fold in Python.

Both give the same records (checked, byte for byte, before anything is timed).  Same process, A B A B, medians of
--repeats.

    python3 scripts/openloop_bench.py --out profiles/r25_openloop.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS_LEN, PRED_LEN, DT, S = 8, 12, 0.4, 20
SEED = 5


def build_scene(n_windows, rng):
    """Window w starts at frame w and holds 5 .. 40 of the scene's 40 columns (ascending)."""
    seq = OBS_LEN + PRED_LEN
    n_cols = 40
    xy = rng.uniform(-15.0, 15.0, (1, n_cols, 2)) + np.cumsum(rng.normal(0.0, 0.3, (n_windows + seq - 1, n_cols, 2)), axis=0)
    pops = rng.integers(5, 41, n_windows)
    col = [np.sort(rng.choice(n_cols, int(P), replace=False)) for P in pops]
    off = np.concatenate([[0], np.cumsum(pops)]).astype(np.int32)
    return xy, (np.arange(n_windows, dtype=np.int32), off, np.concatenate(col).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--max-rows", type=int, default=8192)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import openloop_common as oc
    import sgan_common as sc
    from integrated_path_planning_amd import _abi, synthetic as syn
    from integrated_path_planning_amd.planner import BatchPlanner
    from integrated_path_planning_amd.prediction import (PredictionResampler, SganSampler, SganWeights, WindowTable,
                                                         evaluate_open_loop, open_loop_result)

    rng = np.random.default_rng(0)
    xy, (f0, off, col) = build_scene(args.windows, rng)
    table = WindowTable(f0, off, col)
    W = len(f0)
    chunks = []                                                      # the library's own chunks (csrc/fot_openloop.hpp: ol_chunk_end)
    w0 = 0
    while w0 < W:
        w1 = w0 + 1
        while w1 < W and off[w1 + 1] - off[w0] <= args.max_rows:
            w1 += 1
        chunks.append((w0, w1))
        w0 = w1

    def weights(pooling):
        e, he, hd, m, b, nd = sc.DIMS["c"]
        a = dict(obs_len=OBS_LEN, pred_len=PRED_LEN, embedding_dim=e, encoder_h_dim=he, decoder_h_dim=hd, mlp_dim=m, bottleneck_dim=b,
                 noise_dim=(nd,), num_layers=1, pooling_type=pooling, pool_every_timestep=False, noise_mix_type="ped",
                 batch_norm=False, dropout=0.0, noise_type="gaussian")
        return SganWeights.from_state_dict(a, sc.seeded_state(a, 11, 2.0))

    configs = {"cv": ("cv", None), "no_pooling": ("lstm", weights(None)), "pooled_once": ("sgan", weights("pool_net"))}
    med = lambda v: float(np.median(v))
    doc = {"windows": W, "rows": int(off[-1]), "samples": S, "obs_len": OBS_LEN, "pred_len": PRED_LEN, "max_rows": args.max_rows,
           "chunks": len(chunks), "repeats": args.repeats, "configurations": {}}
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as engine:
        rs = PredictionResampler(engine, pred_len=PRED_LEN, sgan_dt=DT, sim_dt=DT, plan_horizon=PRED_LEN * DT)
        T = rs.n_dense
        dev = torch.device("cuda", 0)
        for name, (method, w) in configs.items():
            n_s = 1 if method == "cv" else S
            sampler = None if w is None else SganSampler(engine, w, n_s, counter_seed=SEED)
            perms = {}

            def one_call():
                return evaluate_open_loop(engine, xy, OBS_LEN, PRED_LEN, DT, method, 0 if w is not None else None, num_samples=n_s,
                                          seed=SEED, windows=table, max_rows=args.max_rows, records=True)

            def composed():
                recs = []
                for (a, b) in chunks:
                    lo, hi = int(off[a]), int(off[b])
                    obs = np.concatenate([xy[f0[i]:f0[i] + OBS_LEN][:, col[off[i]:off[i + 1]]] for i in range(a, b)], axis=1).astype(np.float32)
                    truth = np.concatenate([xy[f0[i] + OBS_LEN:f0[i] + OBS_LEN + PRED_LEN][:, col[off[i]:off[i + 1]]] for i in range(a, b)],
                                           axis=1).transpose(1, 0, 2)
                    c_off = (off[a:b + 1] - off[a]).astype(np.int32)
                    N = hi - lo
                    if method == "cv":
                        dense = rs.predict_cv(obs, float32_observations=True)          # [N, T, 2] host: S = 1, the blocks lie in order
                        origins = [(int(c_off[i]) * T, 1, int(c_off[i + 1] - c_off[i]), T, False, 0) for i in range(b - a)]
                        recs.append(engine.prediction_scores(dense, origins, truth, 1, PRED_LEN))
                        continue
                    raw = sampler.sample(obs, c_off, slots=np.arange(a, b), steps=np.zeros(b - a, np.int64))
                    torch.cuda.synchronize()
                    out = torch.empty((n_s, N, T, 2), device=dev, dtype=torch.float64)
                    rs.resample_device(raw.data_ptr(), np.float32, n_s, N, obs[-1].astype(np.float64), None, 0.0, out.data_ptr(), np.float64)
                    engine.synchronize()
                    if (a, b) not in perms:                          # per-window blocks [S][P_w][T][2]: rows (s, p) of the chunk, window by window
                        idx = np.concatenate([(np.arange(n_s)[:, None] * N + np.arange(c_off[i], c_off[i + 1])[None]).reshape(-1)
                                              for i in range(b - a)])
                        perms[(a, b)] = torch.as_tensor(idx, device=dev)
                    blocks = out.view(n_s * N, T * 2).index_select(0, perms[(a, b)]).contiguous()
                    origins = [(n_s * int(c_off[i]) * T, n_s, int(c_off[i + 1] - c_off[i]), T, False, 0) for i in range(b - a)]
                    recs.append(engine.prediction_scores(blocks, origins, truth, 1, PRED_LEN))
                rec = np.concatenate(recs)
                return dict(oc.result_of(oc.fold_windows(rec)), records=rec)

            got, want = one_call(), composed()
            same = got["records"].tobytes() == want["records"].tobytes()
            for k in oc.RESULT_KEYS:
                assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) or (method == "cv" and abs(got[k] - want[k]) < 1e-9), (name, k, got[k], want[k])
            assert same or method == "cv", name                      # (CV: fot_predict_cv takes the host path, same numbers)
            a_ms, b_ms = [], []
            for k in range(args.repeats + 1):                        # A B A B; the first pair warms up
                t0 = time.perf_counter(); one_call(); t1 = time.perf_counter(); composed(); t2 = time.perf_counter()
                if k:
                    a_ms.append((t1 - t0) * 1e3); b_ms.append((t2 - t1) * 1e3)
            r = {"call_ms": med(a_ms), "composed_ms": med(b_ms), "ratio": med(b_ms) / med(a_ms), "records_identical": bool(same),
                 "call_ms_all": a_ms, "composed_ms_all": b_ms,
                 "result": {k: (None if isinstance(got[k], float) and np.isnan(got[k]) else got[k]) for k in oc.RESULT_KEYS}}
            doc["configurations"][name] = r
            print(name, json.dumps({k: r[k] for k in ("call_ms", "composed_ms", "ratio", "records_identical")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
