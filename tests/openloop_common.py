"""The open-loop prediction evaluation (fot_openloop_eval; reference examples/run_openloop_prediction.py) restated in NumPy for
the tests (CPU and GPU) from ``prediction_common`` (process_prediction, predict_cv) and ``pred_scores_common`` (one origin's
record), with the reference's fold written from evaluate_scene's loop body -- plus the synthetic scenes, fixture access and a
writer / reader of the emulation program's files.

Tolerances (none invented here): records and totals of identical inputs against this restatement and against the emulation
program: ``SUM_RTOL`` alone (``pred_scores_common``); against the reference's numbers in the fixture on the REFERENCE's raw
samples: ``SUM_RTOL`` plus ``PRED_ATOL`` (``nll``: the fixture's ``nll_atol``), as the prediction-score tests hold them."""
import json
import os
import struct

import numpy as np

from conftest import GOLDEN_DIR
from pred_scores_common import FLAG_NLL, RECORD_DT, origin_terms
from prediction_common import predict_cv, process_samples

FIXTURE = os.path.join(GOLDEN_DIR, "openloop", "cases.npz")
TOTALS_DT = np.dtype([(n, "f8") for n in ("sum_ade", "sum_fde", "sum_ade_agent", "sum_fde_agent", "sum_nll")]
                     + [("traj_count", "i8"), ("nll_count", "i8"), ("n_windows", "i4"), ("flags", "i4")])
RESULT_KEYS = ("n_windows", "n_trajectories", "ade", "fde", "ade_per_agent", "fde_per_agent", "nll")
WINDOW_KEYS = ("ade", "fde", "ade_per_agent", "fde_per_agent", "ade_eval_count", "nll", "nll_eval_count")
OBS_LEN, PRED_LEN, DT = 8, 12, 0.4
# the fixture's two generators (tests/sgan_common.seeded_state): dims "b" of sgan_common, pooled at every step and not pooled
MODEL_ARGS = {
    "lstm": dict(obs_len=OBS_LEN, pred_len=PRED_LEN, embedding_dim=12, encoder_h_dim=20, decoder_h_dim=28, mlp_dim=40,
                 bottleneck_dim=6, noise_dim=(4,), num_layers=1, pooling_type=None, pool_every_timestep=False,
                 noise_mix_type="ped", batch_norm=False, dropout=0.0, noise_type="gaussian"),
    "sgan": dict(obs_len=OBS_LEN, pred_len=PRED_LEN, embedding_dim=12, encoder_h_dim=20, decoder_h_dim=28, mlp_dim=40,
                 bottleneck_dim=6, noise_dim=(4,), num_layers=1, pooling_type="pool_net", pool_every_timestep=True,
                 noise_mix_type="ped", batch_norm=False, dropout=0.0, noise_type="gaussian"),
}
MODEL_SEED = {"lstm": 4101, "sgan": 4102}
MODEL_SCALE = 2.0
NUM_SAMPLES = 5


def load_cases():
    z = np.load(FIXTURE, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def synthetic_scene(n_frames=30, n_ids=8, seed=11, dt=DT):
    """[n_frames, n_ids, 2] float64, NaN where a pedestrian is absent: walkers that enter and leave at different frames (two
    stay throughout, one stands still, one is present in two separate spells) -- the populations of consecutive windows of
    20 frames differ."""
    rng = np.random.default_rng(seed)
    start = rng.uniform(-8.0, 8.0, (n_ids, 2))
    vel = rng.uniform(-1.2, 1.2, (n_ids, 2))
    vel[2] = 0.0                                                        # stands still: process_prediction's constant fill
    steps = vel[None] * dt + rng.normal(0.0, 0.04, (n_frames, n_ids, 2)) * (np.abs(vel[None]).sum(axis=2, keepdims=True) > 0)
    xy = start[None] + np.cumsum(steps, axis=0)
    spells = [(0, n_frames), (0, 27), (0, 23), (0, 20), (1, 26), (3, n_frames), (5, 27), (8, n_frames)]
    back = xy[22, 3].copy() if n_ids > 3 and n_frames > 22 else None
    for i in range(n_ids):
        lo, hi = spells[i % len(spells)]
        xy[:lo, i] = np.nan
        xy[hi:, i] = np.nan
    if back is not None:
        xy[22, 3] = back                                                # (a second spell, too short for any window)
    return xy


def random_scene(rng, n_frames, n_ids, p_absent=0.0):
    """Walkers over the whole scene; with ``p_absent`` every pedestrian misses a random run of frames."""
    xy = rng.uniform(-10.0, 10.0, (1, n_ids, 2)) + np.cumsum(rng.normal(0.0, 0.3, (n_frames, n_ids, 2)), axis=0)
    for i in np.flatnonzero(rng.random(n_ids) < p_absent):
        lo = int(rng.integers(0, n_frames))
        xy[lo:lo + int(rng.integers(1, n_frames)), i] = np.nan
    return xy


def reference_windows(xy, seq_len, stride=1, min_peds=1):
    """``extract_fixed_windows`` written as the reference writes it (frame dictionaries, set intersection, sorted ids):
    (win_frame0, ped_off, row_col) for a dense scene whose columns are the ids in ascending order."""
    by_frame = [{i: xy[t, i] for i in range(xy.shape[1]) if not np.isnan(xy[t, i]).any()} for t in range(xy.shape[0])]
    f0, off, col = [], [0], []
    for start in range(0, xy.shape[0] - seq_len + 1, stride):
        present = set(by_frame[start].keys())
        for fd in by_frame[start + 1:start + seq_len]:
            present &= set(fd.keys())
        if len(present) < min_peds:
            continue
        ids = sorted(present)
        f0.append(start); col += ids; off.append(len(col))
    return np.asarray(f0, np.int32), np.asarray(off, np.int32), np.asarray(col, np.int32)


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------
def window_rows(xy, f0, cols, obs_len, pred_len):
    """(obs [obs_len, P, 2] float32, truth [P, pred_len, 2] float64) of one window."""
    win = np.asarray(xy)[f0:f0 + obs_len + pred_len][:, cols].astype(np.float64)
    return win[:obs_len].astype(np.float32), np.ascontiguousarray(win[obs_len:].transpose(1, 0, 2))


def window_record(xy, f0, cols, obs_len, pred_len, dt, raw=None):
    """One window's record.  raw None: constant velocity from the float32 observations; else the generator's raw samples
    [S, pred_len, P, 2] of the window's rows, resampled from the float32 last observation."""
    obs, truth = window_rows(xy, f0, cols, obs_len, pred_len)
    kw = dict(sgan_dt=dt, sim_dt=dt, plan_horizon=pred_len * dt)
    if raw is None:
        dense = predict_cv(obs[-1], obs[-2] if obs_len >= 2 else None, 0.0, pred_len=pred_len, **kw)[None]
    else:
        dense = process_samples(np.asarray(raw), obs[-1].astype(np.float64), 0.0, **kw)
    return origin_terms(dense, truth, 1)


def scene_records(xy, table, obs_len, pred_len, dt, raw=None):
    """Every window's record; raw: [S, pred_len, rows, 2] of the whole table."""
    f0, off, col = table
    out = np.zeros(len(f0), RECORD_DT)
    for w in range(len(f0)):
        lo, hi = int(off[w]), int(off[w + 1])
        out[w] = window_record(xy, int(f0[w]), col[lo:hi], obs_len, pred_len, dt, None if raw is None else raw[:, :, lo:hi])
    return out


def window_metrics(r):
    """``calculate_aggregate_metrics`` of the window's history (one eligible origin) from its record (metrics.py:96-113,
    171-176): the sums start at 0.0, ``ade = total_ade / trajectory_count`` with ``total_ade = min * n_peds``."""
    nan = float("nan")
    P = int(r["n_peds"])
    m = dict(ade=nan, fde=nan, ade_per_agent=nan, fde_per_agent=nan, ade_eval_count=P, nll=nan, nll_eval_count=0)
    if P > 0:
        m["ade"] = (0.0 + float(r["ade_scene"]) * P) / P
        m["fde"] = (0.0 + float(r["fde_scene"]) * P) / P
        m["ade_per_agent"] = (0.0 + float(r["ade_agent_sum"])) / P
        m["fde_per_agent"] = (0.0 + float(r["fde_agent_sum"])) / P
    if int(r["flags"]) & FLAG_NLL and int(r["nll_count"]) > 0:
        m["nll"] = -(0.0 + float(r["log_lik_sum"])) / int(r["nll_count"])
        m["nll_eval_count"] = int(r["nll_count"])
    return m


def fold_windows(records, raw_sums=False):
    """``evaluate_scene``'s loop over the windows' metrics (run_openloop_prediction.py:122-142) -> TOTALS_DT.  raw_sums: the
    WRONG fold a library would be tempted to write -- the records' own sums instead of ``m[...] * count`` --, kept for the
    test that tells the two apart."""
    t = np.zeros((), TOTALS_DT)
    sums = [0.0] * 5
    traj = nll_n = flags = 0
    for r in records:
        m = window_metrics(r)
        n = m["ade_eval_count"]
        flags |= int(r["flags"])
        if n > 0 and not np.isnan(m["ade"]):
            if raw_sums:
                sums[0] += float(r["ade_scene"]) * n; sums[1] += float(r["fde_scene"]) * n
                sums[2] += float(r["ade_agent_sum"]); sums[3] += float(r["fde_agent_sum"])
            else:
                sums[0] += m["ade"] * n; sums[1] += m["fde"] * n
                sums[2] += m["ade_per_agent"] * n; sums[3] += m["fde_per_agent"] * n
            traj += n
        k = m["nll_eval_count"]
        if k > 0 and not np.isnan(m["nll"]):
            sums[4] += -float(r["log_lik_sum"]) if raw_sums else m["nll"] * k
            nll_n += k
    for name, v in zip(TOTALS_DT.names[:5], sums):
        t[name] = v
    t["traj_count"], t["nll_count"], t["n_windows"], t["flags"] = traj, nll_n, len(records), flags
    return t


def result_of(t):
    """evaluate_scene's dictionary from totals (a TOTALS_DT record or the library's structure)."""
    get = (lambda k: t[k]) if isinstance(t, np.ndarray) or isinstance(t, np.void) else (lambda k: getattr(t, k))
    nan = float("nan")
    n, k = int(get("traj_count")), int(get("nll_count"))
    return dict(n_windows=int(get("n_windows")), n_trajectories=n, ade=float(get("sum_ade")) / n if n else nan,
                fde=float(get("sum_fde")) / n if n else nan, ade_per_agent=float(get("sum_ade_agent")) / n if n else nan,
                fde_per_agent=float(get("sum_fde_agent")) / n if n else nan, nll=float(get("sum_nll")) / k if k else nan)


def totals_record(t):
    """The library's ``_abi.OpenLoopTotals`` as a TOTALS_DT record."""
    out = np.zeros((), TOTALS_DT)
    for k in TOTALS_DT.names:
        out[k] = getattr(t, k)
    return out


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def close(got, want, rtol, atol, what):
    if np.isnan(want) or np.isinf(want):
        assert (np.isnan(got) and np.isnan(want)) or got == want, f"{what}: {got!r}, expected {want!r}"
    else:
        assert abs(got - want) <= atol + rtol * abs(want), f"{what}: {got!r}, expected {want!r} (diff {got - want:.3e})"


def assert_result_close(got, want, rtol, atol, nll_atol, label):
    for k in ("n_windows", "n_trajectories"):
        assert int(got[k]) == int(want[k]), f"{label} {k}: {got[k]!r}, expected {want[k]!r}"
    for k in ("ade", "fde", "ade_per_agent", "fde_per_agent"):
        close(float(got[k]), float(want[k]), rtol, atol, f"{label} {k}")
    close(float(got["nll"]), float(want["nll"]), rtol, nll_atol, f"{label} nll")


def assert_totals_close(got, want, rtol, label):
    for k in ("traj_count", "nll_count", "n_windows", "flags"):
        assert int(got[k]) == int(want[k]), f"{label} {k}: {int(got[k])}, expected {int(want[k])}"
    for k in TOTALS_DT.names[:5]:
        close(float(got[k]), float(want[k]), rtol, 0.0, f"{label} {k}")


# ---- tests/emu/fot_openloop_emu --------------------------------------------------------------------------------------------------------
def write_emu_case(path, xy, table, obs_len, pred_len, dt, raw=None, S=None, max_rows=0, dtype=np.float64):
    f0, off, col = (np.ascontiguousarray(v, np.int32) for v in table)
    xy = np.ascontiguousarray(xy, dtype)
    S = (1 if raw is None else raw.shape[0]) if S is None else S
    with open(path, "wb") as f:
        f.write(struct.pack("<10i", xy.shape[0], xy.shape[1], len(f0), 0 if dtype == np.float32 else 1, obs_len, pred_len,
                            0 if raw is None else 1, S, max_rows, 0))
        f.write(struct.pack("<d", dt))
        f.write(f0.tobytes()); f.write(off.tobytes()); f.write(col.tobytes())
        f.write(xy.tobytes())
        if raw is not None:
            f.write(np.ascontiguousarray(raw, np.float32).tobytes())


def read_emu_out(path):
    """(code, totals or None, records or None)"""
    with open(path, "rb") as f:
        data = f.read()
    code, n = struct.unpack_from("<2i", data, 0)
    if code != 0:
        return code, None, None
    t = np.frombuffer(data, TOTALS_DT, 1, 8)[0]
    return code, t, np.frombuffer(data, RECORD_DT, n, 8 + TOTALS_DT.itemsize)
