"""Resident episodes that predict from a recorded sample tensor (fot_loop_set_samples, prediction.RecordedSamples /
record_samples), the part that needs no GPU: a recording of the scripted source replayed through the stepwise loop on the
oracle against the reference fixtures and against the live source; the index arithmetic of csrc/fot_samplerec.hpp --
the code k_loop_sample_rows and the host run -- against NumPy, past 2^31 and 2^32 elements on offsets alone; the Python
validation and the refusals that keep their messages."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import recorded_samples_common as rs
from closed_loop_common import OracleEngine, OracleResampler, assert_episode_matches, load_dist_episodes, scripted_sample_source
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.prediction import RecordedSamples, record_samples

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SHIM_SO = os.path.join(EMU_DIR, "_build", "libfot_samplerec_emu.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")


def test_library_exports_the_entry_point():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    assert hasattr(lib, "fot_loop_set_samples") and "fot_loop_set_samples" in _abi.SYMBOLS
    assert re.search(r"\bint\s+fot_loop_set_samples\s*\(", header)
    assert _abi.ABI_VERSION == 8 and re.search(r"#define\s+FOT_ABI_VERSION\s+8\b", header)   # an addition: the version stays


# ---- 1. the recording equals the live calls ---------------------------------------------------------------------------------
def _history_bytes(hist):
    out = []
    for r in hist:
        p = r.planned_path
        out.append((r.time, r.ego.x, r.ego.y, r.ego.yaw, r.ego.v, r.ego.a, r.ego.jerk, r.ego.state.name,
                    r.ped_positions.tobytes(), r.ped_velocities.tobytes(),
                    None if r.predicted_trajectories is None else r.predicted_trajectories.tobytes(),
                    tuple(sorted(r.metrics.items())),
                    None if p is None else (p.cost,) + tuple(np.asarray(getattr(p, f)).tobytes() for f in _abi.PATH_FIELDS)))
    return out


@pytest.mark.parametrize("name", ["s4_eps0", "s5_best_only"])
def test_recording_replayed_on_the_oracle_equals_the_reference_and_the_live_source(name):
    """The scripted source recorded once over the tracks alone (no ego, no planning), then the stepwise loop on the oracle
    reading the recording: the reference's episode, and array for array the history the live source gives -- the observer's
    window does not depend on the ego."""
    ep = load_dist_episodes()
    var = ep["meta"]["variants"][name]
    cfg, tracks = dict(var["config"]), [ep[name + "_ped_traj"]]
    src = scripted_sample_source(var["n_samples"], cfg["pred_len"])
    rec = record_samples(cfg, tracks, src, var["steps"], dtype=np.float64)
    assert isinstance(rec, RecordedSamples) and rec.recorded and rec.needs_history and rec.first_step == 0
    assert rec.num_samples == var["n_samples"] and rec.samples.dtype == np.float64
    assert rec.samples.shape == (var["steps"], var["n_samples"], cfg["pred_len"], tracks[0].shape[1], 2)
    assert np.isfinite(rec.samples).all()                           # (the warm-up fills the observer: every step predicts)
    runs = []
    for source in (rec, src):
        sim = BatchedClosedLoop(cfg, tracks, engine=OracleEngine(cfg), resampler=OracleResampler(cfg), sample_source=source)
        hist = sim.run()[0]
        assert_episode_matches(hist, sim.episodes[0].termination_reason, ep, name)
        runs.append(_history_bytes(hist))
    assert runs[0] == runs[1]


def test_record_samples_fills_the_steps_before_the_observer_is_ready_with_nan():
    """A shorter warm-up leaves the observer filling for the first lock steps: their rows are NaN, the first ready step's
    row is the source's answer to the observer's window at that step."""
    ep = load_dist_episodes()
    var = ep["meta"]["variants"]["s4_eps0"]
    cfg, tracks = dict(var["config"]), [ep["s4_eps0_ped_traj"]]
    src = scripted_sample_source(3, cfg["pred_len"])
    full = record_samples(cfg, tracks, src, 12, dtype=np.float64)
    short = record_samples(cfg, tracks, src, 12, dtype=np.float64, warmup_frames=22)      # 10 frames short: ready at step 9
    ready = np.isfinite(short.samples).all(axis=(1, 2, 3, 4))
    assert not np.isfinite(short.samples[~ready]).any()
    assert list(np.flatnonzero(ready)) == [9, 10, 11]
    # the clock is the tracks' own: step k of the short run is frame 23 + k, step k of the full one frame 33 + k, and the
    # observer has sampled the same frames 4, 8, ..., 32 in both
    assert full.samples.shape == short.samples.shape and np.isfinite(full.samples).all()
    assert np.array_equal(short.samples[10:12], full.samples[0:2])


# ---- 2. the index arithmetic ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(EMU_DIR, "fot_samplerec_emu.cpp"), os.path.join(CSRC, "fot_samplerec.hpp")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SHIM_SO, srcs[0]], check=True)
    L = C.CDLL(SHIM_SO)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.sr_step_elems_of.restype = L.sr_rec_elems_of.restype = L.sr_src_of.restype = L.sr_dst_of.restype = i64
    L.sr_step_elems_of.argtypes = [i32, i32, i32]
    L.sr_rec_elems_of.argtypes = [i64, i32, i32, i32]
    L.sr_covers_of.argtypes = [i32, i32, i64]
    L.sr_split_of.argtypes = [i32, i32, i32, i64, vp]
    L.sr_src_of.argtypes = [i32, i32, i32, i64, i32, i32, i32]
    L.sr_dst_of.argtypes = [i32, i32, i32, i32, i32, i32]
    L.sr_column_of.argtypes = [i32, vp, vp, vp, vp]
    L.sr_fill_columns_of.argtypes = [i32, vp, vp, vp, vp]
    L.sr_kernel_offsets.argtypes = [i32, i32, i32, i32, i64, vp, vp, vp]
    return L


PED_OFFS = {
    "ragged": np.cumsum([0, 0, 1, 33, 0, 65, 30, 0]),              # slots of 0 pedestrians at either end and in the middle
    "single": np.cumsum([0, 7]),
}
RUNNING = {
    "ragged": ([0, 1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], [0, 1, 2, 4, 5, 6], [0, 1, 2, 3, 4, 5], [2, 5], [0, 3, 6], [5]),
    "single": ([0],),
}


@pytest.mark.parametrize("layout", sorted(PED_OFFS))
def test_every_element_of_a_frame_maps_to_the_restated_offset(shim, layout):
    """All slots, the first / a middle / the last slot dropped, slots of no pedestrians anywhere, first_step > 0: the
    column of every row (per row as a kernel would form it, and the table the host forms), and the element every lane of
    k_loop_sample_rows reads and writes."""
    ped_off = PED_OFFS[layout].astype(np.int32)
    n_cols = int(ped_off[-1])
    for slots in RUNNING[layout]:
        ped_ep, ep_ped0, ep_slot = rs.frame_tables(ped_off, slots)
        want_cols = rs.columns_of(ped_off, slots)
        rows = len(want_cols)
        got = np.array([shim.sr_column_of(q, ped_ep.ctypes.data, ep_ped0.ctypes.data, ep_slot.ctypes.data, ped_off.ctypes.data)
                        for q in range(rows)], np.int64)
        assert np.array_equal(got, want_cols), (layout, slots)
        col = np.full(rows + 1, -7, np.int32)
        shim.sr_fill_columns_of(len(slots), ep_ped0.ctypes.data, ep_slot.ctypes.data, ped_off.ctypes.data, col.ctypes.data)
        assert np.array_equal(col[:rows], want_cols) and col[rows] == -7
        for S, L, step, first in ((1, 1, 0, 0), (3, 12, 17, 0), (64, 2, 9, 4)):
            rec_row = step - first
            n = S * L * rows
            assert shim.sr_step_elems_of(S, L, rows) == n
            src, dst = np.full(n + 1, -1, np.int64), np.full(n + 1, -1, np.int64)
            shim.sr_kernel_offsets(S, L, rows, n_cols, rec_row, col.ctypes.data, src.ctypes.data, dst.ctypes.data)
            assert src[n] == -1 and dst[n] == -1
            assert np.array_equal(dst[:n], np.arange(n))             # lane t writes element t: rows innermost, contiguous
            assert np.array_equal(src[:n].reshape(S, L, rows), rs.source_offsets(S, L, n_cols, rec_row, want_cols))
            # ... and a gather through them is the recording's row cut to the running slots' columns
            rec = np.arange((rec_row + 1) * S * L * n_cols, dtype=np.int64).reshape(rec_row + 1, S, L, n_cols)
            assert np.array_equal(rec.ravel()[src[:n]].reshape(S, L, rows), rec[rec_row][:, :, want_cols])


def test_offsets_past_2_31_and_2_32_elements(shim):
    """256 episodes x 30 pedestrians, S = 64, pred_len 12, float64: row 400 starts past 2^31 elements, row 800 past 2^32 --
    checked on the offsets alone, nothing allocated; and a step whose own element count passes 2^32 still splits."""
    S, L, n_cols = 64, 12, 256 * 30
    for rec_row in (0, 400, 800, 2 ** 31 - 1):
        for s, j, col in ((0, 0, 0), (S - 1, L - 1, n_cols - 1), (17, 5, 4321)):
            want = rs.source_offset(S, L, n_cols, rec_row, s, j, col)
            assert shim.sr_src_of(S, L, n_cols, rec_row, s, j, col) == want
    assert rs.source_offset(S, L, n_cols, 400, 0, 0, 0) > 2 ** 31 and rs.source_offset(S, L, n_cols, 800, 0, 0, 0) > 2 ** 32
    assert shim.sr_rec_elems_of(2 ** 31 - 1, S, L, n_cols) == (2 ** 31 - 1) * S * L * n_cols
    # lane -> (s, j, row) on both sides of the 32-bit path
    sjr = np.zeros(3, np.int32)
    for S2, L2, rows in ((64, 32, 7680), (64, 32, 3_000_000)):
        total = S2 * L2 * rows
        assert shim.sr_step_elems_of(S2, L2, rows) == total
        for t in (0, 1, rows - 1, rows, total // 2 + 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + rows + 1, total - 1):
            if not 0 <= t < total:
                continue
            shim.sr_split_of(S2, L2, rows, t, sjr.ctypes.data)
            assert tuple(sjr) == (t // rows // L2, t // rows % L2, t % rows), (rows, t)
            assert shim.sr_dst_of(S2, L2, rows, *[int(v) for v in sjr]) == t
    assert 64 * 32 * 3_000_000 > 2 ** 32


def test_which_steps_a_recording_covers(shim):
    for first, n, step, want in ((0, 1, 0, 1), (0, 1, 1, 0), (4, 3, 3, 0), (4, 3, 4, 1), (4, 3, 6, 1), (4, 3, 7, 0),
                                 (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 32 - 3, 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 32 - 2, 0)):
        assert shim.sr_covers_of(first, n, step) == want, (first, n, step)


# ---- 3. Python validation ------------------------------------------------------------------------------------------------------
def test_recorded_samples_validation():
    ep = load_dist_episodes()
    cfg = dict(ep["meta"]["variants"]["s4_eps0"]["config"])
    tracks = [ep["s4_eps0_ped_traj"]]
    P, L = tracks[0].shape[1], cfg["pred_len"]
    good = np.zeros((5, 4, L, P, 2))
    ok = RecordedSamples(good, first_step=3)
    assert (ok.num_samples, ok.first_step, ok.recorded, ok.needs_history) == (4, 3, True, True)
    with pytest.raises(ValueError, match=r"\[n_steps, S, pred_len, sum P, 2\]"):
        RecordedSamples(good[0])                                    # wrong rank
    with pytest.raises(ValueError, match=r"\[n_steps, S, pred_len, sum P, 2\]"):
        RecordedSamples(np.zeros((5, 4, L, P, 3)))                  # a wrong last axis
    with pytest.raises(ValueError, match="S <= 64"):
        RecordedSamples(np.zeros((1, 65, 1, 1, 2)))
    with pytest.raises(ValueError, match="float32 or float64"):
        RecordedSamples(np.zeros((5, 4, L, P, 2), np.int32))
    with pytest.raises(ValueError, match="first_step"):
        RecordedSamples(good, first_step=-1)
    kw = dict(engine=OracleEngine(cfg), resampler=OracleResampler(cfg))
    with pytest.raises(ValueError, match="pedestrian columns"):     # sum P differs from the tracks
        BatchedClosedLoop(cfg, tracks, sample_source=RecordedSamples(np.zeros((5, 4, L, P + 1, 2))), **kw)
    with pytest.raises(ValueError, match="pred_len"):               # pred_len differs from the configuration
        BatchedClosedLoop(cfg, tracks, sample_source=RecordedSamples(np.zeros((5, 4, L - 1, P, 2))), **kw)
    # a step outside the recording is named
    sim = BatchedClosedLoop(cfg, tracks, sample_source=RecordedSamples(np.zeros((2, 4, L, P, 2)), first_step=1), **kw)
    with pytest.raises(IndexError, match="lock step 0 predicts.*covers steps 1 .. 2"):
        sim.step()


def test_stepwise_rows_are_cut_to_the_running_slots():
    rng = np.random.default_rng(5)
    ped_off = np.array([0, 2, 2, 5, 9])
    rec = RecordedSamples(rng.normal(size=(6, 3, 4, 9, 2)).astype(np.float32), first_step=2)
    rec.attach(ped_off, 4, device_samples=False)
    whole = rec(None, None, slots=np.arange(4), steps=np.full(4, 2))
    assert whole.dtype == np.float32 and np.array_equal(whole, rec.samples[0])
    part = rec(None, np.array([0, 2, 6]), slots=np.array([0, 3]), steps=np.array([7, 7]))
    assert part.flags.c_contiguous and np.array_equal(part, rec.samples[5][:, :, [0, 1, 5, 6, 7, 8]])
    with pytest.raises(ValueError, match="slots, steps"):
        rec(None, None)
    with pytest.raises(ValueError, match="one and the same lock step"):
        rec(None, None, slots=np.array([0, 3]), steps=np.array([3, 4]))
    with pytest.raises(IndexError, match="lock step 8"):
        rec(None, None, slots=np.array([0, 3]), steps=np.array([8, 8]))
    with pytest.raises(ValueError, match="the frame has 5 pedestrians"):
        rec(None, np.array([0, 2, 5]), slots=np.array([0, 3]), steps=np.array([3, 3]))


def test_pinned_refusals_keep_their_messages_without_a_recording():
    """The constructor's refusals where no RecordedSamples is involved, word for word; the ones that need the library's own
    sampler are held by tests/test_gpu_loop_sgan.py."""
    ep = load_dist_episodes()
    cfg = dict(ep["meta"]["variants"]["s4_eps0"]["config"])
    tracks = [ep["s4_eps0_ped_traj"]]
    src = scripted_sample_source(4, cfg["pred_len"])
    msg = "resident=True needs the constant-velocity predictor"
    with pytest.raises(ValueError, match=msg):                      # a plain callable
        BatchedClosedLoop(cfg, tracks, sample_source=src, device_samples=True, resident=True)
    with pytest.raises(ValueError, match=msg):                      # a source without device_samples
        BatchedClosedLoop(cfg, tracks, sample_source=src, resident=True)
    with pytest.raises(ValueError, match=msg):                      # ... a recording too: it goes through device memory
        BatchedClosedLoop(cfg, tracks, sample_source=RecordedSamples(np.zeros((2, 4, cfg["pred_len"], 14, 2))), resident=True)
    with pytest.raises(ValueError, match="summaries=True with a sampler"):
        BatchedClosedLoop(cfg, tracks, sample_source=RecordedSamples(np.zeros((2, 4, cfg["pred_len"], 14, 2))),
                          device_samples=True, resident=True, summaries=True)
    with pytest.raises(ValueError, match="summaries=True needs resident=True"):
        BatchedClosedLoop(cfg, tracks, sample_source=src, summaries=True)
    with pytest.raises(ValueError, match="prediction_scores=True scores the stepwise loop's distributions"):
        BatchedClosedLoop(cfg, tracks, sample_source=src, device_samples=True, resident=True, prediction_scores=True)
