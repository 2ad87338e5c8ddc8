"""Whole replayed episodes inside the library (fot_loop_set_replay / fot_loop_run), the part that needs no GPU: the C
ABI's symbols and structure layouts, and the host logic of csrc/fot_replay.hpp -- replay clock, observer, prepend test,
termination test -- run through a g++ build of tests/emu/fot_replay_emu.cpp against closed_loop.py's Observer,
ReplayPedestrians and BatchedClosedLoop._loop_frame."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop, Observer, ReplayPedestrians

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SHIM_SO = os.path.join(EMU_DIR, "_build", "libfot_replay_emu.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
NEW_SYMBOLS = ("fot_loop_set_replay", "fot_loop_run")


def test_library_exports_the_replay_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} not exported by libfot.so"
        assert sym in _abi.SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} not declared in include/fot.h"


def test_ctypes_mirrors_of_the_replay_structures_match_c(tmp_path):
    fields_r = [n for n, _ in _abi.LoopReplay._fields_]
    fields_o = [n for n, _ in _abi.LoopRunOut._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fot.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(fot_loop_replay), sizeof(fot_loop_run_out));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(fot_loop_replay, {n}));\n' for n in fields_r)
                   + "".join(f'  printf("%zu\\n", offsetof(fot_loop_run_out, {n}));\n' for n in fields_o)
                   + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_abi.LoopReplay), C.sizeof(_abi.LoopRunOut)]
    want += [getattr(_abi.LoopReplay, n).offset for n in fields_r] + [getattr(_abi.LoopRunOut, n).offset for n in fields_o]
    assert got == want
    assert tuple(fields_o) == _abi.LOOP_RUN_OUT_FIELDS


@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(EMU_DIR, "fot_replay_emu.cpp"), os.path.join(CSRC, "fot_replay.hpp")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SHIM_SO, srcs[0]], check=True)
    L = C.CDLL(SHIM_SO)
    vp = C.c_void_p
    L.replay_clock_run.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp, vp]
    L.replay_rows.argtypes = [C.c_int, vp, C.c_int, vp]
    L.replay_rows.restype = None
    L.replay_prepend_flags.argtypes = [C.c_int, vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, vp]
    L.replay_prepend_flags.restype = None
    L.replay_termination_codes.argtypes = [C.c_int, vp, vp, C.c_double, C.c_double, vp]
    L.replay_termination_codes.restype = None
    return L


def _clock(shim, obs_len, dt, sgan_dt, warmup, n_steps):
    state, stale = np.zeros((n_steps, 4), np.int32), np.zeros(n_steps)
    shim.replay_clock_run(obs_len, dt, sgan_dt, warmup, n_steps, state.ctypes.data, stale.ctypes.data)
    return state, stale


def _prepend(shim, off, last, prev, cur, sgan_dt, dt, stale):
    off = np.ascontiguousarray(off, np.int32)
    last, prev, cur = (np.ascontiguousarray(a, np.float64) for a in (last, prev, cur))
    flag = np.zeros(len(off) - 1, np.uint8)
    shim.replay_prepend_flags(len(off) - 1, off.ctypes.data, last.ctypes.data, prev.ctypes.data, cur.ctypes.data,
                              sgan_dt, dt, stale, flag.ctypes.data)
    return flag.astype(bool)


def _python_frame(off, hist, pos, dt, sgan_dt, ped_time, last_time):
    """BatchedClosedLoop._loop_frame on a loop object that holds just what the method reads."""
    n = len(off) - 1
    loop = BatchedClosedLoop.__new__(BatchedClosedLoop)
    loop.ego, loop.ego_radius, loop.ped_radius, loop.footprint = np.zeros((n, 5)), 1.0, 0.3, None
    loop.peds, loop.dt, loop.sgan_dt, loop.ped_time, loop._device_samples = [None] * n, dt, sgan_dt, ped_time, False
    loop.resampler = SimpleNamespace(pred_len=8, params=None)
    loop.observer = SimpleNamespace(is_ready=True, history=hist, last_sample_time=last_time)
    frame, _ = loop._loop_frame(np.arange(n), np.asarray(off), pos, np.zeros_like(pos))
    return np.asarray(frame["prepend"], bool), float(frame["staleness"])


@pytest.mark.parametrize("block", range(4))
def test_clock_observer_and_prepend_equal_python(shim, block):
    """60 seeds per block (240 in all): random recordings -- episodes with 0, 1 and many pedestrians, recordings shorter
    than the run --, dt in {0.05, 0.1, 0.2}, obs_len in {2, 8}.  After every step: replay row of every episode, readiness,
    the frames of the observer's last two samples and the staleness equal ReplayPedestrians / Observer exactly; the
    prepend flags equal _loop_frame's on the same data."""
    for seed in range(60 * block, 60 * (block + 1)):
        rng = np.random.default_rng(seed)
        dt = (0.05, 0.1, 0.2)[seed % 3]
        obs_len = (2, 8)[(seed // 3) % 2]
        sgan_dt = 0.4
        warmup = int(obs_len * sgan_dt / dt) if seed % 5 else int(rng.integers(0, 4))     # (some start with an empty observer)
        n_steps = int(rng.integers(20, 70))
        counts = [0, 1, int(rng.integers(2, 12))] + [int(rng.integers(0, 6)) for _ in range(int(rng.integers(0, 4)))]
        rng.shuffle(counts)
        n_frames = [int(rng.integers(1, warmup + n_steps + 10)) for _ in counts]
        n_frames[int(rng.integers(len(counts)))] = max(1, (warmup + n_steps) // 2)          # held for half of the run
        tracks = []
        for P, F in zip(counts, n_frames):
            start = rng.uniform(-30, 30, (1, P, 2))
            walk = rng.uniform(-1.5, 1.5, (1, P, 2)) * (rng.random((1, P, 1)) > 0.4)       # (some stand still)
            tracks.append(start + walk * dt * np.arange(F)[:, None, None])
        peds = [ReplayPedestrians(tr, dt) for tr in tracks]
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        t_max = max(n_frames)
        side = np.zeros((t_max, int(off[-1]), 2))
        for e, tr in enumerate(tracks):
            side[: len(tr), off[e]:off[e + 1]] = tr
            side[len(tr):, off[e]:off[e + 1]] = tr[-1]
        obs = Observer(obs_len, dt, sgan_dt)
        frame, ped_time, frames_of = 0, 0.0, []                    # frames_of: frame of every sample in the window

        def advance():
            nonlocal frame, ped_time
            for p in peds:
                p.step()
            frame += 1
            ped_time += dt
            before = len(obs.history), (obs.timestamps[-1] if obs.timestamps else None)
            obs.update(side[min(frame, t_max - 1)], ped_time)
            if (len(obs.history), obs.timestamps[-1] if obs.timestamps else None) != before:
                frames_of.append(frame)
                del frames_of[:-obs_len]

        for _ in range(warmup):
            advance()
        state, stale = _clock(shim, obs_len, dt, sgan_dt, warmup, n_steps)
        for k in range(n_steps):
            advance()
            assert state[k, 0] == frame
            for e, p in enumerate(peds):
                row = np.zeros(1, np.int32)
                shim.replay_rows(1, np.array([frame], np.int32).ctypes.data, p.n_frames, row.ctypes.data)
                assert row[0] == p._idx, (seed, k, e)
            assert bool(state[k, 1]) == obs.is_ready, (seed, k)
            last_t = obs.last_sample_time
            want_stale = max(ped_time - last_t, 0.0) if last_t is not None else 0.0
            assert stale[k] == want_stale, (seed, k)
            if not obs.is_ready:
                assert tuple(state[k, 2:]) == (-1, -1)
                continue
            assert tuple(state[k, 2:]) == (frames_of[-1], frames_of[-2]), (seed, k)
            np.testing.assert_array_equal(obs.history[-1], side[min(state[k, 2], t_max - 1)])
            np.testing.assert_array_equal(obs.history[-2], side[min(state[k, 3], t_max - 1)])
            pos = side[min(frame, t_max - 1)]
            want, py_stale = _python_frame(off, obs.history, pos, dt, sgan_dt, ped_time, last_t)
            assert py_stale == stale[k]
            got = _prepend(shim, off, obs.history[-1], obs.history[-2], pos, sgan_dt, dt, stale[k])
            np.testing.assert_array_equal(got, want, err_msg=f"seed {seed} step {k}")


def test_prepend_on_the_allclose_boundary(shim):
    """Pedestrians whose current position lies on the 1e-8 + 1e-5 |x| boundary of the first predicted one, a few
    representable numbers to either side: the flag equals _loop_frame's for every one of them, and both answers occur."""
    rng = np.random.default_rng(7)
    dt, sgan_dt = 0.1, 0.4
    seen = set()
    for trial in range(300):
        stale = float(rng.choice([0.0, 0.1, 0.30000000000000004]))
        last = rng.uniform(-40, 40, (1, 2)).astype(np.float32).astype(np.float64)
        prev = (last - rng.uniform(-0.6, 0.6, (1, 2))).astype(np.float32).astype(np.float64)
        vel32 = (last.astype(np.float32) - prev.astype(np.float32)) / np.float32(sgan_dt)
        first = last + vel32.astype(np.float64) * ((dt + 0.0 * dt) + stale)
        axis, sign = int(rng.integers(2)), float(rng.choice([-1.0, 1.0]))
        x = first[0, axis]
        edge = x + sign * (1e-8 + 1e-5 * abs(x)) / (1.0 - sign * np.sign(x) * 1e-5)      # |first - pos| ~ tol(pos)
        for nudge in range(-6, 7):
            v = edge
            for _ in range(abs(nudge)):
                v = np.nextafter(v, np.inf if nudge > 0 else -np.inf)
            pos = first.copy()
            pos[0, axis] = v
            hist = [prev, last]
            want, _ = _python_frame([0, 1], hist, pos, dt, sgan_dt, 1.0 + stale, 1.0)
            got = _prepend(shim, [0, 1], last, prev, pos, sgan_dt, dt, max((1.0 + stale) - 1.0, 0.0))
            assert got[0] == want[0], (trial, nudge)
            seen.add(bool(want[0]))
    assert seen == {False, True}


def test_termination_codes_equal_the_numpy_test(shim):
    rng = np.random.default_rng(3)
    s_end = 71.25
    s_now = np.concatenate([rng.uniform(0, 80, 500), [s_end - 2.0, np.nextafter(s_end - 2.0, 0), np.nextafter(s_end - 2.0, 100),
                                                       np.nan, np.inf, -np.inf, s_end]])
    coll = (rng.random(len(s_now)) < 0.3).astype(np.int32)
    code = np.zeros(len(s_now), np.int32)
    shim.replay_termination_codes(len(s_now), coll.ctypes.data, s_now.ctypes.data, s_end, 2.0, code.ctypes.data)
    collided = coll != 0
    with np.errstate(invalid="ignore"):
        at_goal = s_end - s_now < 2.0
    want = np.zeros(len(s_now), np.int32)
    want[at_goal & ~collided] = 2
    want[collided] = 1
    np.testing.assert_array_equal(code, want)
    assert set(want) == {0, 1, 2}


def test_resident_needs_the_librarys_own_engine_and_the_cv_predictor():
    cfg = dict(dt=0.1, prediction_method="cv")
    tracks = [np.zeros((10, 1, 2))]
    with pytest.raises(ValueError, match="resident"):
        BatchedClosedLoop(cfg, tracks, engine=object(), resident=True)
    with pytest.raises(ValueError, match="resident"):
        BatchedClosedLoop(cfg, tracks, sample_source=lambda last, prev: None, resident=True)
    with pytest.raises(ValueError, match="resident"):
        BatchedClosedLoop(cfg, tracks, fused=False, resident=True)
    with pytest.raises(ValueError):
        BatchedClosedLoop(cfg, tracks, fused="two-call")
