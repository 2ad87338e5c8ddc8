"""Sampler loops whose slots name their Social-GAN model (fot_loop_set_sampler_models), the part that needs no GPU: the
symbols; the unit tables of csrc/fot_sweep.hpp (sweep_model_tables, sweep_model_rows -- the code the host runs) against
prediction.model_scenes over named and fuzzed frames; one model against sweep_crowd_tables; numbers worked out by hand;
and the Python rules.

The C++ runs in a program of its own (tests/emu/fot_model_emu.cpp): built plainly and a second time with
-fsanitize=address,undefined, and run as it is (never loaded into Python).  The GPU leg is tests/test_gpu_loop_models.py."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import loop_crowd_common as cr
import loop_models_common as lm
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import SganSampler, crowd_scenes, model_scenes

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
NEW_SYMBOLS = ("fot_sgan_max_models", "fot_sgan_load_model", "fot_sgan_unload_model", "fot_sgan_sample_model",
               "fot_loop_set_sampler_models", "fot_debug_loop_sampler_shapes")


def test_library_exports_the_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _abi.SYMBOLS
        assert re.search(r"\b(int|int32_t)\s+%s\s*\(" % name, header)
    assert lib.fot_sgan_max_models() == 8
    assert _abi.ABI_VERSION == 8 and re.search(r"#define\s+FOT_ABI_VERSION\s+8\b", header)   # additions: the version stays
    for key in ("slot_model", "model_kinds"):
        assert key in inspect.signature(BatchPlanner.loop_set_sampler).parameters
    assert "slot_model" in inspect.signature(SganSampler.__init__).parameters
    assert hasattr(BatchPlanner, "debug_loop_sampler_shapes")
    # without a handle every entry answers FOT_ERR_INVALID
    assert lib.fot_sgan_load_model(None, 0, None, 0, None) == _abi.ERR_INVALID
    assert lib.fot_sgan_unload_model(None, 0) == _abi.ERR_INVALID
    assert lib.fot_sgan_sample_model(None, 0, 0, None, None, 1, None, 0, None, None) == _abi.ERR_INVALID
    assert lib.fot_loop_set_sampler_models(None, 1, 0, 1, None, 1, None, None) == _abi.ERR_INVALID
    assert lib.fot_debug_loop_sampler_shapes(None, 0, None, None) == _abi.ERR_INVALID


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def build(tag, flags):
    exe = os.path.join(EMU_DIR, "_build", "fot_model_emu_" + tag)
    srcs = [os.path.join(EMU_DIR, "fot_model_emu.cpp"), os.path.join(CSRC, "fot_sweep.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, srcs[0]], check=True)
    return exe


def all_frames():
    return dict(lm.FRAMES, **lm.fuzzed_frames(60, 20240613))


def run_lines(exe, lines, env=None):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    return [[int(v) for v in g.split()] for g in got], r


def run_cases(exe, env=None):
    frames = all_frames()
    got, r = run_lines(exe, [lm.case_line(*f) for f in frames.values()], env)
    for (name, f), answer in zip(frames.items(), got):
        assert answer == lm.expected_tables(*f), (name, f)
    return r


def test_tables_equal_model_scenes():
    """Interleaved crowds and models, slots with zero pedestrians, a unit whose lowest slot has ended, a model with no
    active unit, one model, eight models, and 60 fuzzed frames: sweep_model_tables and the gather table of
    sweep_model_rows print what prediction.model_scenes gives."""
    run_cases(build("o2", ["-O2"]))
    fuzz = lm.fuzzed_frames(60, 20240613).values()                    # the fuzz reaches the cases it is there for
    assert any(n_models > 1 + max([model[e] for e in running], default=0) for _, _, model, n_models, running in fuzz)
    assert any(0 in [P[e] for e in running] for P, _, _, _, running in fuzz)


def test_program_is_clean_under_address_and_undefined_sanitizers():
    # (the runtimes linked into the program itself: it runs as it is, whatever the environment preloads)
    exe = build("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-static-libubsan"])
    r = run_cases(exe, dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_one_model_reproduces_the_crowd_tables():
    """n_models = 1: the tables are sweep_crowd_tables' own, number for number, on every frame's crowds."""
    frames = all_frames()
    lines, crowd_lines = [], []
    for slot_P, crowd, _, _, running in frames.values():
        lines.append(lm.case_line(slot_P, crowd, [0] * len(crowd), 1, running))
        crowd_lines.append(" ".join(lines[-1].split()[:-1 - len(crowd)]).replace("models", "crowds", 1))
    got, _ = run_lines(build("o2", ["-O2"]), lines)
    want, _ = run_lines(build("o2", ["-O2"]), crowd_lines)
    for name, g, w, (slot_P, _, _, _, running) in zip(frames, got, want, frames.values()):
        rows = sum(slot_P[e] for e in running)
        assert g[:len(w) - rows] == w[:len(w) - rows], name             # shape, scene_off, scene_slot, scene_crowd, row_scene
        assert g[len(w) - rows:len(w)] == [0] * rows, name              # row_model
        assert g[len(w):len(w) + rows] == w[len(w) - rows:], name       # col


def test_tables_on_numbers_worked_out_by_hand():
    got, _ = run_lines(build("o2", ["-O2"]), [lm.case_line(*lm.FRAMES[k]) for k in (
        "interleaved, every slot running", "the lowest slot of a unit ended", "a model with no active unit")])
    # slots 0 .. 5: P 3 17 3 17 17 3, crowds 0 1 0 1 1 0, models 0 0 1 1 0 1.  Model 0: units (0, 0) = slot 0 and
    # (1, 0) = slots 1, 4; model 1: units (0, 1) = slots 2, 5 and (1, 1) = slot 3
    m0 = [2, 20, 0, 3, 20, 0, 1, 0, 1] + [0] * 3 + [1] * 17
    m1 = [2, 20, 0, 3, 20, 2, 3, 0, 1] + [0] * 3 + [1] * 17
    row_model = [0] * 3 + [0] * 17 + [1] * 3 + [1] * 17 + [0] * 17 + [1] * 3
    col = [0, 1, 2] + list(range(3, 20)) + [0, 1, 2] + list(range(3, 20)) * 2 + [0, 1, 2]
    assert got[0][:len(m0 + m1 + row_model + col)] == m0 + m1 + row_model + col
    assert got[0][len(m0 + m1 + row_model + col):][:4] == [0, 20, 0, 7 * 20] and got[0][-4:] == [1000, 20, 2, 1000 + 7 * 20 + 2]
    # slot 1 ended: slot 4 stands for unit (1, 0)
    assert got[1][:9] == [2, 20, 0, 3, 20, 0, 4, 0, 1]
    # slots 0, 1, 4 run: model 1 has no active unit
    assert got[2][:29] == m0 and got[2][29:32] == [0, 0, 0] and got[2][32:32 + 37] == [0] * 37


# ---- prediction.model_scenes -----------------------------------------------------------------------------------------------------------
def test_model_scenes_of_one_model_is_crowd_scenes():
    for name, (slot_P, crowd, _, _, running) in all_frames().items():
        counts = [slot_P[e] for e in running]
        units, row_model, cols = model_scenes(running, counts, [4] * len(running), crowd, [0] * len(crowd))
        crowds, rep, noise_slots, want_cols = crowd_scenes(running, counts, [4] * len(running), crowd)
        assert len(units) == 1 and all(list(a) == list(b) for a, b in zip(units[0], (crowds, rep, noise_slots))), name
        assert list(cols) == list(want_cols) and not row_model.any() and cols.dtype == np.int64, name


def test_model_scenes_refusals():
    with pytest.raises(ValueError, match="one crowd and one model per slot"):
        model_scenes([0], [3], [0], [0, 0], [0])
    with pytest.raises(ValueError, match="slot_model names 2 slots"):
        model_scenes([0, 2], [3, 3], [0, 0], [0, 0], [0, 1])
    with pytest.raises(ValueError, match="one model id >= 0"):
        model_scenes([0, 1], [3, 3], [0, 0], [0, 0], [0, -1])
    with pytest.raises(ValueError, match="slots 0 and 2 of crowd 0 differ"):                # two slots of one unit
        model_scenes([0, 1, 2], [3, 17, 4], [5, 5, 5], [0, 1, 0], [1, 0, 1])
    model_scenes([0, 1, 2], [3, 17, 4], [5, 5, 6], [0, 1, 0], [1, 0, 0])                     # (units of their own: no comparison)


# ---- the constructor --------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    w0, w1 = lm.weights(lm.POOLED), lm.weights(lm.NO_POOLING)
    ok = dict(counter_seed=1, slot_crowd=[0, 0, 1], slot_model=[0, 1, 1])
    s = SganSampler(None, [w0, w1], lm.S, **ok)
    assert s.slot_model.tolist() == [0, 1, 1] and s.models == [w0, w1] and s.weights is w0
    assert s.model_kinds == [_abi.NOISE_GAUSSIAN, _abi.NOISE_GAUSSIAN]
    uni = lm.weights(lm.PER_SCENE, noise_type="uniform")
    assert SganSampler(None, (w0, uni), lm.S, **ok).model_kinds == [_abi.NOISE_GAUSSIAN, _abi.NOISE_UNIFORM_SYM]
    for missing in ok:
        with pytest.raises(ValueError, match="several models need counter_seed, slot_crowd and slot_model"):
            SganSampler(None, [w0, w1], lm.S, **{k: v for k, v in ok.items() if k != missing})
    with pytest.raises(ValueError, match="noise_type is each model's own"):
        SganSampler(None, [w0, w1], lm.S, noise_type="uniform", **ok)
    with pytest.raises(ValueError, match="1 .. 8 models"):
        SganSampler(None, [], lm.S, **ok)
    with pytest.raises(ValueError, match="1 .. 8 models"):
        SganSampler(None, [w0] * 9, lm.S, **ok)
    with pytest.raises(ValueError, match="model id in 0 .. 1"):
        SganSampler(None, [w0, w1], lm.S, **dict(ok, slot_model=[0, 2, 1]))
    with pytest.raises(ValueError, match="model id in 0 .. 1"):
        SganSampler(None, [w0, w1], lm.S, **dict(ok, slot_model=[0, -1, 1]))
    with pytest.raises(ValueError, match="one entry per slot"):
        SganSampler(None, [w0, w1], lm.S, **dict(ok, slot_model=[0, 1]))
    with pytest.raises(ValueError, match="share obs_len and pred_len"):
        SganSampler(None, [w0, lm.weights(lm.NO_POOLING, pred_len=3)], lm.S, **ok)
    with pytest.raises(ValueError, match='Unrecognized noise type "cauchy"'):
        SganSampler(None, [w0, lm.weights(lm.NO_POOLING, noise_type="cauchy")], lm.S, **ok)
    with pytest.raises(ValueError, match="weights is then a sequence"):                     # a single SganWeights stays what it is
        SganSampler(None, w0, lm.S, **ok)
    one = SganSampler(None, w0, lm.S, counter_seed=1, slot_crowd=[0, 0])
    assert one.models is None and one.slot_model is None and one.model_kinds is None
    with pytest.raises(ValueError, match="loads them when it joins"):
        s.load(w1)
    assert cr.S == lm.S
