"""Sampler loops whose slots share crowds (fot_loop_set_sampler_shared), the part that needs no GPU: the symbols; the crowd
tables and the consistency check of csrc/fot_sweep.hpp -- the code the host runs -- against a NumPy restatement
(loop_crowd_common); prediction.crowd_scenes against the same restatement; and the Python rules.

The C++ runs in a program of its own (tests/emu/fot_crowd_emu.cpp): built plainly and a second time with
-fsanitize=address,undefined, and run as it is (never loaded into Python).  The GPU leg is tests/test_gpu_loop_crowd_sampler.py."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import loop_crowd_common as cr
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import SganSampler, crowd_scenes

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")


def test_library_exports_the_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for name in ("fot_loop_set_sampler_shared", "fot_debug_loop_sampler_shape"):
        assert hasattr(lib, name) and name in _abi.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert _abi.ABI_VERSION == 8 and re.search(r"#define\s+FOT_ABI_VERSION\s+8\b", header)   # additions: the version stays
    assert "row_slot = crowd id" in header                            # the noise key, where fot_sgan_noise is described
    assert "slot_crowd" in inspect.signature(BatchPlanner.loop_set_sampler).parameters
    assert "slot_crowd" in inspect.signature(SganSampler.__init__).parameters


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def build(tag, flags):
    exe = os.path.join(EMU_DIR, "_build", "fot_crowd_emu_" + tag)
    srcs = [os.path.join(EMU_DIR, "fot_crowd_emu.cpp"), os.path.join(CSRC, "fot_sweep.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, srcs[0]], check=True)
    return exe


# name -> (pedestrian count of every slot, crowd of every slot, running slots)
SIX = [3, 17, 3, 17, 17, 3]
INTERLEAVED = [0, 1, 0, 1, 1, 0]
TABLE_CASES = {
    "every slot running": (SIX, INTERLEAVED, [0, 1, 2, 3, 4, 5]),
    "the first slot of a crowd ended": (SIX, INTERLEAVED, [1, 2, 3, 4, 5]),
    "the first slots of both crowds ended": (SIX, INTERLEAVED, [2, 4, 5]),
    "a crowd wholly ended": (SIX, INTERLEAVED, [1, 3, 4]),
    "the other crowd wholly ended": (SIX, INTERLEAVED, [2, 5]),
    "one slot left": (SIX, INTERLEAVED, [4]),
    "a crowd of no pedestrians": ([0, 5, 0, 5, 2], [1, 0, 1, 0, 2], [0, 1, 2, 3, 4]),
    "a crowd of no pedestrians, alone": ([0, 5, 0, 5, 2], [1, 0, 1, 0, 2], [0, 2]),
    "ids that are not dense": ([4, 4, 9, 9, 1], [7, 7, 40, 40, 2], [0, 1, 2, 3, 4]),
    "ids that are not dense, descending": ([4, 9, 4, 9, 1], [900, 40, 900, 40, 2], [0, 1, 2, 3, 4]),
    "blocks, not interleaved": ([3, 3, 3, 17, 17], [0, 0, 0, 1, 1], [0, 1, 2, 3, 4]),
    "one slot per crowd": ([3, 17, 1, 33], [0, 1, 2, 3], [0, 1, 2, 3]),
    "one slot per crowd, a slot ended": ([3, 17, 1, 33], [0, 1, 2, 3], [0, 2, 3]),
    "one slot per crowd, crowds reversed": ([3, 17, 1], [2, 1, 0], [0, 1, 2]),
    "no slot running": (SIX, INTERLEAVED, []),
}


def table_cases():
    out = []
    for name, (slot_P, crowd, running) in TABLE_CASES.items():
        counts = [slot_P[e] for e in running]
        t = cr.crowd_tables(counts, running, crowd)
        line = "tables %d %s %s %d %s" % (len(running), " ".join(map(str, counts)), " ".join(map(str, running)), len(crowd),
                                          " ".join(map(str, crowd)))
        want = [len(t["scene_slot"]), t["scene_off"][-1], int(t["identity"])] + t["scene_off"] + t["scene_slot"] + t["scene_crowd"] \
            + t["row_scene"] + t["col"]
        out.append((" ".join(line.split()), " ".join(map(str, want))))
    return out


def consistency_inputs():
    """name -> (counts, frames, crowds, pos [n_frames_max, sum P, 2], expected (code, a, b))."""
    rng = np.random.default_rng(5)
    counts, frames, crowd = [3, 17, 3, 17], [6, 6, 6, 6], [0, 1, 0, 1]
    a, b = rng.normal(0.0, 10.0, (6, 3, 2)), rng.normal(0.0, 10.0, (6, 17, 2))
    equal = np.concatenate([a, b, a, b], axis=1)
    cases = {"equal crowds": (counts, frames, crowd, equal, (0, -1, -1))}
    cases["a differing count"] = ([3, 17, 3, 16], frames, crowd, equal[:, :-1], (1, 1, 3))
    cases["a differing n_frames"] = (counts, [6, 6, 5, 6], crowd, equal, (2, 0, 2))
    off = equal.copy()
    off[5, 3 + 17 + 3 + 16, 1] = np.nextafter(off[5, 3 + 17 + 3 + 16, 1], np.inf)      # one ulp, the last frame, the last pedestrian
    cases["one differing coordinate in the last frame"] = (counts, frames, crowd, off, (3, 1, 3))
    held = equal.copy()
    held[4:, 3 + 17:3 + 17 + 3] += 1.0                                # frames a slot never replays do not count
    cases["a difference past the recorded frames"] = (counts, [4, 6, 4, 6], crowd, held, (0, -1, -1))
    zero = equal.copy()
    zero[2, 0, 0], zero[2, 20, 0] = 0.0, -0.0                         # bytes, not values
    cases["zero against minus zero"] = (counts, frames, crowd, zero, (3, 0, 2))
    cases["one slot per crowd"] = (counts, [6, 5, 4, 3], [3, 2, 1, 0], off, (0, -1, -1))
    return cases


def consistency_cases():
    out = []
    for name, (counts, frames, crowd, pos, want) in consistency_inputs().items():
        assert cr.crowds_consistent(counts, frames, crowd, pos) == want, name
        line = "consistent %d %s %s %s %d %s" % (len(counts), " ".join(map(str, counts)), " ".join(map(str, frames)),
                                                 " ".join(map(str, crowd)), len(pos), " ".join(float(v).hex() for v in pos.reshape(-1)))
        out.append((line, "%d %d %d" % want))
    return out


def run_cases(exe, env=None):
    cases = table_cases() + consistency_cases()
    r = subprocess.run([exe], input="\n".join(c[0] for c in cases) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for (line, want), answer in zip(cases, got):
        assert answer.split() == want.split(), (line[:200], answer[:200], want[:200])
    return r


def test_tables_and_consistency_equal_the_restatement():
    """Crowds of 3 and 17 pedestrians, their slots interleaved: every slot running, the first slot of a crowd ended (its
    representative moves), a crowd wholly ended, a crowd without pedestrians, ids that are not dense, one slot per crowd;
    the consistency check on equal crowds, a differing count, a differing n_frames and one coordinate off by one ulp in
    the last frame."""
    run_cases(build("o2", ["-O2"]))


def test_program_is_clean_under_address_and_undefined_sanitizers():
    # (the runtimes linked into the program itself: it runs as it is, whatever the environment preloads)
    exe = build("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-static-libubsan"])
    r = run_cases(exe, dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_restated_table_properties():
    """The restatement itself, on numbers worked out by hand."""
    t = cr.crowd_tables(SIX, [0, 1, 2, 3, 4, 5], INTERLEAVED)
    assert t["scene_off"] == [0, 3, 20] and t["scene_slot"] == [0, 1] and t["scene_crowd"] == [0, 1] and not t["identity"]
    assert t["col"] == [0, 1, 2] + list(range(3, 20)) + [0, 1, 2] + list(range(3, 20)) * 2 + [0, 1, 2]
    t = cr.crowd_tables([17, 3, 17, 17, 3], [1, 2, 3, 4, 5], INTERLEAVED)                  # slot 0 ended: slot 2 stands for crowd 0
    assert t["scene_slot"] == [2, 1] and t["scene_off"] == [0, 3, 20]
    t = cr.crowd_tables([17, 17, 17], [1, 3, 4], INTERLEAVED)                             # crowd 0 ended
    assert t["scene_slot"] == [1] and t["scene_crowd"] == [1] and t["col"] == list(range(17)) * 3
    t = cr.crowd_tables([0, 5, 0, 5, 2], [0, 1, 2, 3, 4], [1, 0, 1, 0, 2])                 # crowd 1 has no pedestrians: no scene
    assert t["scene_crowd"] == [0, 2] and t["scene_slot"] == [1, 4] and t["col"] == [0, 1, 2, 3, 4] * 2 + [5, 6]
    t = cr.crowd_tables([3, 17, 1, 33], [0, 1, 2, 3], [0, 1, 2, 3])                        # one slot per crowd: today's step
    assert t["identity"] and t["scene_off"] == [0, 3, 20, 21, 54] and t["scene_slot"] == [0, 1, 2, 3]
    assert t["row_scene"] == [0] * 3 + [1] * 17 + [2] + [3] * 33 and t["col"] == list(range(54))
    assert not cr.crowd_tables([3, 17, 1], [0, 1, 2], [2, 1, 0])["identity"]              # (the crowds' order is not the slots')


# ---- prediction.crowd_scenes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_crowd_scenes_equals_the_restatement(name):
    slot_P, crowd, running = TABLE_CASES[name]
    counts = [slot_P[e] for e in running]
    t = cr.crowd_tables(counts, running, crowd)
    crowds, rep, noise_slots, cols = crowd_scenes(running, counts, [11] * len(running), crowd)
    assert list(crowds) == t["scene_crowd"] == list(noise_slots)
    assert [running[i] for i in rep] == t["scene_slot"]
    assert list(cols) == t["col"] and cols.dtype == np.int64


def test_crowd_scenes_refuses_slots_that_disagree():
    with pytest.raises(ValueError, match="slots 0 and 2 of crowd 0 differ"):
        crowd_scenes([0, 1, 2], [3, 17, 4], [5, 5, 5], [0, 1, 0])
    with pytest.raises(ValueError, match="slots 1 and 3 of crowd 1 differ"):
        crowd_scenes([0, 1, 3], [3, 17, 17], [5, 5, 6], [0, 1, 0, 1])
    with pytest.raises(ValueError, match="slot_crowd names 2 slots"):
        crowd_scenes([0, 2], [3, 3], [0, 0], [0, 0])
    crowd_scenes([0, 2], [3, 0], [5, 6], [0, 1, 0])                     # (a slot without pedestrians is in no scene)


def test_slot_crowd_needs_the_counter_mode():
    with pytest.raises(ValueError, match="slot_crowd .* needs counter_seed"):
        SganSampler(None, cr.weights(), cr.S, slot_crowd=[0, 0])
    with pytest.raises(ValueError, match="one crowd id >= 0 per slot"):
        SganSampler(None, cr.weights(), cr.S, counter_seed=1, slot_crowd=[0, -1])
    s = SganSampler(None, cr.weights(), cr.S, counter_seed=1, slot_crowd=[0, 1, 0])
    assert s.slot_crowd.tolist() == [0, 1, 0] and SganSampler(None, cr.weights(), cr.S, counter_seed=1).slot_crowd is None
