"""Sweep loops (fot_loop_begin_sweep, fot_loop_set_samples_shared), the part that needs no GPU: the two symbols; the
layout arithmetic of csrc/fot_sweep.hpp -- the code the sweep forms of the selection and block kernels and the host run --
against a NumPy restatement, past 2^31 points on offsets alone; and the Python rules.

The arithmetic runs in a program of its own (tests/emu/fot_sweep_emu.cpp): built plainly and a second time with
-fsanitize=address,undefined, and run as it is (never loaded into Python).  The GPU leg is tests/test_gpu_loop_sweep.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import loop_sweep_common as sw
from closed_loop_common import load_episodes, scenario_config
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import COMMON_FIELDS, BatchedClosedLoop, merge_configs, scenario_key, _Cfg
from integrated_path_planning_amd.prediction import RecordedSamples

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
DIST, REP = sw.DIST, sw.REP


def test_library_exports_the_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for name in ("fot_loop_begin_sweep", "fot_loop_set_samples_shared"):
        assert hasattr(lib, name) and name in _abi.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert _abi.ABI_VERSION == 8 and re.search(r"#define\s+FOT_ABI_VERSION\s+8\b", header)   # additions: the version stays
    assert (sw.DIST, sw.REP) == (0, 1) and re.search(r"#define\s+FOT_LOOP_PLAN_REPRESENTATIVE\s+1\b", header)


# ---- the arithmetic of fot_sweep.hpp ------------------------------------------------------------------------------------------------
def build(tag, flags):
    exe = os.path.join(EMU_DIR, "_build", "fot_sweep_emu_" + tag)
    srcs = [os.path.join(EMU_DIR, "fot_sweep_emu.cpp"), os.path.join(CSRC, "fot_sweep.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, srcs[0]], check=True)
    return exe


COUNTS = (0, 1, 33, 65, 30)
MODES = {"all distribution": [DIST] * 5, "all representative": [REP] * 5, "alternating": [DIST, REP, DIST, REP, DIST],
         "alternating, representative first": [REP, DIST, REP, DIST, REP]}
RUNNING = ([0, 1, 2, 3, 4], [1, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 3], [1, 3], [3], [0])


def layout_cases():
    """(input line, expected answer) of every layout case."""
    out = []
    for modes in MODES.values():
        for slots in RUNNING:
            counts = [COUNTS[e] for e in slots]
            for S, T, select_all in ((6, 51, False), (1, 2, True), (64, 256, False)):
                end = sw.dist_end(counts, S, T)
                out.append((counts, slots, modes, end, T, select_all))
    # past 2^31 points: three episodes of a million pedestrians at S = 64 and 51 time entries -- offsets only
    big = [1_000_000, 1_000_000, 999_999]
    for modes in ([REP, REP, REP], [DIST, REP, REP], [REP, DIST, REP]):
        out.append((big, [0, 1, 2], modes, sw.dist_end(big, 64, 51), 51, False))
        out.append((big, [2, 0, 1], modes, 2 ** 40 + 7, 256, True))
    lines = []
    for counts, slots, modes, end, T, select_all in out:
        size, off, sel = sw.layout(counts, slots, modes, end, T, select_all)
        line = "layout %d %d %d %d %s %s %d %s" % (len(counts), end, T, int(select_all), " ".join(map(str, counts)),
                                                   " ".join(map(str, slots)), len(modes), " ".join(map(str, modes)))
        lines.append((line, " ".join([str(size)] + ["%d %d" % (o, s) for o, s in zip(off, sel)])))
    return lines


def column_cases():
    own = list(np.cumsum((0,) + COUNTS)[:-1])
    tables = {"own": (own, sum(COUNTS)), "shared": ([0] * 5, 65), "overlapping": ([0, 3, 10, 5, 20], 70),
              "reversed": ([129, 128, 95, 30, 0], 129), "one short": (own, sum(COUNTS) - 1), "negative": ([0, 0, -1, 0, 0], 200),
              "no columns": ([0] * 5, 0)}
    lines = []
    for name, (col0, n_rec) in tables.items():
        for slots in RUNNING:
            counts = [COUNTS[e] for e in slots]
            fit = sw.columns_fit(COUNTS, col0, n_rec)
            assert fit == (name not in ("one short", "negative", "no columns")), name
            line = "columns %d %s %s %d %s %s %d" % (len(slots), " ".join(map(str, counts)), " ".join(map(str, slots)), len(COUNTS),
                                                     " ".join(map(str, COUNTS)), " ".join(map(str, col0)), n_rec)
            want = "1 " + " ".join(map(str, sw.columns(counts, slots, col0))) if fit else "0"
            lines.append((line.replace("  ", " "), want.strip()))
    return lines


def capacity_cases():
    return [("capacity %d %d %d" % (S, n, T), str((S + 1) * n * T)) for S, n, T in ((1, 1, 2), (20, 1920, 51), (64, 2 ** 24, 256))]


def run_cases(exe, env=None):
    cases = layout_cases() + column_cases() + capacity_cases()
    r = subprocess.run([exe], input="\n".join(c[0] for c in cases) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for (line, want), answer in zip(cases, got):
        assert answer.split() == want.split(), (line[:200], answer[:200], want[:200])
    return r


def test_layout_and_columns_equal_the_restatement():
    """Pedestrian counts (0, 1, 33, 65, 30) under all-distribution, all-representative and alternating modes, with every
    slot running and with the first, a middle and the last slot dropped; offsets beyond 2^31 points (computed, nothing
    allocated); the column table for own, shared, overlapping and reversed slot_col0 and the three range refusals."""
    some = dict(layout_cases())
    assert any(int(w.split()[0]) > 2 ** 31 for w in some.values())
    run_cases(build("o2", ["-O2"]))


def test_program_is_clean_under_address_and_undefined_sanitizers():
    # (the runtimes linked into the program itself: it runs as it is, whatever the environment preloads)
    exe = build("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-static-libubsan"])
    r = run_cases(exe, dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_restated_layout_properties():
    """The restatement itself: the planning blocks follow the distribution blocks without a gap, in frame order; an
    episode without pedestrians takes no room; select_all selects everything and moves nothing."""
    counts, slots = list(COUNTS), [0, 1, 2, 3, 4]
    end = sw.dist_end(counts, 6, 51)
    size, off, sel = sw.layout(counts, slots, MODES["alternating, representative first"], end, 51)
    assert off == [end, -1, end, -1, end + 33 * 51] and sel == [1, 0, 1, 0, 1] and size == end + (33 + 30) * 51
    assert sw.layout(counts, slots, MODES["all distribution"], end, 51) == (end, [-1] * 5, [0] * 5)
    assert sw.layout(counts, slots, MODES["all distribution"], end, 51, True) == (end, [-1] * 5, [1] * 5)
    assert sw.layout(counts, slots, MODES["all representative"], end, 51)[0] == end + sum(counts) * 51


# ---- the Python rules ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meta():
    return load_episodes()["meta"]


def test_the_plan_mode_is_an_episodes_own(meta):
    base = scenario_config(meta)
    assert "distribution_aware_planning" not in dict(COMMON_FIELDS)
    aware = dict(base, distribution_aware_planning=True)
    distinct, slot, per = merge_configs([base, aware, base])
    assert len(distinct) == 1 and list(slot) == [0, 0, 0]              # the same scenario, another mode
    assert scenario_key(_Cfg(base)) == scenario_key(_Cfg(aware))
    assert [bool(getattr(c, "distribution_aware_planning", False)) for c in per] == [False, True, False]
    for name, value in (("chance_epsilon", 0.2), ("collision_margin_inflation", 1.25)):
        distinct, slot, _ = merge_configs([aware, dict(aware, **{name: value})])
        assert len(distinct) == 2 and list(slot) == [0, 1], name


def test_forms_that_take_one_configuration_keep_their_refusals(meta):
    base = scenario_config(meta)
    aware = dict(base, distribution_aware_planning=True)
    tracks = [np.zeros((40, 2, 2))] * 2
    rec = lambda: RecordedSamples(np.zeros((4, 3, base["pred_len"], 4, 2)))
    one = "the five-call step, stand-in engines and sample sources take one configuration"
    # mixed modes or scenarios outside the one-call step with samples in device memory
    for kw in (dict(sample_source=rec()), dict(sample_source=rec(), device_samples=True, fused=False),
               dict(sample_source=rec(), device_samples=True, engine=object()),
               dict(sample_source=rec(), device_samples=True, resampler=object())):
        with pytest.raises(ValueError, match=one):
            BatchedClosedLoop([base, aware], tracks, **kw)
        with pytest.raises(ValueError, match=one):
            BatchedClosedLoop([aware, dict(aware, chance_epsilon=0.2)], tracks, **kw)
    with pytest.raises(ValueError, match="summaries=True with a sampler"):
        BatchedClosedLoop([base, aware], tracks, sample_source=rec(), device_samples=True, resident=True, summaries=True)
    with pytest.raises(ValueError, match="plan_on_representative_sample needs device_samples=True"):
        BatchedClosedLoop([base, base], tracks, sample_source=rec(), plan_on_representative_sample=True)
    # a distribution-aware episode needs a multi-sample predictor, wherever it stands in the list
    with pytest.raises(ValueError, match="distribution_aware_planning needs a multi-sample predictor"):
        BatchedClosedLoop([dict(base, prediction_method="cv"), dict(aware, prediction_method="cv")], tracks)


def test_recorded_samples_slot_col0(meta):
    L = 3
    samples = np.arange(5 * 2 * L * 7 * 2, dtype=np.float64).reshape(5, 2, L, 7, 2)
    ped_off = [0, 3, 3, 7, 9]                                          # slots of 3, 0, 4 and 2 pedestrians
    ok = RecordedSamples(samples, slot_col0=[0, 6, 3, 5])
    ok.attach(ped_off, L, False)                                        # (7 columns serve 9 pedestrians)
    RecordedSamples(samples, slot_col0=[4, 7, 0, 0]).attach(ped_off, L)    # a slot without pedestrians may name the end
    for bad, slot in (([0, 0, 4, 0], 2), ([5, 0, 0, 0], 0), ([0, 0, 0, -1], 3), ([0, 8, 0, 0], 1)):
        with pytest.raises(ValueError, match=f"slot {slot} reads columns"):
            RecordedSamples(samples, slot_col0=bad).attach(ped_off, L)
    with pytest.raises(ValueError, match="slot_col0 names 3 slots"):
        RecordedSamples(samples, slot_col0=[0, 0, 0]).attach(ped_off, L)
    with pytest.raises(ValueError, match="7 pedestrian columns, the tracks 9"):
        RecordedSamples(samples).attach(ped_off, L)                     # without the map the sum counts, as before
    # the stepwise call cuts its rows through the same map the library's table holds
    for slots in ([0, 1, 2, 3], [2, 3], [3, 0], [1]):
        counts = [ped_off[e + 1] - ped_off[e] for e in slots]
        cols = sw.columns(counts, slots, [0, 6, 3, 5])
        off = np.concatenate([[0], np.cumsum(counts)])
        got = ok.sample(None, off, slots=slots, steps=np.full(len(slots), 2))
        assert got.shape == (2, L, len(cols), 2) and np.array_equal(got, samples[2][:, :, cols])
    shared = RecordedSamples(samples[:, :, :, :4], slot_col0=[0, 0, 0, 0])
    shared.attach([0, 4, 8, 12, 16], L, False)
    got = shared.sample(None, None, slots=[0, 1, 2, 3], steps=[1, 1, 1, 1])
    assert np.array_equal(got, np.concatenate([samples[1][:, :, :4]] * 4, axis=2))
