"""Episode summary metrics of the resident loop (fot_loop_summary_enable / fot_loop_summaries), the part that needs no
GPU: the C ABI's symbols and the record's layout; the NumPy restatement of the definition (tests/summary_common.py) held
to the reference fixture on episodes run with the oracle-backed stand-ins; and the ring / totals / truncated-tail
arithmetic of csrc/fot_summary.hpp -- the code the kernels run -- against a direct evaluation of the definition."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from closed_loop_common import OracleEngine, OracleResampler, load_episodes, scenario_config
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from summary_common import (assert_summary_matches_reference, load_summaries, reference_summary, summary_of_history)

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SHIM_SO = os.path.join(EMU_DIR, "_build", "libfot_summary_emu.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
EXISTING = ("base", "fast", "shift", "walls", "turn", "footprint", "inflate", "rnd0", "rnd1", "rnd2", "rnd3", "rnd4", "rnd5")
WEAVE = ("weave0", "weave1", "weave2", "weave3", "weave_short")


def test_library_exports_the_summary_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for sym in ("fot_loop_summary_enable", "fot_loop_summaries"):
        assert hasattr(lib, sym), f"{sym} not exported by libfot.so"
        assert sym in _abi.SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} not declared in include/fot.h"
    assert "sizeof(fot_loop_summary)" in _abi.ABI_WORD_NAMES


def test_ctypes_mirror_of_the_summary_record_matches_c(tmp_path):
    fields = [n for n, _ in _abi.LoopSummary._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fot.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(fot_loop_summary));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(fot_loop_summary, {n}));\n' for n in fields) + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.LoopSummary)] + [getattr(_abi.LoopSummary, n).offset for n in fields]
    assert got[0] % 8 == 0
    # every key of the reference's dictionary is a field
    assert set(BatchedClosedLoop.SUMMARY_KEYS) <= set(fields)


def test_summaries_need_a_resident_loop():
    """The keyword is refused before any engine is built where the loop is not resident."""
    with pytest.raises(ValueError, match="resident=True"):
        BatchedClosedLoop({}, [], summaries=True)


# ---- the restatement against the reference ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures():
    return load_episodes(), load_summaries()


def test_fixture_holds_what_the_tests_need(fixtures):
    episodes, fix = fixtures
    meta = fix["meta"]
    assert tuple(meta["keys"]) == BatchedClosedLoop.SUMMARY_KEYS
    assert tuple(meta["int_keys"]) == BatchedClosedLoop.SUMMARY_INT_KEYS
    assert set(meta["variants"]) == set(EXISTING) | set(WEAVE) and tuple(meta["weave"]) == WEAVE
    for name in EXISTING:                                          # the same runs as the per-step fixture
        assert meta["variants"][name]["steps"] == episodes["meta"]["variants"][name]["steps"]
        assert meta["variants"][name]["termination"] == episodes["meta"]["variants"][name]["termination"]
    for name in WEAVE:                                             # far above the comparison's tolerance
        s = reference_summary(fix, name)
        assert s["ade_eval_count"] > 0 and s["ade"] > 1e-2 and s["planning_ade"] > 1e-2
    assert {meta["variants"][n]["scenario"] for n in WEAVE} == {"scenario_01", "scenario_02", "scenario_03"}
    short = meta["variants"]["weave_short"]
    assert short["n_frames"] < short["steps"]                      # the recording ends first: its last frame is held
    fast = reference_summary(fix, "fast")                          # stops before the first complete standard horizon
    assert np.isnan(fast["ade"]) and fast["ade_eval_count"] == 0 and fast["pred_samples"] == 0
    assert fast["planning_eval_count"] > 0 and np.isnan(fast["nll"])
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_summary_episodes.npz"))
    assert size < os.path.getsize(os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_cv_episodes.npz"))


def _config_and_tracks(fixtures, name):
    episodes, fix = fixtures
    if name in WEAVE:
        return dict(fix["meta"]["variants"][name]["config"]), fix[name + "_ped_traj"]
    return scenario_config(episodes["meta"], name), episodes[name + "_ped_traj"]


@pytest.mark.parametrize("name", EXISTING + WEAVE)
def test_restatement_matches_the_reference(fixtures, name):
    """The episode free-running on the oracle-backed stand-ins, summarised by tests/summary_common.py, against the
    reference's calculate_aggregate_metrics of its own run; for base also the prefixes of 60 and 100 steps."""
    _, fix = fixtures
    cfg, tracks = _config_and_tracks(fixtures, name)
    sim = BatchedClosedLoop(cfg, [tracks], engine=OracleEngine(cfg), resampler=OracleResampler(cfg))
    hist = list(sim.run()[0])
    v = fix["meta"]["variants"][name]
    assert len(hist) == v["steps"] and sim.episodes[0].termination_reason == v["termination"]
    kw = dict(dt=cfg["dt"], sgan_dt=v["sgan_dt"], pred_len=v["pred_len"], num_samples=cfg.get("num_samples", 1))
    assert_summary_matches_reference(summary_of_history(hist, **kw), reference_summary(fix, name), name)
    for n in fix["meta"]["prefixes"].get(name, ()):
        assert_summary_matches_reference(summary_of_history(hist[:n], **kw), reference_summary(fix, name, n), f"{name}[:{n}]")


def test_restatement_of_an_empty_history_and_a_bad_ratio():
    s = summary_of_history([], 0.1, 0.4, 12)
    assert s["min_dist"] == 0.0 and s["min_ttc"] == float("inf") and s["max_jerk"] == 0.0 and s["mean_accel"] == 0.0
    assert np.isnan(s["ade"]) and np.isnan(s["planning_ade"]) and s["ade_eval_count"] == 0 and s["pred_samples"] == 0
    with pytest.raises(ValueError):
        summary_of_history([], 0.15, 0.4, 12)


# ---- the ring arithmetic the kernels run --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(EMU_DIR, "fot_summary_emu.cpp"), os.path.join(CSRC, "fot_summary.hpp")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SHIM_SO, srcs[0]], check=True)
    L = C.CDLL(SHIM_SO)
    vp = C.c_void_p
    L.summary_stride_of.argtypes = [C.c_double, C.c_double]
    L.summary_ring_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]
    return L


def _direct(rows, P, L, n_dense, stride, pred_len):
    """The definition, origin by origin over the whole history of L steps (fot.h, fot_loop_summary)."""
    tot = [0.0, 0.0, 0.0, 0.0]
    n_std = n_plan = 0
    for i in range(L):
        if P[i] <= 0:
            continue
        E = min(n_dense, L - (i + 1))
        if E > 0:
            s = 0.0
            for k in range(E):
                s += rows[i, k]
            tot[2] += s / E
            tot[3] += rows[i, E - 1]
            n_plan += int(P[i])
        if n_dense > stride * pred_len - 1 and i + stride * pred_len < L:
            s = 0.0
            for j in range(1, pred_len + 1):
                s += rows[i, stride * j - 1]
            tot[0] += s / pred_len
            tot[1] += rows[i, stride * pred_len - 1]
            n_std += int(P[i])
    nan = float("nan")
    return [tot[0] / n_std if n_std else nan, tot[1] / n_std if n_std else nan, tot[2] / n_plan if n_plan else nan,
            tot[3] / n_plan if n_plan else nan, float(n_std), float(n_plan)]


def test_ring_fold_equals_the_definition(shim):
    """Random episode lengths, horizons, strides and rows (some steps without a prediction): a summary taken from the ring
    at any length -- mid-run, the run then continued -- equals the definition evaluated directly on the first L steps.
    Both add the same terms in the same order, so the comparison is exact."""
    rng = np.random.default_rng(2024)
    cases = [(1, 1, 1, 5), (3, 2, 2, 9), (50, 4, 12, 274), (50, 4, 12, 41), (49, 4, 12, 130), (47, 4, 12, 100), (8, 3, 2, 0)]
    for _ in range(60):
        n_dense = int(rng.integers(1, 40))
        stride = int(rng.integers(1, 6))
        pred_len = int(rng.integers(1, 10))
        cases.append((n_dense, stride, pred_len, int(rng.integers(0, 4 * n_dense + 3))))
    n_std_seen = n_trunc_seen = 0
    for n_dense, stride, pred_len, L in cases:
        rows = rng.uniform(0.0, 3.0, (max(L, 1), n_dense))
        P = rng.integers(1, 9, max(L, 1)).astype(np.int32)
        P[rng.random(len(P)) < 0.15] = 0
        at = np.unique(np.concatenate([[0, L], rng.integers(0, L + 1, 6)])).astype(np.int32)
        out = np.zeros((len(at), 6))
        assert shim.summary_ring_run(n_dense, stride, pred_len, L, rows.ctypes.data, P.ctypes.data, len(at), at.ctypes.data,
                                     out.ctypes.data) == len(at)
        for j, l_at in enumerate(at):
            want = _direct(rows, P, int(l_at), n_dense, stride, pred_len)
            np.testing.assert_array_equal(out[j], want, err_msg=f"n_dense {n_dense} stride {stride} pred_len {pred_len} L {l_at}")
            n_std_seen += want[4] > 0
            n_trunc_seen += 0 < l_at < n_dense
    assert n_std_seen > 20 and n_trunc_seen > 20


def test_stride_is_the_reference_rule(shim):
    assert shim.summary_stride_of(0.4, 0.1) == 4 and shim.summary_stride_of(0.4, 0.2) == 2
    assert shim.summary_stride_of(0.4, 0.4) == 1 and shim.summary_stride_of(0.4, 0.05) == 8
    for sgan_dt, dt in ((0.4, 0.15), (0.4, 0.3), (0.1, 0.4), (0.4, 0.25)):
        assert shim.summary_stride_of(sgan_dt, dt) == 0, (sgan_dt, dt)
