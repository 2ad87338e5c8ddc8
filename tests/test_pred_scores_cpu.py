"""Prediction scores (fot_prediction_scores / fot_loop_prediction_scores), the part that needs no GPU: the NumPy
restatement (tests/pred_scores_common.py) against the reference fixture, unit origins and whole episodes; the arithmetic of
csrc/fot_predscore.hpp -- the code the kernel runs -- built with gcc as a stand-alone program, against the restatement;
the C ABI's symbols and record layouts; the Python keyword's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from closed_loop_common import OracleEngine, OracleResampler, scripted_sample_source
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from pred_scores_common import (FIXTURE, FLAG_NLL, METRIC_KEYS, RECORD_DT, assert_metrics_match_reference,
                                assert_records_close, fold, layouts, load_cases, origin_terms, random_origin, unit_case,
                                unit_metrics, write_emu_cases)

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_EXE = os.path.join(EMU_DIR, "_build", "fot_predscore_emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
UNITS = ("s1", "s2", "s64", "p1", "p33", "p65", "p300_e1", "p90_e12", "e1_stride1", "e12_stride4", "tail", "offset100",
         "identical_s4", "identical_but_one", "bw_floor_mixed", "logp_floor_mixed", "picks_differ", "ade_fde_differ")
EPISODES = ("s6_eps02", "s4_eps0", "s5_best_only", "weave_s5", "weave_s4")


@pytest.fixture(scope="module")
def fix():
    return load_cases()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_prediction_score_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for sym in ("fot_prediction_scores", "fot_loop_prediction_scores"):
        assert hasattr(lib, sym), f"{sym} not exported by libfot.so"
        assert sym in _abi.SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} not declared in include/fot.h"
    assert "sizeof(fot_pred_score)" in _abi.ABI_WORD_NAMES and "sizeof(fot_pred_origin)" in _abi.ABI_WORD_NAMES
    assert _abi.ABI_VERSION == 8 and re.search(r"#define FOT_ABI_VERSION 8\b", header)


def test_ctypes_mirrors_of_the_score_structures_match_c(tmp_path):
    lines = []
    for c_name, mirror in (("fot_pred_score", _abi.PredScore), ("fot_pred_origin", _abi.PredOrigin)):
        lines.append(f'  printf("%zu\\n", sizeof({c_name}));\n')
        lines += [f'  printf("%zu\\n", offsetof({c_name}, {n}));\n' for n, _ in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fot.h"\nint main(void) {\n' + "".join(lines)
                   + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for mirror in (_abi.PredScore, _abi.PredOrigin):
        want += [C.sizeof(mirror)] + [getattr(mirror, n).offset for n, _ in mirror._fields_]
    assert got == want
    assert C.sizeof(_abi.PredScore) == 56 == RECORD_DT.itemsize and C.sizeof(_abi.PredOrigin) == 32
    assert [n for n, _ in _abi.PredScore._fields_] == list(RECORD_DT.names)


def test_the_keyword_is_refused_where_it_cannot_work():
    """Before any engine is built: no sample source, a resident loop; a stand-in engine without the entry point."""
    with pytest.raises(ValueError, match="sample_source"):
        BatchedClosedLoop({}, [], prediction_scores=True)
    with pytest.raises(ValueError, match="resident=False"):
        BatchedClosedLoop({}, [], prediction_scores=True, resident=True)
    with pytest.raises(ValueError, match="library's own engine"):
        BatchedClosedLoop({}, [], prediction_scores=True, sample_source=lambda a, b: None, engine=object())
    with pytest.raises(ValueError, match="resident=True"):                  # summaries keeps its meaning
        BatchedClosedLoop({}, [], summaries=True)


# ---- the restatement against the reference --------------------------------------------------------------------------------
def test_fixture_holds_what_the_tests_need(fix):
    meta = fix["meta"]
    assert tuple(meta["keys"]) == METRIC_KEYS
    assert set(meta["units"]) == set(UNITS) and tuple(meta["episodes"]) == EPISODES
    eps = [meta["episodes"][n] for n in EPISODES]
    # (s4_eps0: the reference run collides after 45 steps, before a 48-step horizon completes -- the NaN / 0 answer)
    assert all(e["reference"]["nll_eval_count"] > 0 for n, e in zip(EPISODES, eps) if n != "s4_eps0")
    short = meta["episodes"]["s4_eps0"]
    assert short["steps"] < 48 and short["reference"]["ade_eval_count"] == 0 and np.isnan(short["reference"]["nll"])
    assert any(e["reference"]["ade_per_agent"] < e["reference"]["ade"] for e in eps)
    assert sum(e["log_p_floored"] for e in eps) > 0 and sum(e["log_p_free"] for e in eps) > 0
    assert 0.0 < meta["nll_atol"] < 1e-6                                 # far below any value it is added to
    assert os.path.getsize(FIXTURE) < 850_000                            # the largest fixture committed before it


@pytest.mark.parametrize("name", UNITS)
def test_restatement_matches_the_reference_on_unit_origins(fix, name):
    dense, truth, stride, want = unit_case(fix, name)
    rec = origin_terms(dense, truth, stride)
    assert_metrics_match_reference(unit_metrics(rec), want, fix["meta"]["nll_atol"], name)
    assert bool(rec["flags"] & FLAG_NLL) == (want["nll_eval_count"] > 0)


def _host_loop_records(cfg, tracks, n_samples):
    """The episode free-running on the oracle-backed stand-ins with the scripted sample source; per step the distribution
    the loop recorded, scored by the restatement."""
    src = scripted_sample_source(n_samples, cfg["pred_len"])
    sim = BatchedClosedLoop(cfg, [tracks], engine=OracleEngine(cfg), resampler=OracleResampler(cfg), sample_source=src)
    stride, E = int(round(0.4 / cfg["dt"])), int(cfg["pred_len"])
    records = []
    for _ in range(int(cfg["total_time"] / cfg["dt"])):
        if sim.step() == 0:
            break
        d = sim._score_dist
        if d is not None and d.shape[2] > stride * E - 1:
            rows = np.minimum(sim.frame + stride * np.arange(1, E + 1), len(tracks) - 1)
            records.append((int(sim.step_counts[0]) - 1, origin_terms(d, tracks[rows].transpose(1, 0, 2), stride)))
    return records, int(sim.step_counts[0]), stride, E


@pytest.mark.parametrize("name", EPISODES)
def test_restatement_matches_the_reference_on_whole_episodes(fix, name):
    """Per-origin terms + the deferred fold against the reference's own calculate_aggregate_metrics dictionary."""
    ep = fix["meta"]["episodes"][name]
    records, L, stride, E = _host_loop_records(dict(ep["config"]), fix[name + "_ped_traj"], ep["n_samples"])
    assert L == ep["steps"]
    assert_metrics_match_reference(fold(records, L, stride, E), ep["reference"], fix["meta"]["nll_atol"], name)


# ---- csrc/fot_predscore.hpp on the CPU ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    srcs = [os.path.join(EMU_DIR, "fot_predscore_emu.cpp"), os.path.join(CSRC, "fot_predscore.hpp")]
    if not os.path.exists(EMU_EXE) or os.path.getmtime(EMU_EXE) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(EMU_EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EMU_EXE, srcs[0]], check=True)

    def run(cases, tmp_path):
        inp, outp = str(tmp_path / "cases.bin"), str(tmp_path / "records.bin")
        write_emu_cases(inp, cases)
        subprocess.run([EMU_EXE, inp, outp], check=True)
        return np.fromfile(outp, dtype=RECORD_DT)
    return run


def test_emulation_matches_the_restatement_on_unit_origins(fix, emu, tmp_path):
    """Both layouts, both element types, skip 0 / 1; a float32 block is held to the restatement fed the rounded values."""
    cases, want, labels = [], [], []
    for name in UNITS:
        dense, truth, stride, _ = unit_case(fix, name)
        for t_major in (False, True):
            for skip in (0, 1):
                for dt in (np.float64, np.float32):
                    cases.append((layouts(dense, t_major, skip, dt), truth, stride, t_major, skip))
                    want.append(origin_terms(dense.astype(dt), truth, stride))
                    labels.append(f"{name} t_major={t_major} skip={skip} {np.dtype(dt).name}")
    got = emu(cases, tmp_path)
    assert len(got) == len(want)
    for g, w, label in zip(got, want, labels):
        assert_records_close(g, w, label)


def test_emulation_matches_the_restatement_on_random_origins(emu, tmp_path):
    rng = np.random.default_rng(77)
    cases, want = [], []
    for i in range(300):
        dense, truth, stride = random_origin(rng)
        t_major, skip = bool(i & 1), (i >> 1) & 1
        dt = np.float32 if i % 5 == 0 else np.float64
        cases.append((layouts(dense, t_major, skip, dt), truth, stride, t_major, skip))
        want.append(origin_terms(dense.astype(dt), truth, stride))
    got = emu(cases, tmp_path)
    n_nll = n_skipped = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert_records_close(g, w, f"random origin {i}")
        n_nll += bool(w["flags"] & FLAG_NLL)
        n_skipped += not (w["flags"] & FLAG_NLL)
    assert n_nll > 100 and n_skipped > 10
