"""Cutting encounters out of recorded clips (fot_encounters_extract, fidelity.extract_encounters), the part that needs no
GPU: the NumPy restatement of the whole chain (tests/encounters_common.py) and the package's own alignment against the
reference's answers (tests/golden/encounters), bit for bit; csrc/fot_encounter.hpp -- the checks, the candidate spans the
library's host code finds, the column walk, the compaction, the rank selection, the cruise speeds and the goals -- as a
stand-alone program (tests/emu/fot_encounter_emu.cpp) against the restatement, bit for bit, and the same program built with
-fsanitize=address,undefined; the C ABI's symbol and structures; fidelity_report's use of a carried recorded side.

The largest relative difference between the restatement's cruise speeds and goals and the reference's goes to the file
FOT_ENCOUNTERS_PROFILE names (expected: 0, the same NumPy operations)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import encounters_common as ec
import fidelity_common as fc
from conftest import ROOT
from integrated_path_planning_amd import _abi, batch, fidelity

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
EMU_SRCS = [os.path.join(EMU_DIR, "fot_encounter_emu.cpp"), os.path.join(CSRC, "fot_encounter.hpp"), os.path.join(CSRC, "fot_fidelity.hpp")]
MODES = (None, "median", "quantile", "freewalk")


@pytest.fixture(scope="module")
def fixture():
    return ec.load_fixture()


def _build(name, *flags):
    exe = os.path.join(EMU_DIR, "_build", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in EMU_SRCS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, EMU_SRCS[0]], check=True)
    return exe


def _runner(exe):
    def run(tmp_path, case, **kw):
        inp, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        ec.write_emu_case(inp, case["ped_xy"], case["ped_vel"], case["ego_xy"], case["ego_psi"], case["ego_vel"], case["dt"],
                          **dict(case["kw"], **kw))
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return ec.read_emu_out(outp)
    return run


@pytest.fixture(scope="module")
def emu():
    return _runner(_build("fot_encounter_emu", "-O2"))


def expected(case, **kw):
    return ec.expected_call(case["ped_xy"], case["ped_vel"], case["ego_xy"], case["ego_psi"], case["ego_vel"], case["dt"],
                            **dict(case["kw"], **kw))


def fixture_call(clip, **kw):
    ego_xy, ego_psi, ego_vel, dt = ec.align(clip)
    return ec.call(clip["name"], clip["ped_xy"], (ego_xy, ego_psi, ego_vel), dt=dt, ped_vel=clip.get("ped_vel"), **kw)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_the_abi_words_stay():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    assert hasattr(lib, "fot_encounters_extract"), "fot_encounters_extract not exported by libfot.so"
    assert "fot_encounters_extract" in _abi.SYMBOLS and re.search(r"\bint\s+fot_encounters_extract\s*\(", header)
    assert _abi.ABI_VERSION == 8 and re.search(r"#define FOT_ABI_VERSION 8\b", header)
    assert re.search(r"#define FOT_ABI_INFO_WORDS 35\b", header) and len(_abi.abi_expectation()) == 35
    for name, value in (("SHORT", 0), ("NO_PEDS", 1), ("FAR", 2), ("KEPT", 3), ("CRUISE_NONE", 0), ("CRUISE_MEDIAN", 1),
                        ("CRUISE_QUANTILE", 2), ("CRUISE_FREEWALK", 3), ("SCENE_DEVICE", 1), ("MEASURE_REAL", 2)):
        assert re.search(rf"#define FOT_ENC_{name} {value}\b", header), name
    assert (_abi.ENC_SHORT, _abi.ENC_NO_PEDS, _abi.ENC_FAR, _abi.ENC_KEPT) == (ec.SHORT, ec.NO_PEDS, ec.FAR, ec.KEPT)
    assert {k: v for k, v in _abi.ENC_CRUISE.items() if k != "none"} == ec.MODES


def test_ctypes_mirrors_of_the_structures_match_c(tmp_path):
    pairs = (("fot_encounter_params", _abi.EncounterParams), ("fot_encounter_span", _abi.EncounterSpan))
    lines = []
    for c_name, mirror in pairs:
        lines.append(f'  printf("%zu\\n", sizeof({c_name}));\n')
        lines += [f'  printf("%zu\\n", offsetof({c_name}, {n}));\n' for n, _ in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fot.h"\nint main(void) {\n' + "".join(lines) + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, mirror in pairs:
        want += [C.sizeof(mirror)] + [getattr(mirror, n).offset for n, _ in mirror._fields_]
    assert got == want
    assert batch.ENCOUNTER_SPAN_DT.itemsize == ec.SPAN_DT.itemsize == 80 and C.sizeof(_abi.EncounterParams) == 72
    assert list(batch.ENCOUNTER_SPAN_DT.names) == list(ec.SPAN_DT.names)
    assert [batch.ENCOUNTER_SPAN_DT.fields[n][1] for n in ec.SPAN_DT.names] == [ec.SPAN_DT.fields[n][1] for n in ec.SPAN_DT.names]


# ---- the restatement and the package's alignment against the reference ----------------------------------------------------------
def test_fixture_holds_every_outcome(fixture):
    clips, meta = fixture
    seen = {s[2] for per_vehicle in meta["statuses"].values() for spans in per_vehicle for s in spans}
    assert seen == {"KEPT", "SHORT", "NO_PEDS", "FAR"}
    assert clips["dut3"][0]["veh_xy"].shape[1] == 3 and clips["single"][0]["veh_xy"].shape[1] == 1
    assert "ped_vel" not in clips["nopsi"][0] and "veh_psi" not in clips["nopsi"][0]
    assert np.isnan(clips["single"][0]["veh_xy"][20:24]).all()
    total = sum(os.path.getsize(os.path.join(ec.GOLDEN_DIR, f)) for f in os.listdir(ec.GOLDEN_DIR))
    assert total < 200_000


@pytest.mark.parametrize("name", ("single", "nopsi", "dut3", "nobody"))
def test_alignment_equals_the_references(fixture, name):
    clip, ref = fixture[0][name]
    for label, got in (("restatement", ec.align(clip)), ("package", fidelity.align_vehicles(fidelity.RecordedClip(**clip)))):
        for k, g in zip(("ref_ego_xy", "ref_ego_psi", "ref_ego_vel"), got[:3]):
            assert ec.same(g, ref[k]), f"{label}: {k}"
        assert got[3] == float(ref["ref_dt"]), label
    dt = float(ref["ref_dt"])
    assert ec.same(ec.velocities(clip["ped_xy"], clip.get("ped_vel"), dt), ref["ref_ped_vel"])
    if clip.get("ped_vel") is None:
        assert ec.same(fidelity.fallback_velocities(clip["ped_xy"], dt), ref["ref_ped_vel"])


def test_alignment_edges():
    grid = np.arange(6) * 0.5
    t = np.array([2.0, 0.5, np.nan, 1.0, 1.5])
    v = np.array([4.0, 1.0, 9.0, np.nan, 3.0])
    for f in (ec.channel_on_grid, fidelity._onto_grid):
        got = f(t, v, grid)
        assert np.isnan(got[[0, 5]]).all() and got[1:5].tolist() == [1.0, 2.0, 3.0, 4.0]          # unsorted, a gap bridged
        assert np.isnan(f(t[:2], np.array([1.0, np.nan]), grid)).all()                             # fewer than two samples
        assert np.isfinite(f(np.array([0.0 + 5e-10, 2.5 - 5e-10]), np.array([0.0, 1.0]), grid)[[0, 5]]).all()   # the 1e-9 slack
        turn = f(np.array([0.0, 2.5]), np.array([3.1, -3.1]), grid, angular=True)                  # through pi, not through 0
        assert np.all(np.abs(turn) > 3.0)
    one = fidelity.RecordedClip("one", np.array([1.0]), np.zeros((1, 1, 2)), np.array([0]), np.array([0.0, 2.0]), np.zeros((2, 1, 2)),
                                np.array([0]))
    assert fidelity.align_vehicles(one)[3] == 0.4


def test_extraction_equals_the_references(fixture):
    clips, meta = fixture
    for name in meta["clips"]:
        clip, ref = clips[name]
        got = ec.extract([clip])
        assert [e["clip"] for e in got] == meta["encounters"][name]
        for i, e in enumerate(got):
            for f in ("times", "ego_xy", "ego_psi", "ego_vel", "ped_xy", "ped_vel", "ped_ids"):
                assert ec.same(e[f], ref[f"enc{i}_{f}"]), (name, i, f)
            assert e["min_separation"] == float(ref[f"enc{i}_min_separation"]) and e["dt"] == float(ref["ref_dt"])
        ego_xy, ego_psi, ego_vel, dt = ec.align(clip)
        spans = ec.candidate_spans(clip["ped_xy"], clip.get("ped_vel"), ego_xy, ego_psi, ego_vel, dt)
        want = [(k, s[0], s[1], s[2]) for k, per_vehicle in enumerate(meta["statuses"][name]) for s in per_vehicle]
        assert [(s["vehicle"], s["frame0"], s["frame1"], ec.STATUS_NAMES[s["status"]]) for s in spans] == want
    everything = [clips[n][0] for n in meta["clips"]]
    assert [e["clip"] for e in ec.extract(everything)] == meta["multivehicle"]
    assert [e["clip"] for e in ec.extract(everything, multivehicle=False)] == meta["single_vehicle_only"]


def test_boundary_conditions_equal_the_references(fixture):
    clips, meta = fixture
    worst = {}
    for name in meta["clips"]:
        clip, ref = clips[name]
        for i, e in enumerate(ec.extract([clip])):
            mine = {"cruise_median": ec.cruise_speeds(e["ego_xy"], e["ped_xy"], e["ped_vel"], "median"),
                    "cruise_q85": ec.cruise_speeds(e["ego_xy"], e["ped_xy"], e["ped_vel"], "quantile", 0.85),
                    "cruise_free": ec.cruise_speeds(e["ego_xy"], e["ped_xy"], e["ped_vel"], "freewalk", 0.5, 8.0),
                    "goals": ec.far_goals(e["ped_xy"], e["ped_vel"], 50.0)}
            for k, got in mine.items():
                worst[k] = max(worst.get(k, 0.0), ec.relative_difference(got, ref[f"enc{i}_{k}"]))
    print("largest relative difference to the reference:", worst)
    path = os.environ.get("FOT_ENCOUNTERS_PROFILE")
    if path:
        with open(path, "w") as f:
            json.dump({"restatement_vs_reference_largest_relative_difference": worst}, f)
    assert worst == {k: 0.0 for k in worst} and len(worst) == 4, worst


# ---- csrc/fot_encounter.hpp on the CPU ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("single", "nopsi", "dut3", "nobody"))
def test_emulation_equals_the_restatement_on_the_fixture(fixture, emu, tmp_path, name):
    clip, ref = fixture[0][name]
    for mode in MODES:
        case = fixture_call(clip, cruise=mode, cruise_q=ec.DEFAULT_Q.get(mode, 0.85))
        code, got = emu(tmp_path, case)
        assert code == 0
        ec.assert_call_matches(got, expected(case), f"{name} {mode}")
    # ... and so the reference's boundary conditions, through the header's arithmetic
    kept = [s for s in got["spans"] if s["status"] == ec.KEPT]
    for i, s in enumerate(kept):
        rows = slice(int(s["row_base"]), int(s["row_base"]) + int(s["n_ped"]))
        assert ec.same(got["cruise"][rows], ref[f"enc{i}_cruise_free"]) and ec.same(got["goals"][rows], ref[f"enc{i}_goals"])
        assert float(s["min_separation"]) == float(ref[f"enc{i}_min_separation"])


def test_emulation_equals_the_restatement_on_the_designed_calls(emu, tmp_path):
    for case in ec.edge_calls():
        for mode in MODES:
            code, got = emu(tmp_path, case, cruise=mode)
            assert code == 0
            ec.assert_call_matches(got, expected(case, cruise=mode), f"{case['label']} {mode}")
    code, got = emu(tmp_path, ec.edge_calls()[0], measure_real=False)
    assert code == 0 and got["series"].size == 0 and np.all(got["onset_step"] == -1)


def test_emulation_equals_the_restatement_on_the_fuzz(emu, tmp_path):
    calls = ec.fuzz_calls()
    counts = ec.call_status_counts(calls)
    assert counts[ec.KEPT] >= 0.1 * counts.sum() and np.all(counts > 0), counts
    for case in calls:
        code, got = emu(tmp_path, case)
        assert code == 0
        ec.assert_call_matches(got, expected(case), case["label"])


def test_emulation_refuses(emu, tmp_path):
    case = ec.edge_calls()[1]
    for kw in (dict(min_len=0), dict(min_sep_threshold=np.nan), dict(accel_threshold=np.nan), dict(max_distance=np.nan),
               dict(cruise="quantile", cruise_q=1.5), dict(cruise="freewalk", cruise_q=-0.1), dict(cruise="quantile", cruise_q=np.nan)):
        assert emu(tmp_path, case, **kw)[0] == 1, kw
    for dt in (0.0, -1.0, np.inf, np.nan):
        assert emu(tmp_path, dict(case, dt=dt))[0] == 1, dt


def test_emulation_under_sanitizers(tmp_path):
    run = _runner(_build("fot_encounter_emu_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for case in ec.edge_calls() + ec.fuzz_calls()[:8]:
        mode = case["kw"].get("cruise", "freewalk")
        code, got = run(tmp_path, case, cruise=mode)
        assert code == 0
        ec.assert_call_matches(got, expected(case, cruise=mode), case["label"])


# ---- the Python layer without a GPU ---------------------------------------------------------------------------------------------
class CountingEngine:
    """fidelity_eval by the restatement, counted"""

    def __init__(self):
        self.calls = 0

    def fidelity_eval(self, packed, accel_threshold=0.3, max_distance=5.0, interaction_distance=None):
        self.calls += 1
        encs, truth = [], None if packed.truth is None else []
        for i in range(packed.n):
            s0, s1, n = int(packed.step_off[i]), int(packed.step_off[i + 1]), int(packed.n_ped[i])
            r0 = int(sum((int(packed.step_off[j + 1]) - int(packed.step_off[j])) * int(packed.n_ped[j]) for j in range(i)))
            shape = (s1 - s0, n, 2)
            encs.append(dict(ego_xy=packed.ego[2 * s0:2 * s1].reshape(-1, 2), ped_xy=packed.ped[2 * r0:2 * r0 + 2 * shape[0] * n].reshape(shape),
                             dt=float(packed.dt[i])))
            if truth is not None:
                truth.append(packed.truth[2 * r0:2 * r0 + 2 * shape[0] * n].reshape(shape))
        rec, series, where, step, _ = fc.evaluate(encs, truth=truth, accel_threshold=accel_threshold, max_distance=max_distance,
                                                   interaction_distance=interaction_distance)
        return rec.astype(batch.FIDELITY_ENC_DT), series, where, step


def test_report_uses_a_carried_recorded_side(fixture):
    clips, meta = fixture
    encs = ec.extract([clips[n][0] for n in meta["clips"]])
    rng = np.random.default_rng(5)
    sims = [e["ped_xy"] + rng.normal(0.0, 0.2, e["ped_xy"].shape) for e in encs]
    plain = CountingEngine()
    want = fidelity.fidelity_report(plain, encs, sims)
    assert plain.calls == 2
    carried = []
    for e in encs:
        r, _, where, step, _, _ = fc.record(e["ego_xy"], e["ped_xy"], dt=e["dt"])
        carried.append(dict(e, real=dict(record=r.astype(batch.FIDELITY_ENC_DT), onset_dist=where, onset_step=step, **fidelity.REPORT_ONSET)))
    once = CountingEngine()
    got = fidelity.fidelity_report(once, carried, sims)
    assert once.calls == 1
    assert list(got) == list(want) and all(np.array_equal(got[k], want[k], equal_nan=True) for k in want)
    # a recorded side taken with other onset parameters, or missing from one encounter, is not used
    for spoil in (lambda c: dict(c, real=dict(c["real"], max_distance=4.0)), lambda c: dict(c, real=None)):
        again = CountingEngine()
        fidelity.fidelity_report(again, [spoil(carried[0])] + carried[1:], sims)
        assert again.calls == 2


def test_span_counts_are_the_librarys():
    for case in ec.edge_calls() + ec.fuzz_calls()[:10]:
        min_len = case["kw"].get("min_len", 5)
        want = expected(case)["spans"]
        if case["ped_xy"].shape[1] == 0:
            continue
        got = batch.encounter_span_counts(case["ego_xy"], case["ego_psi"], case["ego_vel"], min_len)
        assert got == (len(want), int(np.sum(want["frame1"] - want["frame0"] >= min_len))), case["label"]
