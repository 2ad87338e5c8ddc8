"""Footprint re-verification (fot_footprint_recheck, fot_loop_footprint_*), the part that needs no GPU: the NumPy restatement
(tests/footprint_obs_common.py) against the reference's own answers (tests/golden/footprint_obs/cases.npz) bit for bit;
csrc/fot_footprint_obs.hpp -- the geometry, the checks, the step values, the heading scan and the fold the library runs -- as
a stand-alone program (tests/emu/fot_footprint_obs_emu.cpp) against the restatement, also built with
-fsanitize=address,undefined; the scan's chunk carry at widths 1, 2 and 256; both sides of every strict `<`; the C ABI's
symbols and structures; the Python layer on a stand-in engine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import footprint_obs_common as fc
from conftest import ROOT
from integrated_path_planning_amd import _abi, safety

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_EXE = os.path.join(EMU_DIR, "_build", "fot_footprint_obs_emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
EMU_SRCS = [os.path.join(EMU_DIR, "fot_footprint_obs_emu.cpp"), os.path.join(CSRC, "fot_footprint_obs.hpp")]
RECHECK_FROM_RECORD = ("legacy_min_dist", "legacy_collision_steps", "multi_min_dist", "multi_clearance", "multi_violation_steps",
                       "rect_min_surface_dist", "rect_clearance", "rect_violation_steps")
OBS_FROM_RECORD = ("legacy_min_dist", "multi_clearance", "multi_violation_steps", "rect_clearance", "rect_violation_steps")


@pytest.fixture(scope="module")
def fix():
    return fc.load_cases()


def case_of(fix, name):
    return fc.golden_case(fix, fix["meta"]["cases"][name]["inputs"])


def rows_of(records, keys):
    return np.array([[float(r[k]) for k in keys] for r in records]).reshape(len(records), len(keys))


@pytest.fixture(scope="module")
def restated(fix):
    """name -> (stored-yaw records, series, reconstructed-yaw records or None, series) of the restatement, computed once"""
    out = {}
    for name, info in fix["meta"]["cases"].items():
        case = case_of(fix, name)
        stored = fc.recheck(case, info["geom"])
        recon = fc.recheck(case, info["geom"], reconstruct=True) if np.all(np.diff(case["step_off"]) >= 2) else None
        for a in stored + (recon or ()):
            a.setflags(write=False)
        out[name] = (stored, recon)
    return out


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fot_footprint_recheck", "fot_loop_footprint_enable", "fot_loop_footprint_obs")


def test_library_exports_the_entry_points_and_the_abi_words_stay():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} not exported by libfot.so"
        assert sym in _abi.SYMBOLS and re.search(r"\bint\s+" + sym + r"\s*\(", header)
    assert _abi.ABI_VERSION == 8 and re.search(r"#define FOT_ABI_VERSION 8\b", header)
    assert re.search(r"#define FOT_ABI_INFO_WORDS 35\b", header) and len(_abi.abi_expectation()) == 35


def test_ctypes_mirrors_of_the_structures_match_c(tmp_path):
    pairs = (("fot_footprint_geom", _abi.FootprintGeom), ("fot_footprint_step", _abi.FootprintStep),
             ("fot_footprint_obs", _abi.FootprintObs))
    lines = []
    for c_name, mirror in pairs:
        lines.append(f'  printf("%zu\\n", sizeof({c_name}));\n')
        lines += [f'  printf("%zu\\n", offsetof({c_name}, {n}));\n' for n, _ in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fot.h"\nint main(void) {\n' + "".join(lines)
                   + '  printf("%d\\n", FOT_MAX_CIRCLES);\n  return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, mirror in pairs:
        want += [C.sizeof(mirror)] + [getattr(mirror, n).offset for n, _ in mirror._fields_]
    assert got == want + [8]
    assert np.dtype(_abi.FootprintObs).itemsize == fc.RECORD_DT.itemsize == 64
    assert [n for n, _ in _abi.FootprintObs._fields_] == list(fc.RECORD_DT.names)
    assert [n for n, _ in _abi.FootprintStep._fields_] == list(fc.STEP_DT.names)


# ---- the restatement against the reference: the same NumPy operations, bit for bit ----------------------------------------
def test_fixture_holds_what_the_tests_need(fix):
    meta = fix["meta"]
    assert os.path.getsize(fc.GOLDEN) < 220 * 1024
    assert set(meta["episodes"]) == {"base", "rnd3", "walls", "turn"} and meta["margin"] == 1e-9
    counts = meta["episode_counts"]
    assert sum(counts["base"]) > 0 and sum(counts["rnd3"]) > 0
    synth = fc.golden_case(fix, "synth")
    pops = np.diff(synth["ped_off"])
    assert pops.min() == 0 and pops.max() >= 12 and meta["cases"]["synth"]["M"] > 80.0
    assert not fix["synth_moving"].all() and fix["synth_moving"].any()
    steps = np.diff(synth["step_off"])
    assert 2 in steps and 3 in steps and not fix["synth_moving"][synth["step_off"][-2]:].any()      # one never moves
    for g in ("legacy", "multi", "rect"):
        for side in ("at", "below", "above"):
            assert meta["cases"][f"thr_{g}_{side}"]["exempt"]


def test_circle_cover_equals_the_references(fix):
    for n, want in fix["meta"]["cover"].items():
        off, radius = fc.circle_cover(4.5, 2.0, int(n))
        assert off.tolist() == want["offsets"] and radius == want["radius"]


def test_restatement_equals_the_reference_bit_for_bit(fix, restated):
    for name in fix["meta"]["cases"]:
        (rec, series, _), recon = restated[name]
        got = np.stack([series["legacy"], series["multi"], series["rect"]], axis=1)
        assert got.tobytes() == fix[name + "_series"].tobytes(), f"{name}: per-step values"
        assert rows_of(rec, RECHECK_FROM_RECORD).tobytes() == fix[name + "_recheck_stored"].tobytes(), f"{name}: recheck, stored yaw"
        assert rows_of(rec, OBS_FROM_RECORD).tobytes() == fix[name + "_obs"].tobytes(), f"{name}: observational metrics"
        case = case_of(fix, name)
        for lo, hi in zip(case["step_off"][:-1], case["step_off"][1:]):
            if hi - lo < 2:
                continue
            x, y = case["xy"][lo:hi, 0], case["xy"][lo:hi, 1]
            assert fc.reconstruct_heading(x, y).tobytes() == fix[name + "_yaw_recon"][lo:hi].tobytes(), f"{name}: heading"
            assert np.array_equal(fc.heading_terms(x, y)[2], fix[name + "_moving"][lo:hi])
        if recon is not None:
            assert rows_of(recon[0], RECHECK_FROM_RECORD).tobytes() == fix[name + "_recheck_recon"].tobytes(), f"{name}: recheck, reconstructed"


# ---- csrc/fot_footprint_obs.hpp on the CPU -----------------------------------------------------------------------------------
def _build(exe, *flags):
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in EMU_SRCS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, EMU_SRCS[0]], check=True)
    return exe


def _runner(exe):
    def run(tmp_path, case, geom=None, **kw):
        inp, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        fc.write_emu_case(inp, case, geom, **kw)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return fc.read_emu_out(outp)
    return run


@pytest.fixture(scope="module")
def emu():
    return _runner(_build(EMU_EXE, "-O2"))


def test_emulation_matches_the_restatement_on_the_fixture(fix, restated, emu, tmp_path):
    """Within the derived bound everywhere; bit for bit where every heading is 0 (cos = 1, sin = 0: every operation exact or
    the same single rounding on both sides); counts and the moving mask equal."""
    worst = 0.0
    for name, info in fix["meta"]["cases"].items():
        case, tol = case_of(fix, name), fc.dist_tol(info["M"])
        (rec, series, _), recon = restated[name]
        code, g_rec, g_series, g_yaw, _, off, radius = emu(tmp_path, case, info["geom"])
        assert code == 0 and g_yaw.tobytes() == case["yaw"].tobytes()
        n = dict(fc.DEFAULT_GEOM, **info["geom"])
        want_off, want_r = fc.circle_cover(n["vehicle_length"], n["vehicle_width"], n["n_circles"])
        assert off[:len(want_off)].tobytes() == want_off.tobytes() and radius == want_r
        worst = max(worst, fc.assert_series_close(g_series, series, tol, name), fc.assert_records_close(g_rec, rec, tol, name))
        if not np.any(case["yaw"]):
            assert g_series.tobytes() == series.tobytes() and g_rec.tobytes() == rec.tobytes(), f"{name}: yaw = 0 is exact"
        if recon is not None:
            code, g_rec, g_series, g_yaw, g_moving, _, _ = emu(tmp_path, case, info["geom"], reconstruct=True)
            assert code == 0
            fc.assert_close(g_yaw, recon[2], fc.YAW_TOL, f"{name}: heading")
            if not info["exempt"]:
                assert np.array_equal(g_moving, fix[name + "_moving"]), f"{name}: moving mask"
            fc.assert_records_close(g_rec, recon[0], tol, name + " reconstructed")
    assert worst <= fc.dist_tol(100.0)


@pytest.mark.parametrize("geometry", ("legacy", "multi", "rect"))
def test_both_sides_of_every_strict_comparison(fix, emu, tmp_path, geometry):
    """The reference's value is the threshold, one ulp below it, one ulp above it: 0, 1, 0 steps, and the same bytes."""
    col = {"legacy": "legacy_collision_steps", "multi": "multi_violation_steps", "rect": "rect_violation_steps"}[geometry]
    counts = []
    for side in ("at", "below", "above"):
        name = f"thr_{geometry}_{side}"
        info = fix["meta"]["cases"][name]
        code, rec, series, _, _, _, _ = emu(tmp_path, case_of(fix, name), info["geom"])
        want = fc.recheck(case_of(fix, name), info["geom"])
        assert code == 0 and rec.tobytes() == want[0].tobytes() and series.tobytes() == want[1].tobytes()
        counts.append(int(rec[0][col]))
    assert counts == [0, 1, 0]


def test_the_moving_comparison_at_its_threshold(fix, emu, tmp_path):
    """dx = v exactly, dy = 0, v = 1e-4 and its neighbours: only the upper neighbour moves; a standing step 1 holds step
    0's heading (pi / 2), a moving one has heading 0."""
    got = {}
    for side in ("at", "below", "above"):
        name = f"moving_{side}"
        code, _, _, yaw, moving, _, _ = emu(tmp_path, case_of(fix, name), reconstruct=True)
        assert code == 0 and np.array_equal(moving, fix[name + "_moving"])
        fc.assert_close(yaw, fix[name + "_yaw_recon"], fc.YAW_TOL, name)
        got[side] = (bool(moving[1]), float(yaw[1]))
    assert [got[s][0] for s in ("at", "below", "above")] == [False, False, True]
    assert got["above"][1] == 0.0 and abs(got["at"][1] - np.pi / 2) <= fc.YAW_TOL


def test_the_scans_chunk_carry_at_widths_1_2_and_256(emu, tmp_path):
    case = fc.scan_case()
    want = fc.recheck(case, reconstruct=True)[2]
    outs = []
    for width in (1, 2, 256, 7, 64):
        code, _, _, yaw, moving, _, _ = emu(tmp_path, case, reconstruct=True, chunk=width)
        assert code == 0
        fc.assert_close(yaw, want, fc.YAW_TOL, f"chunk width {width}")
        for lo, hi in zip(case["step_off"][:-1], case["step_off"][1:]):
            assert np.array_equal(moving[lo:hi], fc.heading_terms(case["xy"][lo:hi, 0], case["xy"][lo:hi, 1])[2])
        outs.append(yaw.tobytes())
    assert all(o == outs[0] for o in outs), "the heading depends on the chunk width"
    off = case["step_off"]
    assert not moving[250:263].any() and moving[249] and moving[263]     # a standstill of steps 250 .. 262, across 256
    assert np.all(yaw[250:263] == yaw[249])
    assert int(np.argmax(moving[off[1]:off[2]])) == 1 and yaw[off[1]] == yaw[off[1] + 1]       # a lead-in of 1 step
    assert int(np.argmax(moving[off[2]:off[3]])) == 300                                        # ... and of 300 steps
    assert np.all(yaw[off[2]:off[2] + 300] == yaw[off[2] + 300])
    assert not moving[off[3]:off[4]].any() and not yaw[off[3]:off[4]].any()                    # never moves: zeros


REFUSALS = [("length_0", dict(geom=dict(vehicle_length=0.0))), ("width_negative", dict(geom=dict(vehicle_width=-1.0))),
            ("radius_negative", dict(geom=dict(ped_radius=-0.1))), ("legacy_negative", dict(geom=dict(legacy_radius=-1.0))),
            ("circles_0", dict(geom=dict(n_circles=0))), ("circles_9", dict(geom=dict(n_circles=9))),
            ("step_off_from_1", dict(step_off=[1, 3])), ("step_off_decreasing", dict(step_off=[0, 3, 2])),
            ("no_step", dict(step_off=[0, 3, 3])), ("one_step_no_yaw", dict(step_off=[0, 1, 3], reconstruct=True)),
            ("ped_off_from_1", dict(ped_off=[1, 1, 1, 1])), ("ped_off_decreasing", dict(ped_off=[0, 2, 1, 2])),
            ("n_traj_negative", dict(n_traj=-1))]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_emulation_refuses_what_the_library_refuses(emu, tmp_path, name, change):
    rng = np.random.default_rng(3)
    x, y, heading = fc.drive(rng, 3)
    case = fc.make_case([(x, y, heading, fc.crowd_near(rng, x, y, [1, 0, 1]))])
    if "step_off" in change:
        case["step_off"] = np.asarray(change["step_off"], np.int32)
    if "ped_off" in change:
        case["ped_off"] = np.asarray(change["ped_off"], np.int32)
    got = emu(tmp_path, case, change.get("geom"), reconstruct=change.get("reconstruct", False), n_traj=change.get("n_traj"))
    assert got[0] == 1
    # ... and a one-step trajectory WITH its yaw is served
    if name == "one_step_no_yaw":
        assert emu(tmp_path, case)[0] == 0


def test_emulation_runs_clean_under_address_and_undefined_sanitizers(fix, emu, tmp_path):
    """Stand-alone, built with -fsanitize=address,undefined (-fno-sanitize-recover: a finding ends the run): fixture cases,
    the scan at several widths, a trajectory without pedestrians, eight circles, and a refusal -- the plain build's bytes."""
    san = _runner(_build(EMU_EXE + "_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-static-libasan", "-static-libubsan"))
    synth, scan = case_of(fix, "synth"), fc.scan_case()
    bad = dict(synth, step_off=np.array([0, 3, 2], np.int32))
    cases = [((synth,), {}), ((synth, {"n_circles": 8}), dict(reconstruct=True)), ((case_of(fix, "ep_turn"),), dict(reconstruct=True)),
             ((scan,), dict(reconstruct=True, chunk=1)), ((scan,), dict(reconstruct=True, chunk=2)), ((scan,), dict(reconstruct=True)),
             ((case_of(fix, "thr_rect_at"), fix["meta"]["cases"]["thr_rect_at"]["geom"]), {}), ((bad,), {})]
    for args, kw in cases:
        a, b = san(tmp_path, *args, **kw), emu(tmp_path, *args, **kw)
        assert a[0] == b[0]
        if a[0] == 0:
            assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a[1:], b[1:]))
    assert a[0] == 1


# ---- the Python layer on a stand-in engine ----------------------------------------------------------------------------------
class RestatedEngine:
    """``BatchPlanner.footprint_recheck`` on the restatement: what the Python layer hands over, and how often."""

    def __init__(self):
        self.calls = []

    def footprint_recheck(self, geom, step_off, xy, yaw, ped_off, ped_xy, want_series=False, want_yaw=False):
        self.calls.append(dict(n=len(step_off) - 1, reconstruct=yaw is None))
        g = dict(vehicle_length=geom.vehicle_length, vehicle_width=geom.vehicle_width, n_circles=geom.n_circles,
                 ped_radius=geom.ped_radius, legacy_radius=geom.legacy_radius)
        case = dict(step_off=np.asarray(step_off), xy=np.asarray(xy), yaw=yaw, ped_off=np.asarray(ped_off), ped_xy=np.asarray(ped_xy))
        rec, series, used = fc.recheck(case, g, reconstruct=yaw is None)
        return rec, (series if want_series else None), (used if want_yaw else None)


def test_footprint_geometry_defaults_and_refusals():
    g = safety.footprint_geometry()
    assert (g.vehicle_length, g.vehicle_width, g.n_circles, g.ped_radius, g.legacy_radius) == (4.5, 2.0, 3, 0.2, 1.0 + 0.2)
    g = safety.footprint_geometry({"n_circles": 5, "ped_radius": 0.3, "ego_radius": 1.1})
    assert g.n_circles == 5 and g.legacy_radius == 1.1 + 0.3
    assert safety.footprint_geometry({"legacy_radius": 2.0}).legacy_radius == 2.0
    with pytest.raises(ValueError, match="unknown keys"):
        safety.footprint_geometry({"length": 4.5})


def test_recheck_npz_sends_all_files_through_one_call_and_returns_the_references_rows(fix, tmp_path):
    case = case_of(fix, "synth")
    paths = []
    for t, (lo, hi) in enumerate(zip(case["step_off"][:-1], case["step_off"][1:])):
        if hi - lo < 2:
            continue
        obj = np.empty(hi - lo, dtype=object)
        for i in range(lo, hi):
            obj[i - lo] = case["ped_xy"][case["ped_off"][i]:case["ped_off"][i + 1]]
        d = tmp_path / f"run_{t}"
        d.mkdir()
        np.savez(d / "trajectory.npz", ego_x=case["xy"][lo:hi, 0], ego_y=case["xy"][lo:hi, 1], ego_yaw=case["yaw"][lo:hi],
                 ped_positions=obj, min_distances=fix["synth_series"][lo:hi, 0])
        paths.append(d / "trajectory.npz")
    eng = RestatedEngine()
    rows = safety.recheck_npz(eng, paths)
    assert eng.calls == [dict(n=len(paths), reconstruct=False)]
    cols = fix["meta"]["recheck_cols"]
    for t, row in enumerate(rows):
        assert list(row)[:3] == ["run", "steps", "yaw_source"] and row["run"] == f"run_{t}" and row["yaw_source"] == "stored"
        assert [float(row[k]) for k in cols] == fix["synth_recheck_stored"][t].tolist()
        finite = np.isfinite(fix["synth_series"][case["step_off"][t]:case["step_off"][t + 1], 0]).all()
        assert row["stored_vs_recomputed_maxdiff"] == 0.0 if finite else np.isnan(row["stored_vs_recomputed_maxdiff"])
    eng = RestatedEngine()
    rows = safety.recheck_npz(eng, paths, yaw="reconstruct")
    assert eng.calls == [dict(n=len(paths), reconstruct=True)]
    assert [[float(r[k]) for k in cols] for r in rows] == fix["synth_recheck_recon"].tolist()
    assert all(r["yaw_source"] == "reconstructed" for r in rows)
    with pytest.raises(ValueError, match="stored"):
        safety.footprint_recheck(eng, [], yaw="held")


def test_a_stand_in_engine_refuses_the_keyword():
    from closed_loop_common import OracleEngine, load_episodes, scenario_config
    from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
    ep = load_episodes()
    cfg = scenario_config(ep["meta"], "base")
    with pytest.raises(ValueError, match="footprint_obs"):
        BatchedClosedLoop(cfg, [ep["base_ped_traj"]], engine=OracleEngine(cfg), footprint_obs=True)
