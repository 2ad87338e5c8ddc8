"""The flat form of the evaluation walk against the general lean form, on the host (tests/emu/fot_flatframe_emu.cpp).

The program walks every candidate of every case in both forms -- in one piece and in 2 and 3 time segments, in both
forms of the step bookkeeping -- and compares what the walk hands on bit for bit.  Cases: every golden on an exactly
straight path that is lean-eligible, every case of tests/flatframe_common.py, and the non-finite egos.  Two builds:

  fused      -DFOT_HOST_FMA under the front end's contraction rule with hardware FMA (the ROCm clang, the compiler of
             the device code: -ffp-contract=on -mfma) -- the general form contracts as it does on the device, the
             flat form's FOT_FMA is one rounding.  Needs that compiler and an FMA-capable CPU.
  unfused    g++ -ffp-contract=off without FOT_HOST_FMA: every product and sum rounded on its own in both forms.
             The identities hold there too (each dropped operation is a multiplication by one or an addition of zero).

The fused build is also made with -fsanitize=address,undefined and run as a plain executable.
"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import flatframe_common as ff
from conftest import Golden, golden_names
from helpers import request_from_golden
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest
from integrated_path_planning_amd.params import make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "fot_flatframe_emu.cpp"), os.path.join(EMU_DIR, "fot_emu.cpp"),
           os.path.join(CSRC, "fot_math.hpp"), os.path.join(CSRC, "fot_setup.hpp"), os.path.join(CSRC, "fot_types.h"),
           os.path.join(ROOT, "include", "fot.h")]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def cpu_has_fma():
    try:
        return bool(re.search(r"\bfma\b", open("/proc/cpuinfo").read()))
    except OSError:
        return False


FUSED = os.path.exists(CLANG) and cpu_has_fma()
BUILDS = {"unfused": ["g++", "-O2", "-std=c++17", "-ffp-contract=off"]}
if FUSED:
    BUILDS["fused"] = [CLANG, "-O2", "-std=c++17", "-ffp-contract=on", "-mfma", "-DFOT_HOST_FMA"]
    BUILDS["fused-sanitized"] = [CLANG, "-O1", "-g", "-std=c++17", "-ffp-contract=on", "-mfma", "-DFOT_HOST_FMA",
                                 "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
else:
    BUILDS["unfused-sanitized"] = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=undefined"]


def build(tag):
    exe = os.path.join(EMU_DIR, "_build", "fot_flatframe_emu_" + tag)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in SOURCES):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([*BUILDS[tag], "-o", exe, SOURCES[0]], check=True)
    return exe


def pack_case(name, kw, waypoints, req):
    """one case of the program's file: planner, knots, ego, obstacles (float64; a single-track tensor as one sample)"""
    params = make_params(**kw)
    pb = PackedBatch([PlanRequest(**{**req.__dict__, "scenario": 0})])
    wx, wy = (np.ascontiguousarray(w, np.float64) for w in waypoints)
    out = [name.encode()[:63].ljust(64, b"\0"), struct.pack("<i", C.sizeof(params)), bytes(params),
           struct.pack("<i", len(wx)), wx.tobytes(), wy.tobytes(),
           bytes(pb.ego[0]), pb.target[:1].tobytes(), bytes(pb.overrides[0]), pb.max_stop[:1].tobytes(),
           struct.pack("<i", pb.static_xy.shape[0]), pb.static_xy.astype(np.float64).tobytes(),
           pb.dyn_dims[0].astype(np.int32).tobytes(), pb.dyn_xy.astype(np.float64).tobytes()]
    return b"".join(out)


def straight_lean_goldens():
    """(name, kwargs, waypoints, request) of the goldens whose waypoints have one coordinate constant, on planners the
    lean form takes: at most 64 samples, no footprint circles, no chance budget"""
    out = []
    for n in golden_names():
        g = Golden(n)
        if "planner" not in g.meta or "wx" not in g.z or g.meta.get("footprint"):
            continue
        wx, wy = np.asarray(g["wx"], np.float64), np.asarray(g["wy"], np.float64)
        if not (np.all(wy == wy[0]) or np.all(wx == wx[0])):
            continue
        kw = g.planner_kwargs()
        p = make_params(**kw)
        if int(round(p.max_t / p.dt)) + 1 > 64 or kw.get("chance_epsilon", 0.0) != 0.0:
            continue
        out.append(("golden/" + n, kw, (wx, wy), request_from_golden(g)))
    return out


def all_cases():
    out = straight_lean_goldens()
    flat = [p.name for p in ff.paths() if p.flat]
    out += [(c.name, c.kw, c.path.waypoints, c.req) for c in ff.cases(path_names=flat)]
    # (the paths that are not flat: nothing is compared on them, the program only has to say so)
    out += [(c.name, c.kw, c.path.waypoints, c.req) for c in ff.cases(path_names=("rotated", "curved"), egos=("beside",), kinds=("none",))]
    for p in ff.paths():
        if p.name in ("x_even", "y_offset"):
            kw, named = ff.nonfinite_requests(p)
            out += [(f"{p.name}/nonfinite {label}", kw, p.waypoints, r) for label, r in named]
    return out


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    cases = all_cases()
    path = tmp_path_factory.mktemp("flatframe") / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"FLATCASE" + struct.pack("<i", len(cases)))
        for c in cases:
            f.write(pack_case(*c))
    return str(path), cases


def parse(stdout):
    rows = {}
    for line in stdout.splitlines():
        m = re.match(r"case (.*?) flat=(\d) rc=(-?\d+) status=(-?\d+) walked=(\d+) compared=(\d+) differences=(\d+) "
                     r"nonfinite=(\d+) seen_nan=(\d+) low_speed=(\d+) held=(\d+)", line)
        if m:
            rows[m.group(1)] = dict(zip(("flat", "rc", "status", "walked", "compared", "differences", "nonfinite", "seen_nan",
                                         "low_speed", "held"), map(int, m.groups()[1:])), line=line)
    return rows


@pytest.mark.parametrize("tag", [t for t in BUILDS if "sanitized" not in t])
def test_flat_walk_equals_the_lean_walk(tag, case_file):
    path, cases = case_file
    r = subprocess.run([build(tag), path], capture_output=True, text=True, timeout=600)
    rows = parse(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert len(rows) == len(cases)
    flat_of = {p.name: p.flat for p in ff.paths()}
    for name, kw, _, _ in cases:
        row = rows[name[:63]]
        # (-114: the emulation's own cross-check of k_cull's two box forms compares NaNs by their bits; it refuses a
        #  Frenet ego with a non-finite acceleration before any candidate is walked)
        assert row["differences"] == 0 and (row["rc"] == 0 or ("nonfinite" in name and row["rc"] == -114)), row["line"]
        want_flat = True if name.startswith("golden/") else flat_of[name.split("/")[0]]
        assert bool(row["flat"]) == want_flat, row["line"]
        if want_flat and row["walked"]:
            assert row["compared"] == row["walked"], row["line"]
    # the cases reach what they are about
    n_gold = sum(1 for n in rows if n.startswith("golden/"))
    assert n_gold >= 10, f"only {n_gold} straight lean goldens"
    assert rows["x_even/creep/none"]["low_speed"] > 0, rows["x_even/creep/none"]["line"]
    assert rows["x_even/ladder/none"]["held"] > 0 and rows["x_even/standing/none"]["held"] == 0
    assert rows["x_even/road_edge/none"]["compared"] > 0
    assert rows["x_even/beside/config3"]["status"] in (_abi.PLAN_OK, _abi.PLAN_NO_PATH)
    poisoned = [n for n, row in rows.items() if "nonfinite" in n and (row["nonfinite"] or row["seen_nan"])]
    assert len(poisoned) >= 10, f"only {len(poisoned)} non-finite egos reach the walk with a poisoned sample"


@pytest.mark.parametrize("tag", [t for t in BUILDS if "sanitized" not in t])
def test_samples_with_non_finite_lateral_states(tag):
    r = subprocess.run([build(tag), "--nonfinite"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"samples (\d+) poisoned=(\d+) differences=(\d+)", r.stdout)
    assert m and int(m.group(1)) > 100000 and int(m.group(2)) > 1000 and int(m.group(3)) == 0, r.stdout


def test_the_path_flag_on_hand_made_coefficients():
    r = subprocess.run([build("unfused"), "--flags"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"flag (.*) got=(\d) want=(\d)", r.stdout)
    assert len(rows) >= 20 and all(g == w for _, g, w in rows), r.stdout
    assert any(w == "1" for _, _, w in rows) and any("last segment" in n and w == "0" for n, _, w in rows)


def test_sanitized_build_runs_clean(case_file):
    """address + undefined-behaviour sanitizers, the program run as a plain executable: all three modes"""
    path, _ = case_file
    tag = next(t for t in BUILDS if "sanitized" in t)
    exe = build(tag)
    for args in ([path], ["--nonfinite"], ["--flags"]):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
            f"{args}: exit {r.returncode}\n" + r.stdout[-1500:] + r.stderr[-3000:]
