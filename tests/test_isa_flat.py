"""The flat forms of the lean evaluation kernels in the device ISA of the current sources: the build-time guard lists them
on lines of their own shape, they keep within the lean forms' register / spill / scratch limits with no instruction
touching a hand-issued load's destination in flight, and scripts/isa_loop.py shows the flat time step with fewer float64
and fewer vector instructions than the lean one."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
GUARD = os.path.join(ROOT, "scripts", "isa_check_async.py")
LOOP = os.path.join(ROOT, "scripts", "isa_loop.py")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
LEAN = ("k_evaluate_split_lean", "k_evaluate_group_lean")       # the lean kernels that have a flat form
ROW = r"\(vgpr (\d+), sgpr spills (\d+), vgpr spills (\d+), scratch (\d+) B\)"

pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc not available")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """the gfx950 ISA of csrc/fot_kernels.hip under the Makefile's flags (device side only)"""
    s = tmp_path_factory.mktemp("isa") / "fot.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-ffp-contract=on", "--offload-arch=gfx950", "-Wno-unused-function", "-S",
                    "--cuda-device-only", "-o", str(s), os.path.join(CSRC, "fot_kernels.hip")],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return str(s)


def test_guard_lists_the_flat_kernels_on_their_own_lines(isa):
    r = subprocess.run([sys.executable, GUARD, isa, "--min-kernels", "6", "--min-flat", "2"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    flat, lean = {}, {}
    for line in r.stdout.splitlines():
        m = re.match(r"flat form of (k_evaluate\w*): (k_evaluate\w*): (\d+) instructions touching a destination in flight of "
                     r"(\d+) hand-issued scalar loads " + ROW, line)
        if m:
            assert m.group(2) == m.group(1) + "_flat", line
            flat[m.group(1)] = dict(zip(("findings", "loads", "vgpr", "sspill", "vspill", "scratch"), map(int, m.groups()[2:])))
        m = re.match(r"(k_evaluate\w*) \(lean form\): .*" + ROW, line)
        if m:
            lean[m.group(1)] = dict(zip(("vgpr", "sspill", "vspill", "scratch"), map(int, m.groups()[1:])))
        assert not re.match(r"k_evaluate\w*_flat\b", line), f"a flat kernel on a line of the other kernels' shape: {line}"
    assert sorted(flat) == sorted(LEAN) and set(LEAN) <= set(lean), r.stdout
    for name in LEAN:
        f, l = flat[name], lean[name]
        assert f["findings"] == 0 and f["loads"] > 0 and f["vspill"] == 0 and f["scratch"] == 0, (name, f)
        assert f["vgpr"] <= l["vgpr"] and f["sspill"] <= l["sspill"], (name, f, l)


def test_guard_fails_without_the_flat_kernels(isa, tmp_path):
    """--min-flat counts them: the ISA with the flat kernels' bodies renamed away does not pass"""
    t = open(isa).read()
    cut = tmp_path / "noflat.s"
    cut.write_text(re.sub(r"(k_evaluate\w*?)_lean_flatE", lambda m: m.group(1).replace("k_evaluate", "k_other") + "_lean_flatE", t))
    r = subprocess.run([sys.executable, GUARD, str(cut), "--min-kernels", "6", "--min-flat", "2"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "only 0 flat evaluation kernels" in r.stdout, r.stdout + r.stderr


def loop_table(isa, kernel):
    r = subprocess.run([sys.executable, LOOP, isa, kernel], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head = next(l for l in r.stdout.splitlines() if l.startswith("block"))
    step = next(l for l in r.stdout.splitlines() if l.startswith("per step"))
    walk = next(l for l in r.stdout.splitlines() if l.startswith("min-walk") and "per pair" in l)
    keys = head.split()[2:]
    return dict(zip(keys, map(int, step.split()[3:]))), dict(zip(keys, map(int, walk.split()[3:]))), r.stdout


def test_loop_tables_of_every_evaluation_kernel(isa):
    """isa_loop.py --all: the six kernels of the two forms and the two flat kernels, a table each"""
    r = subprocess.run([sys.executable, LOOP, isa, "--all"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    names = re.findall(r"^(k_evaluate\w*): time-step loop", r.stdout, re.M)
    assert sorted(names) == sorted(["k_evaluate", "k_evaluate_split", "k_evaluate_group", "k_evaluate_lean", "k_evaluate_split_lean",
                                    "k_evaluate_group_lean", "k_evaluate_split_lean_flat", "k_evaluate_group_lean_flat"]), r.stdout
    assert len(re.findall(r"^per step", r.stdout, re.M)) == 8


@pytest.mark.parametrize("base", LEAN)
def test_the_flat_step_is_shorter(isa, base):
    lean, lean_walk, out_l = loop_table(isa, base)
    flat, flat_walk, out_f = loop_table(isa, base + "_flat")
    assert lean["VALU"] > 100 and lean["f64"] > 50, out_l                              # a table, not zeros
    # at least the ten float64 operations of the curvature terms and the CK_SINGULAR test's compares; the same min-only walk,
    # one LDS read less (the row's kappa_r and kappa_r'), and no more scalar work
    assert flat["f64"] <= lean["f64"] - 10 and flat["VALU"] <= lean["VALU"] - 13, (lean, flat)
    assert flat["cmp"] < lean["cmp"] and flat["LDS"] < lean["LDS"], (lean, flat)
    assert flat_walk == lean_walk and flat["SALU"] <= lean["SALU"], (lean, flat)
    assert "circles" not in out_f.splitlines()[0]
