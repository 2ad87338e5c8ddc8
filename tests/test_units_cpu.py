"""The plan unit stays apart from prediction and the closed loop: csrc/fot_kernels.hip includes none of their headers, and
the headers it does include are exactly the prerequisites the Makefile gives fot_kernels.o -- work on prediction or the
loop rebuilds neither the evaluation kernels nor bench.py's kernel_source_hash.  Preprocessing only: include
dependencies, never instructions."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
OBJECT = "_obj/fot_kernels.o"
# headers of prediction, the closed loop and the Social-GAN generator
FOREIGN = ("fot_summary.hpp", "fot_predscore.hpp", "fot_loopscore.hpp", "fot_repsample.hpp", "fot_replay.hpp",
           "fot_samplerec.hpp", "fot_sgan.h", "fot_sgan.hpp", "fot_noise.hpp", "fot_loop_kernels.h")


def make(*args):
    # no skip where hipcc or make is missing: the library cannot be built without them either, and a guard that switches
    # itself off guards nothing
    assert HIPCC and shutil.which("make"), "hipcc and make are needed (as for building libfot.so)"
    r = subprocess.run(["make", "-C", CSRC, "--no-print-directory", "HIPCC=" + HIPCC, *args], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def project_files(paths):
    """of `paths` (relative to csrc), the ones inside the repository, relative to its root"""
    out = set()
    for p in paths:
        full = os.path.realpath(os.path.join(CSRC, p))
        if full.startswith(ROOT + os.sep):
            out.add(os.path.relpath(full, ROOT))
    return out


@pytest.fixture(scope="module")
def compile_flags():
    """the flags of the Makefile's own compile line of fot_kernels.o (dry run), without what makes it write an object"""
    line = next(l for l in make("-n", "-B", OBJECT).splitlines() if " -c fot_kernels.hip" in l)
    words = shlex.split(line)[1:]
    flags, skip = [], False
    for w in words:
        if skip:
            skip = False
        elif w == "-o":
            skip = True
        elif w not in ("-c", "fot_kernels.hip") and not w.startswith("-save-temps"):
            flags.append(w)
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, line
    return flags


@pytest.fixture(scope="module")
def included(compile_flags):
    """what the device pass of fot_kernels.hip reads, by the compiler's own account"""
    def run(*mode):
        r = subprocess.run([HIPCC, *compile_flags, "--cuda-device-only", *mode, "fot_kernels.hip"], cwd=CSRC,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout
    rule = run("-MM")
    files = rule.split(":", 1)[1].replace("\\\n", " ").split() if ":" in rule else []
    if not files:       # (a compiler that writes dependency rules from the host pass only: the device pass's line markers)
        files = sorted(set(re.findall(r'^# \d+ "([^"<][^"]*)"', run("-E"), flags=re.M)))
    files = project_files(files)
    assert "integrated_path_planning_amd/csrc/fot_kernels.hip" in files, files
    return files


def test_plan_unit_includes_no_prediction_or_loop_header(included):
    names = {os.path.basename(f) for f in included}
    assert not names & set(FOREIGN), sorted(names & set(FOREIGN))


def test_plan_unit_includes_exactly_the_makefile_prerequisites(included):
    rule = next(l for l in make("-pn", OBJECT).splitlines() if l.startswith(OBJECT + ":"))
    prereq = project_files(rule.split(":", 1)[1].split())
    headers = lambda files: {f for f in files if f.endswith((".h", ".hpp", ".inc"))}
    assert headers(prereq) and headers(included) == headers(prereq), (sorted(headers(included)), sorted(headers(prereq)))
