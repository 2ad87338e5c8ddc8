"""The plan unit stays apart from prediction and the closed loop: csrc/fot_kernels.hip includes none of their headers, and
the headers it does include are exactly the prerequisites the Makefile gives fot_kernels.o -- work on prediction or the
loop rebuilds neither the evaluation kernels nor bench.py's kernel_source_hash.  The same holds for every object of
libfot.so: each of the three device units and the three host units lists exactly the headers it reads, the handle and
plan unit of the host side reads no launcher header but the plan path's, and what the host units share through
fot_host.hpp is exported nowhere.  Preprocessing and symbol tables only: include dependencies, never instructions."""
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
# every object of libfot.so and its source; the pass that counts: the device pass of a .hip unit, the host pass of a host unit
UNITS = {"_obj/fot_kernels.o": "fot_kernels.hip", "_obj/fot_loop_kernels.o": "fot_loop_kernels.hip",
         "_obj/fot_sgan.o": "fot_sgan.hip", "_obj/fot_host.o": "fot_host.cpp", "_obj/fot_host_pred.o": "fot_host_pred.cpp",
         "_obj/fot_host_loop.o": "fot_host_loop.cpp"}
# headers of prediction, the closed loop and the Social-GAN generator
FOREIGN = ("fot_summary.hpp", "fot_predscore.hpp", "fot_loopscore.hpp", "fot_repsample.hpp", "fot_replay.hpp",
           "fot_samplerec.hpp", "fot_sgan.h", "fot_sgan.hpp", "fot_noise.hpp", "fot_loop_kernels.h")
INTERNAL = "fot::host::"                # the namespace of what fot_host.hpp declares for the other host units


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


def headers(files):
    return {f for f in files if f.endswith((".h", ".hpp", ".inc"))}


@pytest.fixture(scope="module")
def compile_flags():
    """per object, the flags of the Makefile's own compile line (dry run), without what makes it write an object"""
    lines = make("-n", "-B").splitlines()
    out = {}
    for obj, src in UNITS.items():
        line = next(l for l in lines if " -c %s " % src in l)
        flags, skip = [], False
        for w in shlex.split(line)[1:]:
            if skip:
                skip = False
            elif w == "-o":
                skip = True
            elif w not in ("-c", src) and not w.startswith("-save-temps"):
                flags.append(w)
        assert "--offload-arch=gfx950" in flags and "-O3" in flags, line
        out[obj] = flags
    return out


@pytest.fixture(scope="module")
def includes_of(compile_flags):
    """object -> what the compiler reads for it, by its own account"""
    cache = {}

    def get(obj):
        if obj in cache:
            return cache[obj]
        src = UNITS[obj]
        side = "--cuda-device-only" if src.endswith(".hip") else "--cuda-host-only"

        def run(*mode):
            r = subprocess.run([HIPCC, *compile_flags[obj], side, *mode, src], cwd=CSRC, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
            return r.stdout
        rule = run("-MM")
        files = rule.split(":", 1)[1].replace("\\\n", " ").split() if ":" in rule else []
        if not files:       # (a compiler that writes dependency rules from the host pass only: the device pass's line markers)
            files = sorted(set(re.findall(r'^# \d+ "([^"<][^"]*)"', run("-E"), flags=re.M)))
        files = project_files(files)
        assert "integrated_path_planning_amd/csrc/" + src in files, files
        cache[obj] = files
        return files
    return get


@pytest.fixture(scope="module")
def prerequisites():
    """object -> the project files the Makefile makes it depend on"""
    rules = make("-pn").splitlines()
    return lambda obj: project_files(next(l for l in rules if l.startswith(obj + ":")).split(":", 1)[1].split())


@pytest.fixture(scope="module")
def included(includes_of):
    """what the device pass of fot_kernels.hip reads"""
    return includes_of(OBJECT)


def test_plan_unit_includes_no_prediction_or_loop_header(included):
    names = {os.path.basename(f) for f in included}
    assert not names & set(FOREIGN), sorted(names & set(FOREIGN))


def test_plan_unit_includes_exactly_the_makefile_prerequisites(included):
    rule = next(l for l in make("-pn", OBJECT).splitlines() if l.startswith(OBJECT + ":"))
    prereq = project_files(rule.split(":", 1)[1].split())
    headers = lambda files: {f for f in files if f.endswith((".h", ".hpp", ".inc"))}
    assert headers(prereq) and headers(included) == headers(prereq), (sorted(headers(included)), sorted(headers(prereq)))


@pytest.mark.parametrize("obj", sorted(UNITS))
def test_every_unit_includes_exactly_the_makefile_prerequisites(obj, includes_of, prerequisites):
    read, listed = headers(includes_of(obj)), headers(prerequisites(obj))
    assert listed and read == listed, (sorted(read - listed), sorted(listed - read))


def test_host_units_include_the_launcher_headers_they_launch_from(includes_of):
    names = lambda obj: {os.path.basename(f) for f in includes_of(obj)}
    # the handle and plan unit launches the plan path only
    assert "fot_kernels.h" in names("_obj/fot_host.o")
    assert not names("_obj/fot_host.o") & {"fot_loop_kernels.h", "fot_sgan.h"}
    # the prediction unit calls no plan launcher: launch_resample, launch_sample_dist, launch_safety, launch_pred_scores
    # (fot_loop_kernels.h) and the generator's launch_sgan_* (fot_sgan.h)
    assert "fot_kernels.h" not in names("_obj/fot_host_pred.o")
    assert {"fot_loop_kernels.h", "fot_sgan.h"} <= names("_obj/fot_host_pred.o")
    # the loop unit calls one: launch_frenet_state, for the nearest point of the new ego states (fot_loop_observe_begin);
    # its requests reach the other plan launchers through the plan unit's enqueue_plan
    assert {"fot_kernels.h", "fot_loop_kernels.h", "fot_sgan.h"} <= names("_obj/fot_host_loop.o")
    for obj in ("_obj/fot_host.o", "_obj/fot_host_pred.o", "_obj/fot_host_loop.o"):
        assert "fot_host.hpp" in names(obj)


def test_internal_namespace_is_not_exported():
    lib = os.path.join(CSRC, "..", "libfot.so")
    assert os.path.exists(lib), "libfot.so is not built (the suite's session start builds it)"
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    assert nm and filt, "nm / c++filt (or ROCm's llvm-nm / llvm-cxxfilt) are needed"

    def symbols(*mode):
        raw = subprocess.run([nm, *mode, "--defined-only", lib], capture_output=True, text=True, timeout=60, check=True).stdout
        return subprocess.run([filt], input=raw, capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    exported = symbols("-D")
    assert any(l.endswith(" fot_create") for l in exported), exported[:5]
    # the namespace looked for is the one in use: the library's own symbol table names the shared helpers in it
    assert any(INTERNAL + "enqueue_plan(" in l for l in symbols()), "no %senqueue_plan in libfot.so" % INTERNAL
    assert not [l for l in exported if INTERNAL in l], [l for l in exported if INTERNAL in l]
