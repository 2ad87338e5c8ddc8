"""The build-time ceiling on k_frenet_state's vector registers (scripts/isa_check_async.py --max-vgpr, csrc/Makefile).

Four evaluation waves of 112 registers leave 64 of a SIMD's 512: a wave of k_frenet_state starts beside THREE of them up
to 176 registers and has to wait for a second one to leave above that -- with four plan calls in flight that wait was
4 - 5 us of the step (profiles/r25_frenet_waves_ab.txt).  The guard is given kernel metadata as the compiler writes it.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = os.path.join(ROOT, "scripts", "isa_check_async.py")
NAME = "_ZN3fot14k_frenet_stateEPKNS_9DevParamsE"


def metadata(name, vgpr, spills=0, scratch=0):
    return (f"amdhsa.kernels:\n  - .args: []\n    .name:           {name}\n    .private_segment_fixed_size: {scratch}\n"
            f"    .sgpr_count:     106\n    .sgpr_spill_count: 40\n    .vgpr_count:     {vgpr}\n    .vgpr_spill_count: {spills}\n"
            f"    .wavefront_size: 64\n")


def run_guard(tmp_path, text, *args):
    p = tmp_path / "k.s"
    p.write_text(text)
    r = subprocess.run([sys.executable, GUARD, str(p), "--min-kernels", "0", *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout + r.stderr


def test_ceiling_holds_and_catches(tmp_path):
    opt = ("--max-vgpr", "k_frenet_state=176")
    rc, out = run_guard(tmp_path, metadata(NAME, 176), *opt)
    assert rc == 0 and "vgpr 176 of at most 176" in out, out
    rc, out = run_guard(tmp_path, metadata(NAME, 177), *opt)
    assert rc == 1 and "over its register ceiling" in out, out
    rc, out = run_guard(tmp_path, metadata(NAME, 168, spills=25, scratch=104), *opt)      # fits, but by spilling
    assert rc == 1, out
    rc, out = run_guard(tmp_path, metadata("_ZN3fot6k_cullIfEEvPKNS_9DevParamsE", 55), *opt)
    assert rc == 1 and "k_frenet_state: not in" in out, out
    rc, out = run_guard(tmp_path, metadata(NAME, 207))                                    # not asked for: not checked
    assert rc == 0, out


def test_makefile_asks_for_the_ceiling():
    mk = open(os.path.join(ROOT, "integrated_path_planning_amd", "csrc", "Makefile")).read()
    assert "--max-vgpr k_frenet_state=176" in mk
