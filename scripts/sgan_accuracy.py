#!/usr/bin/env python3
"""The accuracy of fot_sgan_sample on a fixture (tests/golden/sgan/cases.npz, or edges.npz with --table edges): per case e_ref = max |reference float32 -
reference float64|, the bound max(8 e_ref, 16 ulp32 of the largest |coordinate|), and the library's largest error
against the reference's float64 output as a ratio of the bound -- on the GPU, and for csrc/fot_sgan.hpp built for the CPU
(tests/emu/fot_sgan_emu.cpp) where that program has been built.

    python3 scripts/sgan_accuracy.py --out profiles/r10_sgan_accuracy.json
    python3 scripts/sgan_accuracy.py --table edges --out profiles/r11_sgan_edges_accuracy.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", choices=("cases", "edges"), default="cases")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sgan_common as sc
    from integrated_path_planning_amd import _abi, synthetic as syn
    from integrated_path_planning_amd.planner import BatchPlanner
    from integrated_path_planning_amd.prediction import SganWeights

    lib = _abi.lib()
    table, path = (sc.CASES, sc.FIXTURE) if args.table == "cases" else (sc.EDGE_CASES, sc.EDGE_FIXTURE)
    fix = sc.load_fixture(path)
    emu = os.path.join(ROOT, "tests", "emu", "_build", "fot_sgan_emu")
    cases = {}
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp, \
            tempfile.TemporaryDirectory() as tmp:
        for name in table:
            a = sc.case_args(name)
            w = SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)))
            obs, off, noise, r32, r64 = sc.fixture_case(fix, name)
            S = noise.shape[0]
            _abi.check(bp._h, lib.fot_sgan_load(bp._h, C.byref(w.desc), w.blob.size, w.blob.ctypes.data))
            out = np.zeros(r64.shape, np.float32)
            _abi.check(bp._h, lib.fot_sgan_sample(bp._h, len(off) - 1, off.ctypes.data, obs.ctypes.data, S,
                                                  noise.ctypes.data if noise.size else None, 0, out.ctypes.data, None))
            bound = sc.accuracy_bound(r32, r64)
            rec = dict(e_ref=float(np.max(np.abs(r32 - r64))), bound=bound,
                       gpu_error=float(np.max(np.abs(out - r64))), gpu_ratio=float(np.max(np.abs(out - r64))) / bound)
            if os.path.exists(emu):
                inp, outp = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
                sc.write_emu_case(inp, bytes(w.desc), w.blob, off, obs, S, noise)
                subprocess.run([emu, inp, outp], check=True)
                e = np.fromfile(outp, dtype=np.float32).reshape(r64.shape)
                rec.update(emu_error=float(np.max(np.abs(e - r64))), emu_ratio=float(np.max(np.abs(e - r64))) / bound)
            cases[name] = rec
            print(name, json.dumps(rec), flush=True)
    doc = dict(fixture=os.path.relpath(path, ROOT), bound="max(8 e_ref, 16 ulp32(max |coordinate|)) against the reference's float64 output",
               worst_gpu_ratio=max(c["gpu_ratio"] for c in cases.values()),
               worst_emu_ratio=max((c["emu_ratio"] for c in cases.values() if "emu_ratio" in c), default=None), cases=cases)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
