#!/usr/bin/env python3
"""Static picture of k_cull's instruction stream: vector instructions by mnemonic class, per phase.

usage: cull_isa_phases.py <fot_kernels-hip-amdgcn-amd-amdhsa-gfx950.s> [float|double]

The phases of cull_group are separated by workgroup barriers, so the text between two `s_barrier`s of the kernel's ISA
is one phase (in layout order, which follows the source for this kernel; cold blocks the compiler moved to the end
land in the last phase).  Counts are static -- instructions in the text, not instructions executed -- and are meant
to be read beside the per-phase counters of profiles/r26_cull_stream.txt.
"""
import collections
import re
import sys

CLASSES = (
    ("lane", re.compile(r"v_(readlane|writelane|readfirstlane)_")),
    ("mov", re.compile(r"v_(mov|accvgpr)")),
    ("select", re.compile(r"v_cndmask")),
    ("cmp", re.compile(r"v_cmpx?_")),
    ("dpp/perm", re.compile(r"v_(permlane|perm_|bfe|bfi|mbcnt|swap)")),
    ("cvt", re.compile(r"v_cvt_")),
    ("f64", re.compile(r"v_\w+_f64")),
    ("trans", re.compile(r"v_(rcp|rsq|sqrt|sin|cos|exp|log)_")),
    ("f32", re.compile(r"v_(pk_)?\w+_f32")),
    ("int64", re.compile(r"v_(lshl_add_u64|mad_[iu]64|lshlrev_b64|lshrrev_b64|ashrrev_i64|add_co|addc_co|sub_co|subb_co)")),
    ("mul32", re.compile(r"v_mul_(lo|hi)_")),
    ("int32", re.compile(r"v_")),
)


def kernel_text(path, dtype):
    tag = "k_cullI%sEE" % ("f" if dtype == "float" else "d")
    lines, on = [], False
    for line in open(path):
        if not on:
            on = line.startswith("_ZN3fot6" + tag) and line.rstrip().split(";")[0].rstrip().endswith(":")
            continue
        if line.startswith(".Lfunc_end"):
            break
        lines.append(line)
    return lines


def main():
    path = sys.argv[1]
    dtype = sys.argv[2] if len(sys.argv) > 2 else "float"
    phases = [collections.Counter()]
    other = collections.Counter()
    for line in kernel_text(path, dtype):
        ins = line.split(";")[0].strip()
        if not ins or ins.endswith(":") or ins.startswith("."):
            continue
        op = ins.split()[0]
        if op == "s_barrier":
            phases.append(collections.Counter())
            continue
        if op.startswith("v_"):
            for name, rx in CLASSES:
                if rx.match(op):
                    phases[-1][name] += 1
                    break
        else:
            kind = "salu" if op.startswith("s_") else ("lds" if op.startswith("ds_") else
                                                       ("flat" if op.startswith("flat_") else
                                                        ("global" if op.startswith("global_") else "other")))
            phases[-1]["(" + kind + ")"] += 1
            other[op.split("_")[0]] += 1
    cols = [c for c, _ in CLASSES] + ["(salu)", "(lds)", "(global)", "(flat)"]
    print("k_cull<%s>: static instructions per phase (between workgroup barriers)" % dtype)
    print("%-6s %6s | " % ("phase", "valu") + " ".join("%8s" % c for c in cols))
    tot = collections.Counter()
    for i, ph in enumerate(phases):
        valu = sum(v for k, v in ph.items() if not k.startswith("("))
        print("%-6d %6d | " % (i, valu) + " ".join("%8d" % ph[c] for c in cols))
        tot.update(ph)
    valu = sum(v for k, v in tot.items() if not k.startswith("("))
    print("%-6s %6d | " % ("all", valu) + " ".join("%8d" % tot[c] for c in cols))


if __name__ == "__main__":
    main()
