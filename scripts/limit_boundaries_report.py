"""Puts the per-scene reports of tests/test_gpu_limit_boundaries.py together into one profile.

    FOT_LIMIT_REPORT_DIR=<dir> python -m pytest tests/test_gpu_limit_boundaries.py -m gpu -s
    python scripts/limit_boundaries_report.py <dir> profiles/<name>.json
"""
import glob
import json
import os
import sys


def main(src, dst):
    out = {"made_by": "FOT_LIMIT_REPORT_DIR=<dir> pytest tests/test_gpu_limit_boundaries.py -m gpu -s; "
                      "scripts/limit_boundaries_report.py <dir> <this file>",
           "dev": "relative difference of the library's debug-path value of a rule's quantity from the oracle's, worst over "
                  "the samples the rule reads; a delta is used on a target at |delta| >= 10 dev",
           "scenes": {}}
    for f in sorted(glob.glob(os.path.join(src, "limit_boundaries_*.json"))):
        with open(f) as fh:
            r = json.load(fh)
        out["scenes"][r.pop("scene")] = r
    worst, keep = {}, {}
    for r in out["scenes"].values():
        for k, v in r["worst_dev"].items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k, v in r["retained_share"].items():
            keep.setdefault(k, []).append((v, r["targets"]))
    out["instances"] = sum(r["instances"] for r in out["scenes"].values())
    out["evaluations"] = sum(r["evaluations"] for r in out["scenes"].values())
    out["worst_dev_per_rule"] = worst
    out["retained_share_all_targets"] = {k: sum(v * n for v, n in lst) / sum(n for _, n in lst) for k, lst in keep.items()}
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: out[k] for k in ("instances", "evaluations", "worst_dev_per_rule", "retained_share_all_targets")},
                     indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
