#!/usr/bin/env python3
"""Golden vectors for the external-path checks behind fot_check_paths / fot_check_collision_paths (build container only).

Runs the REFERENCE methods FrenetPlanner._check_paths, _apply_stop_distance_filter, _check_collision and
_check_collision_distribution (src/planning/frenet_planner.py:307-324, 891-1233) read-only on the hand-made classes and
on the first seeded fuzz calls of tests/check_paths_common.py (which only builds the inputs here).  Writes
tests/golden/check_paths/cases.npz -- inputs and expected outputs only: per path the category of _check_paths (+ the stop
filter when the call has a max_stop_distance; 'dropped' = in no list) and the answer of the collision entry the call's
obstacle set selects.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import check_paths_common as pc  # noqa: E402

N_FUZZ = 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    lg = types.ModuleType("loguru")

    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None

    lg.logger = _Logger()
    sys.modules["loguru"] = lg
    sys.path.insert(0, args.ref)
    from src.core.data_structures import FrenetPath
    from src.core.footprint import EgoFootprint
    from src.planning.cubic_spline import CubicSpline2D
    from src.planning.frenet_planner import FrenetPlanner

    csp = CubicSpline2D([0.0, 50.0, 100.0], [0.0, 0.0, 0.0])
    calls = pc.class_calls() + [pc.fuzz_call(s) for s in range(N_FUZZ)]
    expected = []
    for cl in calls:
        c = dict(cl["cfg"])
        fp = c.pop("footprint")
        if fp is not None:
            c["footprint"] = EgoFootprint(offsets=np.asarray(fp[0], float), radius=float(fp[1]))
        pl = FrenetPlanner(csp, **c)
        paths = [FrenetPath(**{f: list(p[f]) for f in pc.FIELDS}) for p in cl["paths"]]
        static = np.empty((0, 2)) if cl["static"] is None else cl["static"]
        res = pl._check_paths(paths, static, cl["dyn"], cl["overrides"], cl["dist"])
        if cl["max_stop"] is not None:
            pl._apply_stop_distance_filter(res, cl["max_stop"])
        cat = np.full(len(paths), pc.DROPPED)
        for name, members in res.items():
            for m in members:
                cat[[m is q for q in paths].index(True)] = pc.CATEGORIES.index(name)
        if cl["dist"] is not None and cl["dist"].size > 0:
            free = [pl._check_collision_distribution(q, static, cl["dist"], pl.chance_epsilon) for q in paths]
        else:
            free = [pl._check_collision(q, static, cl["dyn"]) for q in paths]
        expected.append(dict(cat=cat, free=np.array(free, bool)))
    os.makedirs(os.path.join(HERE, "check_paths"), exist_ok=True)
    out = os.path.join(HERE, "check_paths", "cases.npz")
    pc.save_calls(out, calls, expected)
    print(f"wrote {len(calls)} calls, {sum(len(c['paths']) for c in calls)} paths, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
