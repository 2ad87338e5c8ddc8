#!/usr/bin/env python3
"""Golden vectors of the REFERENCE planner against prediction distributions of more than 64 samples (build container only).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_samples.py [--ref /root/reference]

The reference's plan() takes a distribution of any sample count; the library plans more than 64 samples only on a
handle whose sample capacity was raised (BatchPlanner(sample_capacity=...), up to 254).  Three cases of
synthetic.config3_instance on the straight path, run by make_golden.run_case and written -- in its format -- to
tests/golden/wide_samples/ (NOT tests/golden/: conftest.golden_names() feeds every top-level case to the golden tests
of a default handle; conftest.Golden("wide_samples/NAME") loads these):

  dist_s100_eps0          S = 100, P = 5, eps = 0                  (a lean-eligible wide launch)
  dist_s100_eps005        S = 100, P = 5, eps = 0.05: max_viol 5   (the four-word sample mask)
  footprint3_s130_eps01   S = 130, P = 4, eps = 0.1: max_viol 13, the 3-circle footprint of the case footprint3

For each case the first seed is taken at which the reference keeps 'ok' and 'collision_error' candidates and, where
eps > 0, at least one candidate's verdict differs from the eps = 0 verdict on the same tensor (the budget decides
something); both are asserted.  No file may be larger than the largest fixture there was, dist_s64.npz.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import import_reference, run_case  # noqa: E402

syn = mg.syn
OUT = os.path.join(HERE, "wide_samples")
MAX_BYTES = 330293                                    # dist_s64.npz
ST_COLLISION, ST_OK = 5, 6
FOOTPRINT3 = dict(length=4.5, width=1.8, n=3)
#        name                     S    P  eps   footprint
CASES = [("dist_s100_eps0", 100, 5, 0.0, None),
         ("dist_s100_eps005", 100, 5, 0.05, None),
         ("footprint3_s130_eps01", 130, 4, 0.1, FOOTPRINT3)]


def case_of(name, seed, S, P, eps, footprint):
    inst = syn.config3_instance(seed, S=S, P=P)
    return dict(name=name, path="straight", planner=dict(syn.CONFIG3_PLANNER, chance_epsilon=eps),
                ego=[float(v) for v in inst.ego], target_speed=syn.TARGET_SPEED, overrides=None, max_stop=None, prev_s=None,
                last_kappa=0.0, footprint=footprint, static=np.empty((0, 2)), dyn=None, dist=inst.dist.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--seeds", type=int, default=64, help="seeds tried per case")
    args = ap.parse_args()
    ref = import_reference(args.ref)
    os.makedirs(OUT, exist_ok=True)
    for name, S, P, eps, footprint in CASES:
        assert int(np.floor(eps * S)) == {0.0: 0, 0.05: 5, 0.1: 13}[eps]
        for seed in range(args.seeds):
            with tempfile.TemporaryDirectory() as tmp:
                out = run_case(ref, case_of(name, seed, S, P, eps, footprint), tmp)
                st = out["cand_status"]
                good = (st == ST_OK).any() and (st == ST_COLLISION).any()
                if good and eps > 0.0:
                    hard = run_case(ref, case_of(name, seed, S, P, 0.0, footprint), tmp)["cand_status"]
                    good = bool((hard != st).any())
                    # the budget only ever forgives: a verdict that differs is a collision at eps = 0
                    assert ((hard == st) | ((hard == ST_COLLISION) & (st != ST_COLLISION))).all(), name
            if good:
                break
        else:
            raise AssertionError(f"{name}: no seed below {args.seeds} meets the conditions")
        out = run_case(ref, case_of(name, seed, S, P, eps, footprint), OUT)
        st = out["cand_status"]
        assert (st == ST_OK).any() and (st == ST_COLLISION).any(), name
        assert out["dist"].shape[:2] == (S, P), name
        size = os.path.getsize(os.path.join(OUT, name + ".npz"))
        assert size <= MAX_BYTES, f"{name}: {size} bytes"
        print(f"{name}: seed {seed}, {size} bytes")


if __name__ == "__main__":
    main()
