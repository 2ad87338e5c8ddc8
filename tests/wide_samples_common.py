"""Instances of the wide-sample tests (test_wide_samples_cpu.py, test_gpu_wide_samples.py): the chance budget of plan()
against prediction distributions of 65 .. 254 samples, on a handle whose sample capacity was raised.

Above 64 samples the count of DISTINCT hitting samples passes through code of its own: the four-word mask of the wide
general kernels (sample s is bit s & 63 of word s >> 6), the four mask words a segment of k_evaluate_split_wide hands to
wave 0, the lean-wide re-check that must not look at sample ids at all, collide_candidate_wide of the external-path
checkers.  The instances are chance_budget_common's, built on its scenes with its placement (Scene.place: a hit is an
obstacle row 0.5 R from a (candidate, step, circle) point of the ORACLE's lattice, every other row 5 km away, the whole
lattice CLEARANCE away from the radius, so a table must EQUAL the oracle's): pattern A hits the target candidate in
exactly max_viol distinct samples (it stays feasible), B in one more (it collides), C in max_viol samples again and
again over steps, pedestrians and circles (feasible).  Hits take their sample ids in the order of sample_ids(): the last
id, then both sides of every word edge.  Nothing is taken from the code under test; importing this module loads no GPU
library.
"""
import functools

import numpy as np

import chance_budget_common as cb
from chance_budget_common import CLEARANCE, P, SCENE_NAMES, max_viol, scene  # noqa: F401

# (eps, S) -> max_viol = floor(eps S) in float64, as the reference computes it
PAIRS = {(0.0, 65): 0, (0.0, 254): 0, (0.02, 65): 1, (0.5, 65): 32, (0.99, 65): 64, (1.0, 65): 65, (0.5, 128): 64,
         (0.51, 128): 65, (0.5, 129): 64, (0.75, 192): 144, (0.253, 254): 64, (0.999, 254): 253, (1.0, 254): 254,
         (0.07, 100): 7, (0.29, 100): 28}
EDGE_IDS = (0, 63, 64, 65, 127, 128, 129, 191, 192, 193)
PATTERNS = ("A", "B", "C")


def pair_facts():
    """What the hand-picked pairs are there for."""
    for (eps, S), m in PAIRS.items():
        assert max_viol(eps, S) == m, (eps, S, max_viol(eps, S), m)
    assert 0.07 * 100 == 7.000000000000001 and 0.29 * 100 == 28.999999999999996      # either side of an integer
    assert all(64 < S <= 254 for _, S in PAIRS)


def sample_ids(S):
    """The order in which hits take their samples: S - 1, then 0, 63, 64, 65, 127, 128, 129, 191, 192, 193 (ids >= S
    dropped), then the rest ascending: the last id, both sides of every word edge, and every id exactly once."""
    first = list(dict.fromkeys(s for s in (S - 1,) + EDGE_IDS if 0 <= s < S))
    ids = first + [s for s in range(S) if s not in first]
    assert len(ids) == S and len(set(ids)) == S, (S, ids)
    return ids


def hits(sc, c, S, n_hit, spread):
    """chance_budget_common._hits with this module's sample order: the first n_hit samples of sample_ids(S) hit
    candidate c, hit j at target step j mod n_steps, pedestrian j mod P, circle j mod n_circles; spread: every hitting
    sample also hits at all other target steps, through both pedestrians and going round the circles.  Scene.place raises
    where a placement cannot keep CLEARANCE: no instance is left out."""
    steps, n_c = sc.steps(c), len(sc.offsets)
    ids = sample_ids(S)[:n_hit]
    d = sc.far_tensor(S)
    for j, s in enumerate(ids):
        d[s, j % P, steps[j % len(steps)]] = sc.place(c, steps[j % len(steps)], j % n_c)
        if spread:
            for q, k in enumerate(steps):
                for ped in range(P):
                    d[s, ped, k] = sc.place(c, k, (j + q + ped) % n_c)
    return d, ids


def pattern_instances(sc):
    """A, B and C for every (eps, S) pair and target candidate.  B needs max_viol + 1 <= S samples to hit: the two eps = 1
    pairs, whose budget is the whole distribution, have none (not a placement that failed: there is no such sample)."""
    out = []
    for (eps, S), m in PAIRS.items():
        for c in sc.cands:
            d, ids = hits(sc, c, S, m, False)
            out.append(cb._instance(sc, "A", "A", eps, S, c, False, hit_ids=ids, dist=d))
            if m + 1 <= S:
                d, ids = hits(sc, c, S, m + 1, False)
                out.append(cb._instance(sc, "B", "B", eps, S, c, True, hit_ids=ids, dist=d))
            d, ids = hits(sc, c, S, m, True)
            out.append(cb._instance(sc, "C", "C", eps, S, c, False, hit_ids=ids, dist=d))
    return out


@functools.lru_cache(maxsize=None)
def instances(name):
    """Every instance of a scene with the oracle's plan (computed once; shared by every test and left unchanged)."""
    sc = scene(name)
    out = pattern_instances(sc)
    for inst in out:
        inst.want = sc.oracle(inst.req, inst.eps, inst.inflation)
        inst.req.dist.setflags(write=False)
    return tuple(out)


def expected_count(sc):
    """instances of a scene: three patterns per pair and target, less the B of the two eps = 1 pairs"""
    return len(sc.cands) * (3 * len(PAIRS) - sum(1 for (e, S), m in PAIRS.items() if m + 1 > S))


def lean_eligible(sc, inst):
    """The launch rule of csrc/fot_host.cpp for a launch of this instance alone or among its like: at most 64 samples
    per candidate, no footprint, no budget."""
    return sc.n_total <= 64 and sc.footprint is None and max_viol(inst.eps, inst.S) == 0
