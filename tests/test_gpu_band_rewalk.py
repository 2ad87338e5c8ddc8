"""The min-only collision walk of k_evaluate and its band re-walk, through plan().

With eps = 0 the sink first walks every chunk of a time step keeping one running float32 minimum per lane: at or below
the sure threshold the candidate is hit, above the miss threshold nothing is near, and only a minimum in the band
between the two sends the lane through the per-chunk walk with its float64 re-check.  Here every instance puts one
target obstacle in that band -- R (1 + delta) from a candidate point, |delta| <= 1e-5, far inside the float32
thresholds' slack -- among a crowd of decoys 1 .. 5 % outside the radius of other lattice points, so that a step's list
spans more than the 32 chunks of one pass of the per-chunk walk.  The target sits first or last in the list.  The same
layout with a chance budget (eps > 0, no min-only walk) checks the other branch of the sink.  Judge: the oracle's
status / keep tables and record, under every evaluation kernel and with float32 tensors.
"""
import numpy as np
import pytest

import eps_band
from helpers import (EVAL_PATHS_NEVER_FLAT as EVAL_PATHS, assert_no_flat_launch, assert_record_matches_oracle,
                     oracle_plan_for_request, set_eval_path)
from oracle import oracle as orc
from test_gpu_collision_boundary import Scene, Target, rounded32

pytestmark = pytest.mark.gpu

BAND_DELTAS = (-1e-5, -1e-6, 1e-6, 1e-5)
N_DECOYS = 320                                   # > 32 chunks of 8 in the step's list


def decoys(sc, rng, k):
    """N_DECOYS static points 1 .. 5 % outside the radius of random lattice points at step k (or their last step)."""
    cands = sc.candidates()
    out = []
    for _ in range(N_DECOYS):
        c = int(rng.choice(cands))
        kk = min(k, int(sc.free.cand_nt[c]) - 1)
        u = ("normal", "rand0", "rand1")[int(rng.integers(0, 3))]
        out.append(Target(sc, c, kk, 0, u, float(rng.uniform(1e-2, 5e-2)), sc.r).pos)
    return np.array(out)


def instances(sc, eps):
    """Per (target candidate, step, delta): eps = 0 -- the target first and last among the static decoys; eps > 0 -- the
    decoys static, the target in one track of a 20-sample distribution, in 1 (within the budget) or 3 samples."""
    rng = np.random.default_rng(2024 + int(eps * 10))
    reqs, labels = [], []
    for c in sc.candidates()[:2]:
        for k in sc.steps(c)[1::2][:2]:
            crowd = decoys(sc, rng, k)
            for d in BAND_DELTAS:
                t = Target(sc, c, k, 0, "normal", d, sc.r)
                if abs(d) < t.floor:
                    continue
                for variant in (0, 1):
                    if eps == 0.0:
                        pts = np.concatenate([t.pos[None], crowd] if variant == 0 else [crowd, t.pos[None]])
                        reqs.append(sc.request(static=pts))
                        labels.append(f"{t.label()} {('first', 'last')[variant]}")
                    else:
                        far = np.repeat((t.pos + 5.0e3)[None], sc.n_t, 0) + np.arange(sc.n_t)[:, None] * 0.01
                        dist = np.repeat(far[None, None], 20, 0)
                        for s_ in (3, 7, 11)[:1 + 2 * variant]:
                            dist[s_, 0, t.k] = t.pos
                        reqs.append(sc.request(static=crowd, dist=dist))
                        labels.append(f"{t.label()} in {1 + 2 * variant} samples")
    return reqs, labels


@pytest.mark.parametrize("scene,eps", [("straight", 0.0), ("far", 0.0), ("arc30", 0.1)])
def test_band_obstacles_among_decoys_match_the_oracle(scene, eps):
    sc = Scene(scene, dict(chance_epsilon=eps))
    reqs, labels = instances(sc, eps)
    assert len(reqs) >= 8
    wants = [oracle_plan_for_request(orc, sc.params, sc.sp, rq, table=True) for rq in reqs]
    wants32 = [oracle_plan_for_request(orc, sc.params, sc.sp, rounded32(rq), table=True) for rq in reqs]
    changed = sum(int((w.cand_status != sc.free.cand_status).any()) for w in wants)
    assert changed >= len(reqs) // 4, f"{scene}: only {changed} of {len(reqs)} instances change a status"
    for path in EVAL_PATHS:
        set_eval_path(sc.bp, path)
        for dtype, ws in ((np.float64, wants), (np.float32, wants32)):
            res = sc.bp.plan_batch(reqs, obstacle_dtype=dtype)
            # (no scene's path is exactly straight: "group" / "split-wave" are the lean kernels, the "-noflat" names add nothing)
            assert_no_flat_launch(sc.bp, f"{scene} eps {eps} [{path}]")
            for i, want in enumerate(ws):
                lab = f"{scene} eps {eps} inst {i} [{path}, {np.dtype(dtype).name}] {labels[i]}"
                _, status, keep, nt = sc.bp.candidates(i)
                np.testing.assert_array_equal(nt, want.cand_nt, err_msg=lab)
                np.testing.assert_array_equal(keep, want.cand_keep, err_msg=lab)
                eps_band.check_status_table(sc.bp, i, status, want.cand_status, lab)
                assert_record_matches_oracle(res.records[i], want, label=lab)
    set_eval_path(sc.bp, "auto")
    sc.bp.close()
