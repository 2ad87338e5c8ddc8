"""Shared by the CPU and GPU tests of planning on the representative prediction sample (fot_loop_plan_sample): NumPy
restatements of the selection (predict_single_best), of the reference's conditional prepend and of the fixed-shape block."""
import numpy as np

ATOL, RTOL = 1e-8, 1e-5                          # np.allclose's defaults (integrated_simulator.py:508-513)
GAP = 1e-9                                       # the two smallest deviation sums differ by more than this, relative


def deviation_sums(dist, off):
    """dist [S, sum P, K, 2] (dense samples only), off [n + 1] -> [S, n]: per episode the sum over its own pedestrians and
    the dense samples of |sample - sample mean| (trajectory_predictor.py:346-351); 0 for an episode without pedestrians."""
    dev = np.linalg.norm(dist - dist.mean(axis=0)[None], axis=-1).sum(axis=2)      # [S, sum P]
    return np.stack([dev[:, off[i]:off[i + 1]].sum(axis=1) for i in range(len(off) - 1)], axis=1)


def host_choice(dist, off):
    """np.argmin per episode, -1 without pedestrians."""
    sums = deviation_sums(dist, off)
    best = np.argmin(sums, axis=0)
    best[np.diff(off) == 0] = -1
    return best


def gaps(dist, off):
    """Per episode with pedestrians and more than one sample: (second smallest - smallest) / second smallest deviation sum."""
    sums = deviation_sums(dist, off)
    out = []
    for i in range(sums.shape[1]):
        if off[i + 1] > off[i] and sums.shape[0] > 1:
            two = np.sort(sums[:, i])[:2]
            out.append((two[1] - two[0]) / two[1] if two[1] > 0 else 0.0)
    return np.array(out)


def prepend_rule(first, cur):
    """True: the current positions lead the block -- unless |first - cur| <= atol + rtol |cur| for every pedestrian on both
    axes (closed_loop.py's form of np.allclose; a NaN makes it false)."""
    first, cur = np.asarray(first, float), np.asarray(cur, float)
    with np.errstate(invalid="ignore"):
        return not bool(np.all(np.abs(first - cur) <= ATOL + RTOL * np.abs(cur)))


def host_block(chosen, cur):
    """chosen [P, n_dense, 2] (the episode's representative sample), cur [P, 2] -> ([P, n_dense + 1, 2], prepended)."""
    pre = prepend_rule(chosen[:, 0], cur)
    if pre:
        return np.concatenate([cur[:, None, :], chosen], axis=1), True
    return np.concatenate([chosen, chosen[:, -1:]], axis=1), False


# ---- the closed-loop episodes of the sampler tests ----------------------------------------------------------------------------
LOOP_MODEL, LOOP_SAMPLES, LOOP_STEPS = "a_pool_step_ped_bn", 4, 12
LOOP_SEED = 0x5EED0123456789AB


def loop_inputs():
    """(configuration, tracks): the weave episode of the prediction-score fixture without distribution_aware_planning, a
    wall of pedestrians charging the ego (an early collision) and an episode without pedestrians."""
    import sgan_common as sc
    from pred_scores_common import load_cases
    fx = load_cases()
    cfg = dict(fx["meta"]["episodes"]["weave_s4"]["config"], distribution_aware_planning=False)
    return cfg, [sc.charging_wall_tracks(), fx["weave_s4_ped_traj"][:, :0], fx["weave_s4_ped_traj"]]
