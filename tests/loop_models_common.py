"""Shared by tests/test_loop_models_cpu.py and tests/test_gpu_loop_models.py (fot_loop_set_sampler_models: a Social-GAN
model per slot of a sampler loop): the seeded models, the frames the table tests run and what csrc/fot_sweep.hpp's
sweep_model_tables must print for a frame according to prediction.model_scenes."""
import numpy as np

import loop_crowd_common as cr
import sgan_common as sc
from integrated_path_planning_amd.prediction import SganWeights, model_scenes

S, SEED = cr.S, cr.SEED
# the pooled checkpoint ('sgan') and the no-pooling one ('lstm') of another dimension set: noise width 8 against 4
POOLED, NO_POOLING = "a_pool_once_ped", "b_none_ped_bn"
PER_SCENE, POOL_STEPS = "a_pool_once_global", "a_pool_step_ped_bn"

_weights = {}


def weights(name, **over):
    """The seeded model of sgan_common's case `name`, its constructor arguments overridden by `over` (pred_len, noise_type)."""
    key = (name, tuple(sorted(over.items())))
    if key not in _weights:
        a = dict(sc.case_args(name), **over)
        _weights[key] = SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)))
    return _weights[key]


# name -> (pedestrian count of every slot, crowd of every slot, model of every slot, models of the loop, running slots)
SIX_P, SIX_CROWD, SIX_MODEL = [3, 17, 3, 17, 17, 3], [0, 1, 0, 1, 1, 0], [0, 0, 1, 1, 0, 1]
FRAMES = {
    "interleaved, every slot running": (SIX_P, SIX_CROWD, SIX_MODEL, 2, [0, 1, 2, 3, 4, 5]),
    "the lowest slot of a unit ended": (SIX_P, SIX_CROWD, SIX_MODEL, 2, [0, 2, 3, 4, 5]),            # unit (1, 0): slot 4 stands for it
    "a unit ended, its crowd runs on under the other model": (SIX_P, SIX_CROWD, SIX_MODEL, 2, [0, 2, 3, 5]),
    "a model with no active unit": (SIX_P, SIX_CROWD, SIX_MODEL, 2, [0, 1, 4]),
    "a model no slot names": (SIX_P, SIX_CROWD, [0, 0, 2, 2, 0, 2], 3, [0, 1, 2, 3, 4, 5]),
    "slots with no pedestrians": ([0, 5, 0, 5, 2, 0], [1, 0, 1, 0, 2, 2], [0, 1, 1, 0, 1, 0], 2, [0, 1, 2, 3, 4, 5]),
    "a unit whose only slots have no pedestrians": ([0, 5, 0], [1, 0, 1], [1, 0, 1], 2, [0, 1, 2]),
    "one crowd, two models": ([9, 9, 9, 9], [0, 0, 0, 0], [0, 0, 1, 1], 2, [0, 1, 2, 3]),
    "models in descending slot order": ([4, 4, 9, 9], [7, 7, 40, 40], [1, 0, 1, 0], 2, [0, 1, 2, 3]),
    "one model": (SIX_P, SIX_CROWD, [0] * 6, 1, [0, 1, 2, 3, 4, 5]),
    "one model, slots ended": (SIX_P, SIX_CROWD, [0] * 6, 1, [2, 4, 5]),
    "eight models": ([2] * 8, [0] * 8, list(range(8)), 8, list(range(8))),
    "no slot running": (SIX_P, SIX_CROWD, SIX_MODEL, 2, []),
}


def fuzzed_frames(n, seed):
    """n random frames: up to 12 slots over up to 4 crowds (the slots of a crowd agree in their pedestrian count, a third of
    the crowds have none) and up to 4 models, a random subset of the slots still running."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in range(n):
        n_slots, n_crowds, n_models = int(rng.integers(1, 13)), int(rng.integers(1, 5)), int(rng.integers(1, 5))
        crowd_P = np.where(rng.random(n_crowds) < 1 / 3, 0, rng.integers(1, 40, n_crowds))
        crowd = rng.integers(0, n_crowds, n_slots)
        model = rng.integers(0, n_models, n_slots)
        running = np.flatnonzero(rng.random(n_slots) < 0.7)
        ids = rng.permutation(50)[:n_crowds]                          # (ids that are not dense)
        out[f"fuzzed {k}"] = (crowd_P[crowd].tolist(), ids[crowd].tolist(), model.tolist(), n_models, running.tolist())
    return out


def expected_tables(slot_P, crowd, model, n_models, running, pred_len=3, s=2, j=1):
    """The numbers tests/emu/fot_model_emu.cpp prints for the frame, formed from prediction.model_scenes."""
    counts = np.array([slot_P[e] for e in running], dtype=np.int64)
    slots = np.array(running, dtype=np.int64)
    units, row_model, cols = model_scenes(slots, counts, [11] * len(running), crowd, model)
    units = list(units) + [(np.zeros(0, np.int64),) * 3] * (n_models - len(units))
    want, widths = [], []
    for crowds, rep, noise_slots in units[:n_models]:
        assert list(noise_slots) == list(crowds)
        P = counts[rep]
        widths.append(int(P.sum()))
        want += [len(rep), int(P.sum())] + np.concatenate([[0], np.cumsum(P)]).astype(int).tolist() + slots[rep].tolist() \
            + crowds.tolist() + np.repeat(np.arange(len(rep)), P).tolist()
    want += row_model.tolist() + cols.tolist()
    for m, c in zip(row_model.tolist(), cols.tolist()):
        want += [1000 * m, widths[m], c, 1000 * m + (s * pred_len + j) * widths[m] + c]
    return want


def case_line(slot_P, crowd, model, n_models, running):
    counts = [slot_P[e] for e in running]
    return " ".join(map(str, ["models", len(running)] + counts + list(running) + [len(crowd)] + list(crowd) + list(model) + [n_models]))
