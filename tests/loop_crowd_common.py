"""Shared by tests/test_loop_crowd_sampler_cpu.py and tests/test_gpu_loop_crowd_sampler.py: the NumPy restatement of the
crowd tables and of the consistency check of csrc/fot_sweep.hpp (fot_loop_set_sampler_shared), the two seeded Social-GAN
models and the crowds of 3 and 17 pedestrians (17 crosses the generator's 16-row tile) the GPU tests run."""
import numpy as np

import loop_crowds_common as lc
import loop_sweep_common as sw
import recorded_samples_common as rs
import sgan_common as sc
from closed_loop_common import load_episodes, scenario_config
from integrated_path_planning_amd.prediction import SganWeights

S = sw.SWEEP_S
SEED = 20240611
PER_PED_MODEL, PER_SCENE_MODEL = "a_pool_step_ped_bn", "a_pool_step_global"     # noise per pedestrian / per scene (FOT_SGAN_NOISE_GLOBAL)
CROWD_COUNTS = (3, 17)
CROWD_FRAMES = 90


# ---- the crowd tables, restated ---------------------------------------------------------------------------------------------------
def crowd_tables(counts, slots, slot_crowd):
    """The tables of a frame whose running episode i has counts[i] pedestrians and sits on slot slots[i]:
    dict(scene_off, scene_slot, scene_crowd, row_scene, col, identity).  A crowd is active when one of its running slots has
    pedestrians; the active crowds in ascending id are the scenes; a scene's rows are those of the crowd's lowest such slot."""
    rep = {}
    for i, (P, e) in enumerate(zip(counts, slots)):
        c = int(slot_crowd[e])
        if P > 0 and (c not in rep or e < slots[rep[c]]):
            rep[c] = i
    crowds = sorted(rep)
    scene_of = {c: k for k, c in enumerate(crowds)}
    scene_P = [int(counts[rep[c]]) for c in crowds]
    scene_off = [0]
    for P in scene_P:
        scene_off.append(scene_off[-1] + P)
    col = [scene_off[scene_of[int(slot_crowd[e])]] + r for P, e in zip(counts, slots) for r in range(int(P))]
    return dict(scene_off=scene_off, scene_slot=[int(slots[rep[c]]) for c in crowds], scene_crowd=crowds,
                row_scene=[k for k, P in enumerate(scene_P) for _ in range(P)], col=col,
                identity=col == list(range(len(col))) and scene_off[-1] == int(sum(counts)))


def crowds_consistent(counts, frames, slot_crowd, pos):
    """(code, slot a, slot b): every slot against the lowest slot of its crowd -- 0: all agree (a = b = -1); 1: the
    pedestrian counts differ; 2: the recorded frames; 3: some byte of the positions [n_frames_max, sum P, 2] of a recorded
    frame."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    for e in range(len(counts)):
        a = next(k for k in range(e + 1) if slot_crowd[k] == slot_crowd[e])
        if a == e:
            continue
        if counts[a] != counts[e]:
            return 1, a, e
        if frames[a] != frames[e]:
            return 2, a, e
        pa, pe = pos[:frames[e], off[a]:off[a + 1]], pos[:frames[e], off[e]:off[e + 1]]
        if np.ascontiguousarray(pa).tobytes() != np.ascontiguousarray(pe).tobytes():
            return 3, a, e
    return 0, -1, -1


# ---- models, crowds and conditions of the GPU tests ----------------------------------------------------------------------------------
def weights(name=PER_PED_MODEL):
    a = sc.case_args(name)
    return SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)))


def base_config(**kw):
    return dict(scenario_config(load_episodes()["meta"], "base"), **kw)


def crowds():
    """Two crowds of 3 and 17 pedestrians (loop_crowds_common.crowd_tracks: the last pedestrian crosses the road ahead)."""
    return lc.crowd_tracks(CROWD_COUNTS, CROWD_FRAMES, lc.TRACK_SEED + 4)


def walled(track, ahead):
    """The crowd with its last three pedestrians charging at the ego from `ahead` metres: the slots over it end in a
    collision within a few lock steps, whatever their condition."""
    out = track.copy()
    out[:, -3:] = rs.charging_wall(len(out), ahead)
    return out
