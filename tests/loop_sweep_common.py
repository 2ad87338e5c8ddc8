"""Shared by tests/test_loop_sweep_cpu.py and tests/test_gpu_loop_sweep.py: the NumPy restatement of csrc/fot_sweep.hpp's
layout arithmetic, the conditions of a sweep over the ragged crowd (recorded_samples_common) and the uniform loop a slot
of a sweep is held against."""
import numpy as np

import recorded_samples_common as rs
from closed_loop_common import load_episodes, scenario_config
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.prediction import RecordedSamples

DIST, REP = _abi.LOOP_PLAN_DISTRIBUTION, _abi.LOOP_PLAN_REPRESENTATIVE


# ---- the layout arithmetic, restated -------------------------------------------------------------------------------------------
def layout(counts, slots, slot_mode, dist_end, T, select_all=False):
    """(tensor size in points, rep_off [n_run] -- -1: the episode plans on its distribution --, select [n_run]) of a frame
    whose running episode i has counts[i] pedestrians and sits on slot slots[i]; Python's unbounded integers."""
    end, off, sel = int(dist_end), [], []
    for P, e in zip(counts, slots):
        rep = int(slot_mode[e]) == REP
        off.append(end if rep else -1)
        sel.append(1 if rep or select_all else 0)
        if rep:
            end += int(P) * int(T)
    return end, off, sel


def dist_end(counts, S, T):
    """Points of the frame's distribution blocks [S][P][T][2]."""
    return sum(int(S) * int(P) * int(T) for P in counts)


def columns(counts, slots, slot_col0):
    """Column of the recording of every row of the frame: row r of running episode i reads slot_col0[slots[i]] + r."""
    return [int(slot_col0[e]) + r for P, e in zip(counts, slots) for r in range(int(P))]


def columns_fit(slot_counts, slot_col0, n_rec_cols):
    return all(int(c) >= 0 and int(c) + int(P) <= int(n_rec_cols) for P, c in zip(slot_counts, slot_col0))


# ---- a sweep over the ragged crowd ----------------------------------------------------------------------------------------------
SWEEP_S = 6                                       # floor(0.2 * 6) = 1 sample may violate under chance_epsilon = 0.2
SWEEP_STEPS = 28                                  # slots 0, 2 and 4 of the ragged crowd have ended by then
# slot -> (path, distribution_aware_planning, chance_epsilon, collision_margin_inflation): modes alternate, slots 0 and 4
# share a scenario, slots 1 and 3 differ in the inflation only (chance_epsilon plays no part in representative mode)
RAGGED_CONDITIONS = (("base", True, 0.2, 1.0), ("turn", False, 0.0, 1.1), ("base", True, 0.0, 1.1),
                     ("turn", False, 0.2, 1.0), ("base", True, 0.2, 1.0))


def condition(path, aware, eps, inflation, pred_len=12):
    cfg = dict(scenario_config(load_episodes()["meta"], path), pred_len=int(pred_len), chance_epsilon=float(eps),
               collision_margin_inflation=float(inflation))
    cfg["distribution_aware_planning"] = bool(aware)
    return cfg


def ragged_conditions(pred_len=12):
    return [condition(*c, pred_len=pred_len) for c in RAGGED_CONDITIONS]


def ragged_egos(cfgs):
    """Every slot starts where its own configuration says; slot 0 just short of the goal of its 60 m path."""
    egos = [list(c["ego_initial_state"]) for c in cfgs]
    egos[0] = [rs.GOAL_START] + egos[0][1:]
    return egos


def modes_of(cfgs):
    return np.array([DIST if c["distribution_aware_planning"] else REP for c in cfgs], np.int32)


def loop(cfg, tracks, egos, source, resident, **kw):
    """A loop over `tracks`: cfg a list -- the sweep --, or one configuration -- the uniform loop of that condition."""
    aware = [c["distribution_aware_planning"] for c in (cfg if isinstance(cfg, list) else [cfg])]
    if not all(aware):
        kw = dict(kw, plan_on_representative_sample=True)
    return BatchedClosedLoop(cfg, tracks, egos, sample_source=source, device_samples=True, resident=resident, **kw)


def recorded(samples, **kw):
    return RecordedSamples(samples, **kw)


def same_metric(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))
