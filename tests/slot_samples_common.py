"""Shared by tests/test_slot_samples_cpu.py and tests/test_gpu_slot_samples.py (a sample count per slot of a sweep loop,
fot_loop_set_slot_samples): the NumPy restatement of the ragged layout of csrc/fot_sweep.hpp, and the ragged crowd of
loop_sweep_common with two pedestrians moved so that the sample count MATTERS on it -- a test that passes with the counts
ignored shows nothing."""
import numpy as np

import loop_sweep_common as sw
import recorded_samples_common as rs

COUNTS = (6, 1, 4, 6, 3)                          # slot -> samples it keeps of the 6-sample recording (loop_sweep_common.SWEEP_S)
assert max(COUNTS) == sw.SWEEP_S

# ---- the layout, restated (Python's unbounded integers) -----------------------------------------------------------------------------
def frame(counts, slots, slot_S, slot_mode, T, select_all=False):
    """(largest count, counts [n_run], blk [n_run + 1], tensor size, rep_off [n_run], select [n_run]) of a frame whose
    running episode i has counts[i] pedestrians and sits on slot slots[i]."""
    ep_S = [int(slot_S[e]) for e in slots]
    blk = [0]
    for P, S in zip(counts, ep_S):
        blk.append(blk[-1] + S * int(P) * int(T))
    size, off, sel = sw.layout(counts, slots, slot_mode, blk[-1], T, select_all)
    return max(ep_S, default=0), ep_S, blk, size, off, sel


def capacity(slot_counts, slot_S, T):
    return sum((int(S) + 1) * int(P) * int(T) for P, S in zip(slot_counts, slot_S))


# ---- a crowd on which the count matters ---------------------------------------------------------------------------------------------
# (x0, y0, vx, vy): where the moved pedestrian stands when the warm-up ends and how it walks [m, m/s].  Found by running
# the oracle loop over a grid of such walkers (tests/test_slot_samples_cpu.py asserts what they were chosen for).
REP_WALKER = (4.0, 2.5, -0.5, -0.6)               # the one pedestrian of slot 1, ahead of the 'turn' path's bend
EPS_WALKER = (7.0, 1.6, -0.8, -0.3)               # pedestrian 0 of the crowd the two-slot chance-budget sweep runs over
EPS_CROWD = 3                                     # that crowd: slot 3's 65 pedestrians (no charging wall: it runs on)
EPS_CONDITION = ("base", True, 0.2, 1.0)          # floor(0.2 * 6) = 1 sample may violate, floor(0.2 * 4) = 0


def walker(x0, y0, vx, vy, n_frames=rs.RAGGED_FRAMES, warmup_frames=32, dt=0.1):
    f = np.arange(n_frames, dtype=np.float64) - warmup_frames
    return np.stack([x0 + vx * dt * f, y0 + vy * dt * f], axis=-1)


def tracks():
    """loop_sweep_common's ragged crowd (0, 1, 33, 65 and 30 pedestrians) with the pedestrian of slot 1 moved."""
    out = [t.copy() for t in rs.ragged_tracks()]
    out[1][:, 0] = walker(*REP_WALKER)
    return out


def eps_crowd():
    """The crowd of the chance-budget premise: slot EPS_CROWD's pedestrians with pedestrian 0 moved."""
    crowd = rs.ragged_tracks()[EPS_CROWD].copy()
    crowd[:, 0] = walker(*EPS_WALKER)
    return crowd


def prefix(rec, k):
    """The first k samples of a recording [n_steps, S, pred_len, cols, 2]."""
    return np.ascontiguousarray(rec[:, :int(k)])
