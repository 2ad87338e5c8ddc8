"""Crowds around the wave (64) and workgroup (256) width for the closed-loop kernels -- k_loop_frame, k_predict_cv_frame,
k_loop_pred_error, k_loop_summary, the ragged resample of a frame's distribution -- shared by tests/test_loop_crowds_cpu.py,
tests/test_gpu_loop_crowds.py and the fixture's generator tests/golden/make_closed_loop_crowds.py.

Builders (pure NumPy, deterministic from a seed) and the preconditions that make the crowds worth running: in every
episode the pedestrians that matter to the ego -- the nearest one, those in the lattice's corridor -- have the HIGHEST
indices, everything below them (and the first rows of the next episode) stands at least 40 m to the side.  A kernel that
loses the tail of an episode, or reads a row of its neighbour, changes min_distance and the plan."""
import json
import os

import numpy as np

from conftest import GOLDEN_DIR

LANE = 64                                        # the wave width the kernels stride by
DECOY_SIDE = 40.0                                # decoys stand at least this far to the side [m]

# ---- the resident crowds (section 3): slots on the base scenario's configuration ----------------------------------------
SLOT_COUNTS = (1, 31, 32, 33, 63, 64, 65, 100, 129, 257, 0)
SLOT_FRAMES = tuple(40 if p in (33, 129) else 90 for p in SLOT_COUNTS)   # a short recording: its last frame is held
TRACK_SEED = 7
EXTRA_STEPS = 15                                 # lock steps beyond n_dense: the ring wraps, standard origins complete
REFERENCE_SLOTS = (33, 64, 65, 257)              # pedestrian counts replayed through the reference simulator as well
SOLO_SLOTS = (33, 64, 65, 257)


def matter_count(P):
    """How many pedestrians of an episode of P matter: those of its last (possibly partial) run of 64, three at most --
    so with P > 64 every one of them has an index of 64 or more."""
    return 0 if P <= 0 else min(3, P - LANE * ((P - 1) // LANE))


def crowd_frame(counts, seed, path_y=0.0):
    """One frame of len(counts) episodes: ped_off, ped_pos, ped_vel [sum P, 2], the observer's float32 samples obs_last /
    obs_prev, egos [n, 5] (x, y, yaw, v, a).  Per episode the last ``matter_count(P)`` pedestrians stand in the corridor
    ahead of the ego (8, 14 and 20 m ahead, index P - 1 the nearest); all others are decoys 40 - 70 m to the side."""
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    n = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    egos = np.column_stack([rng.uniform(0.0, 30.0, n), path_y + rng.normal(0.0, 0.3, n), rng.normal(0.0, 0.04, n),
                            rng.uniform(3.0, 8.0, n), rng.uniform(-0.5, 0.5, n)])
    pos = np.zeros((int(off[-1]), 2))
    vel = rng.normal(0.0, 0.8, pos.shape)
    for e, P in enumerate(counts):
        if P == 0:
            continue
        m = matter_count(P)
        x0, y0 = egos[e, 0], egos[e, 1]
        rows = slice(int(off[e]), int(off[e + 1]))
        side = np.where(np.arange(P) % 2 == 0, 1.0, -1.0)
        p = np.column_stack([x0 + rng.uniform(-20.0, 60.0, P), y0 + side * (DECOY_SIDE + 2.0 + rng.uniform(0.0, 28.0, P))])
        ahead = np.array([20.0, 14.0, 8.0])[3 - m:]                    # index P - 1 is the nearest
        lateral = np.array([-0.9, 0.7, 0.3])[3 - m:] + rng.normal(0.0, 0.1, m)
        p[P - m:] = np.column_stack([x0 + ahead, y0 + lateral])
        pos[rows] = p
        vel[rows][P - m:] *= 0.25                                      # (they stay in the corridor over the horizon)
    obs_prev = (pos - 0.4 * vel).astype(np.float32)
    obs_last = (pos + rng.normal(0.0, 0.01, pos.shape)).astype(np.float32)
    return dict(ped_off=off, ped_pos=pos, ped_vel=vel, obs_last=obs_last, obs_prev=obs_prev, egos=egos, counts=counts)


def assert_frame_preconditions(fr):
    """From the inputs alone: per episode with P >= 2 the nearest pedestrian is index P - 1, every pedestrian that does not
    matter -- and the first rows of the next episode -- is at least DECOY_SIDE to the side of the ego."""
    off, pos, egos = fr["ped_off"], fr["ped_pos"], fr["egos"]
    for e, P in enumerate(fr["counts"]):
        lo, hi = int(off[e]), int(off[e + 1])
        m = matter_count(P)
        if P >= 2:
            d = np.hypot(pos[lo:hi, 0] - egos[e, 0], pos[lo:hi, 1] - egos[e, 1])
            assert int(np.argmin(d)) == P - 1, f"episode {e}: nearest pedestrian {int(np.argmin(d))}, not {P - 1}"
        if P > LANE:
            assert P - m >= LANE, f"episode {e}: a pedestrian that matters below index {LANE}"
        tail = pos[lo:hi - m]
        assert (np.abs(tail[:, 1] - egos[e, 1]) >= DECOY_SIDE).all(), f"episode {e}: a decoy closer than {DECOY_SIDE} m"
        nxt = next((k for k in range(e + 1, len(fr["counts"])) if fr["counts"][k] > 0), None)
        if nxt is not None and fr["counts"][nxt] > matter_count(fr["counts"][nxt]):   # what a read past the end would see
            first = pos[int(off[nxt])]
            assert abs(first[1] - egos[e, 1]) >= DECOY_SIDE, f"episode {e}: the next episode's first row is no decoy"


def crowd_tracks(counts, n_frames, seed, dt=0.1):
    """Recordings [n_frames_i][P_i][2] for a resident loop whose ego starts at the origin along +x (frame spacing dt).

    Columns 0 .. P - 3 are decoys 42 m and more to the side that walk along the road and weave across their heading
    (amplitude 0.2 m + 1 cm per index, phase 0.05 rad per index: the constant-velocity predictor's error is non-zero and
    different for every pedestrian); column P - 2 walks beside the road, column P - 1 -- the nearest -- crosses it ahead
    of the ego, so that the planner reacts."""
    rng = np.random.default_rng(seed)
    frames = [int(n_frames)] * len(counts) if np.ndim(n_frames) == 0 else [int(f) for f in n_frames]
    out = []
    for P, nf in zip(counts, frames):
        P = int(P)
        t = np.arange(nf) * dt
        tr = np.zeros((nf, P, 2))
        j = np.arange(max(P - 2, 0))
        side = np.where(j % 2 == 0, 1.0, -1.0)
        x0, y0 = rng.uniform(-5.0, 60.0, len(j)), side * (45.0 + rng.uniform(0.0, 20.0, len(j)))
        speed = rng.uniform(0.6, 1.5, len(j)) * np.where(rng.random(len(j)) < 0.5, 1.0, -1.0)
        amp, phase = 0.2 + 0.01 * j, 0.05 * j
        if len(j):
            tr[:, :P - 2, 0] = x0[None, :] + speed[None, :] * t[:, None]
            tr[:, :P - 2, 1] = y0[None, :] + amp[None, :] * np.sin(2.0 * np.pi * t[:, None] / 4.0 + phase[None, :])
        jx, jy = rng.uniform(0.0, 4.0), rng.uniform(-1.0, 1.0)
        if P >= 2:                                                     # beside the road, along it
            tr[:, P - 2, 0] = 44.0 + jx + 1.2 * t
            tr[:, P - 2, 1] = 4.6 + 0.15 * np.sin(2.0 * np.pi * t / 3.0 + 0.3 * P)
        if P >= 1:                                                     # across the road, ahead of the ego
            tr[:, P - 1, 0] = 37.0 + jx + 0.12 * np.sin(2.0 * np.pi * t / 5.0 + 0.1 * P)
            tr[:, P - 1, 1] = -9.0 + jy + 1.1 * t
        out.append(tr)
    return out


def slot_tracks():
    """The recordings of the resident crowds (SLOT_COUNTS / SLOT_FRAMES / TRACK_SEED)."""
    return crowd_tracks(SLOT_COUNTS, SLOT_FRAMES, TRACK_SEED)


def rolling_mean_displacement(track, n_steps, n_dense, dt=0.1, sgan_dt=0.4, obs_len=8, keep=None):
    """summary_of_history's rolling mean displacement (planning_ade) of n_steps lock steps, restated from a recording
    alone: the observer samples every sgan_dt of pedestrian time from the warm-up on, the constant-velocity prediction
    continues the last two samples, the truth of dense sample k of step i is frame min(f_i + 1 + k, last), cut to the
    steps that follow i.  keep: the pedestrian columns counted (None: all)."""
    track = np.asarray(track, float)
    if keep is not None:
        track = track[:, keep]
    stride = int(round(sgan_dt / dt))
    last_row = len(track) - 1
    total, count = 0.0, 0
    for i in range(n_steps):
        f = obs_len * stride + 1 + i                                  # the frame of lock step i
        f_last = (f // stride) * stride                               # the observer's last sample, the one before it
        a, b = track[min(f_last, last_row)], track[min(f_last - stride, last_row)]
        v = (a - b) / sgan_dt
        stale = (f - f_last) * dt
        E = min(n_dense, n_steps - 1 - i)
        if E <= 0 or track.shape[1] == 0:
            continue
        k = np.arange(E)
        pred = a[:, None, :] + v[:, None, :] * ((k + 1) * dt + stale)[None, :, None]
        truth = track[np.minimum(f + 1 + k, last_row)].transpose(1, 0, 2)
        total += float(np.hypot(*(pred - truth).transpose(2, 0, 1)).mean(axis=1).sum())
        count += track.shape[1]
    return total / count if count else float("nan")


def assert_track_preconditions(tracks, n_steps, n_dense):
    """From the recordings alone: decoys stay 40 m to the side; in every slot with P >= 2 the nearest pedestrian to the
    ego's start is index P - 1 at the first step's frame; with P > 64, dropping pedestrians 64 and up changes the rolling
    mean displacement by more than 1e-3 relative."""
    for tr in tracks:
        P = tr.shape[1]
        if P >= 3:
            assert (np.abs(tr[:, :P - 2, 1]) >= DECOY_SIDE).all()
        if P >= 2:
            row = tr[min(33, len(tr) - 1)]
            assert int(np.argmin(np.hypot(row[:, 0], row[:, 1]))) == P - 1
        if P > LANE:
            full = rolling_mean_displacement(tr, n_steps, n_dense)
            cut = rolling_mean_displacement(tr, n_steps, n_dense, keep=slice(0, LANE))
            assert abs(full - cut) > 1e-3 * abs(full), f"P = {P}: {full!r} with all, {cut!r} with the first {LANE}"


def load_crowd_episodes():
    """tests/golden/make_closed_loop_crowds.py: the reference simulator's own runs of the REFERENCE_SLOTS recordings, in
    the key layout of reference_cv_episodes.npz (variants "p33", "p64", ...), plus ``<name>_summary``."""
    z = np.load(os.path.join(GOLDEN_DIR, "closed_loop", "reference_crowd_episodes.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def summary_rtol(steps, n_dense, P, floor):
    """The relative tolerance of a mean of non-negative float64 terms summed in another order: n 2^-53 for n terms (the
    bound summary_common.py documents for its SUM_RTOL = 1e-10, which covers 2e5 terms).  A slot's prediction-error means
    add steps x n_dense x P distances at the most, so n = steps * n_dense * P; never below the documented floor."""
    return max(floor, steps * n_dense * P * 2.0 ** -53)


# ---- the single frames (sections 1 and 2): name -> (pedestrian counts, seed) ---------------------------------------------
FRAME_CASES = {"wave": ([63, 64, 65, 0, 1, 128, 129], 101), "block": ([257, 5, 300], 102)}
GROWTH_FRAMES = (([5, 3], 103), ([300, 64], 104), ([5, 3], 105))     # one handle: its frame block grows, then shrinks
DIST_CASES = {"s2": (2, [65, 0, 64, 1, 130], 106), "s64": (64, [65, 3], 107)}
