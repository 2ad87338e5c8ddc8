"""Shared by the tests of sample distributions of more than 64 samples in the closed loop, the samplers and the scores
(a handle with a raised sample capacity): the scripted sample source of the reference fixture
tests/golden/closed_loop/reference_wide_episodes.npz -- called by the reference run that made the fixture and by the
tests that replay it, so the fixture stores results only --, fixture access, and the NumPy restatement of the
representative sample."""
import json
import os

import numpy as np

from conftest import GOLDEN_DIR

# (beside the other episode fixtures, NOT at the top of tests/golden/: conftest.golden_names() feeds every top-level case
#  to the golden plan tests)
FIXTURE = os.path.join(GOLDEN_DIR, "closed_loop", "reference_wide_episodes.npz")
FAN_HALF_ANGLE = 0.6                              # [rad] the whole fan, whatever the number of samples


def wide_raw_sample(obs_last, obs_prev, k, n_samples, pred_len, sgan_dt):
    """Sample k of the scripted multi-sample predictor for LARGE sample counts: [pred_len, P, 2] positions at the
    predictor's own step.  As closed_loop_common.scripted_raw_sample -- every pedestrian keeps walking with its last
    observed velocity, turned by a sample-dependent angle and scaled by a sample-dependent factor -- but the turning
    angles are spread evenly over a FIXED fan of +-FAN_HALF_ANGLE, where that function turns by 0.08 rad per sample
    (+-5 rad at 130 samples: pedestrians walking backwards).  Plain NumPy float64 on both sides."""
    obs_last, obs_prev = np.asarray(obs_last, np.float64), np.asarray(obs_prev, np.float64)
    vel = (obs_last - obs_prev) / sgan_dt
    ang = FAN_HALF_ANGLE * (2.0 * k / (n_samples - 1) - 1.0) if n_samples > 1 else 0.0
    gain = 1.0 + 0.06 * ((k % 3) - 1)
    c, s_ = np.cos(ang) * gain, np.sin(ang) * gain
    v = np.stack([c * vel[:, 0] - s_ * vel[:, 1], s_ * vel[:, 0] + c * vel[:, 1]], axis=1)
    steps = (np.arange(pred_len) + 1.0) * sgan_dt
    return obs_last[None, :, :] + steps[:, None, None] * v[None, :, :]


def wide_sample_source(n_samples, pred_len, sgan_dt=0.4):
    """``(obs_last, obs_prev) -> [S, pred_len, P, 2]``: what BatchedClosedLoop takes as sample_source."""
    return lambda obs_last, obs_prev: np.stack([wide_raw_sample(obs_last, obs_prev, k, n_samples, pred_len, sgan_dt)
                                                for k in range(n_samples)])


def load_wide_episodes():
    """tests/golden/make_closed_loop_wide.py: the layout of closed_loop/reference_dist_episodes.npz."""
    z = np.load(FIXTURE, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def predict_single_best(block, skip=1):
    """predict_single_best (trajectory_predictor.py:346-351) on a block [S, P, T, 2] whose first ``skip`` time entries
    are not part of it: (index of the first minimum, the S deviation sums)."""
    q = np.asarray(block, np.float64)[:, :, skip:]
    dev = np.linalg.norm(q - q.mean(axis=0)[None], axis=-1).sum(axis=(1, 2))
    return int(np.argmin(dev)), dev


def tie_block(rng, S, P, T, a=63, b=64):
    """A distribution [S, P, T, 2] whose samples a and b are the same numbers -- their deviation sums are the same
    operations on the same values, an exact tie -- and lie closest to the mean: the FIRST of the two is the representative
    sample.  The others are pushed away from the centre in pairs of opposite directions."""
    centre = rng.uniform(-30.0, 30.0, (1, P, 1, 2)) + np.cumsum(rng.normal(0.0, 0.2, (1, P, T, 2)), axis=2)
    off = rng.uniform(1.0, 2.0, (S, 1, 1, 2)) * np.where(np.arange(S) % 2 == 0, 1.0, -1.0)[:, None, None, None]
    blk = centre + off + rng.normal(0.0, 0.05, (S, P, T, 2))
    blk[a] = centre[0] + 0.01
    blk[b] = blk[a]
    return np.ascontiguousarray(blk)
