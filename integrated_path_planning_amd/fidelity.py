"""Fidelity statistics of vehicle-pedestrian encounters (RQ2): how close pedestrians come to the vehicle and at what distance
they begin to evade it, simulated against recorded.

The reference's ``min_separation_series``, ``avoidance_onset_distance``, ``compare_distributions_ks``,
``ks_sample_imbalance`` and ``calculate_min_separation`` (src/core/metrics.py) and the measuring half of
``fidelity_report`` / ``objective_rollout_ade`` (src/simulation/calibration_harness.py), with ``engine`` (a
``BatchPlanner``) first.  The Social-Force roll-out is not part of this package: the caller brings the simulated positions
from wherever they were rolled out.  Everything measured on [T, N, 2] arrays -- distances, gradients, the onset search, the
error sums -- runs on the device in ``fot_fidelity_eval``, any number of ragged encounters per call; the pooling, the
medians and the KS test stay on the host, in the reference's order."""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .batch import PackedEncounters

REPORT_KEYS = ("n_encounters", "rollout_ade", "mean_closest_sim", "mean_closest_real", "ks_closest", "p_closest",
               "n_onset_sim", "n_onset_real", "ks_onset", "p_onset", "closest_sim_raw", "closest_real_raw", "onset_sim_raw",
               "onset_real_raw", "onset_per_enc_sim_raw", "onset_per_enc_real_raw")
_warned_scipy = False


def _get(enc, name, default=None):
    return enc.get(name, default) if isinstance(enc, dict) else getattr(enc, name, default)


def fidelity_batch(engine, encounters: Sequence, rollouts: Optional[Sequence] = None, ped_vel: bool = False,
                   accel_threshold: float = 0.3, max_distance: float = 5.0, interaction_distance: Optional[float] = None):
    """One ``fot_fidelity_eval`` call over ``encounters`` (objects or dictionaries with ``ego_xy`` [T, 2], ``ped_xy``
    [T, N, 2], ``dt`` and optionally ``ped_vel``).

    Without ``rollouts`` the encounters' own ``ped_xy`` are measured.  With ``rollouts`` (one [T, N, 2] array per
    encounter) the roll-outs are measured against the encounters' egos, and the encounters' ``ped_xy`` are the truth of the
    roll-out error.  ``ped_vel=True`` takes the velocity from the encounters (recorded side only) instead of differencing
    the positions.  Returns a dictionary: ``records`` (``batch.FIDELITY_ENC_DT`` per encounter: closest, closest_step,
    n_onset, err_sum, err_count), ``series`` (one [T] array per encounter), ``onset_dist`` and ``onset_step`` (one [N]
    array per encounter; NaN / -1: the pedestrian never evades)."""
    encounters = list(encounters)
    recorded = [_get(e, "ped_xy") for e in encounters]
    if rollouts is not None:
        rollouts = list(rollouts)
        if len(rollouts) != len(encounters):
            raise ValueError("one roll-out per encounter")
        if ped_vel:
            raise ValueError("a roll-out has no recorded velocity: ped_vel applies to the recorded side only")
    vel = None
    if ped_vel:
        vel = [_get(e, "ped_vel") for e in encounters]
        if any(v is None for v in vel):
            raise ValueError("ped_vel=True needs every encounter's ped_vel")
    packed = PackedEncounters([_get(e, "ego_xy") for e in encounters], recorded if rollouts is None else rollouts,
                              [float(_get(e, "dt", 0.4)) for e in encounters], ped_vel=vel,
                              truth_xy=None if rollouts is None else recorded)
    rec, series, dist, step = engine.fidelity_eval(packed, accel_threshold=accel_threshold, max_distance=max_distance,
                                                   interaction_distance=interaction_distance)
    so, pb = packed.step_off, packed.ped_base
    n = packed.n
    return dict(records=rec, series=[series[so[i]:so[i + 1]] for i in range(n)],
                onset_dist=[dist[pb[i]:pb[i + 1]] for i in range(n)], onset_step=[step[pb[i]:pb[i + 1]] for i in range(n)])


def min_separation_series(engine, ego_xy, ped_xy) -> np.ndarray:
    """Per-step minimum ego-pedestrian distance [T] (inf where N == 0).  The C entry has no way to ask for the series
    alone: this is a whole ``fot_fidelity_eval`` call of one encounter, whose onset walk runs and is discarded.  For many
    encounters use ``fidelity_batch``, which returns every series of one call."""
    steps = (len(ego_xy), len(ped_xy))
    if steps[0] != steps[1]:
        raise ValueError(f"ego_xy T={steps[0]} != ped_xy T={steps[1]}")
    if steps[0] == 0:
        return np.zeros(0)
    return fidelity_batch(engine, [dict(ego_xy=ego_xy, ped_xy=ped_xy, dt=0.4)])["series"][0]


def avoidance_onset_distance(engine, ego_xy, ped_xy, ped_vel=None, dt: float = 0.4, accel_threshold: float = 0.3,
                             max_distance: float = 5.0) -> np.ndarray:
    """Ego-pedestrian distance at which each pedestrian starts evading the ego: 1-D, one entry per pedestrian that
    evades, in pedestrian order."""
    have_vel = ped_vel is not None
    shape = np.shape(ped_xy)
    if have_vel and np.shape(ped_vel) != shape:
        raise ValueError(f"ped_vel shape {np.shape(ped_vel)} != ped_xy shape {shape}")
    if shape[0] <= 1 or shape[1] < 1:                              # one step has no gradient; nobody to evade
        return np.zeros(0)
    out = fidelity_batch(engine, [dict(ego_xy=ego_xy, ped_xy=ped_xy, ped_vel=ped_vel, dt=dt)], ped_vel=have_vel,
                         accel_threshold=accel_threshold, max_distance=max_distance)
    return out["onset_dist"][0][out["onset_step"][0] >= 0]


KS_LATTICE_MAX_N = 10000


def _ks_statistic(a: np.ndarray, b: np.ndarray) -> float:
    """The largest difference of the two empirical CDFs.  Its true value is a multiple of 1 / lcm(n_a, n_b): up to
    KS_LATTICE_MAX_N samples a side the difference of the two rounded quotients is put back on that lattice, which is
    what scipy's exact mode reports; above it scipy reports the plain difference, and so does this."""
    a, b = np.sort(a), np.sort(b)
    both = np.concatenate([a, b])
    cdf_a = np.searchsorted(a, both, side="right") / a.size
    cdf_b = np.searchsorted(b, both, side="right") / b.size
    d = float(np.max(np.abs(cdf_a - cdf_b)))
    if max(a.size, b.size) <= KS_LATTICE_MAX_N:
        lcm = (a.size // int(np.gcd(a.size, b.size))) * b.size
        d = int(np.round(d * lcm)) * 1.0 / lcm
    return d


def _finite(samples) -> np.ndarray:
    """the finite entries of a sample of any shape, flat"""
    flat = np.ravel(np.asarray(samples, dtype=float))
    return flat[np.isfinite(flat)]


def _p_value(a: np.ndarray, b: np.ndarray) -> float:
    """scipy's p-value of the two-sample test, or NaN (one warning per process) where scipy does not import"""
    global _warned_scipy
    try:
        from scipy.stats import ks_2samp
    except ImportError:
        if not _warned_scipy:
            _warned_scipy = True
            warnings.warn("scipy is not installed: compare_distributions_ks returns NaN p-values", RuntimeWarning)
        return float("nan")
    return float(ks_2samp(a, b).pvalue)


def compare_distributions_ks(sim_samples, real_samples) -> Tuple[float, float]:
    """Two-sample Kolmogorov-Smirnov test: (statistic, p-value).  Inputs are flattened and non-finite values dropped;
    (nan, nan) if either sample is empty after filtering.  The statistic is computed here; the p-value is
    ``scipy.stats.ks_2samp``'s, or NaN (with one warning) where scipy is not installed."""
    pools = (_finite(sim_samples), _finite(real_samples))
    if min(pool.size for pool in pools) == 0:
        return (float("nan"),) * 2
    return _ks_statistic(*pools), _p_value(*pools)


def ks_sample_imbalance(n_sim: int, n_real: int, ratio_warn: float = 2.0) -> Optional[str]:
    """A short warning when a two-sample KS compares pools of very different size (one side empty, or the larger over
    the smaller above ``ratio_warn``), else None.  The texts are the reference's."""
    sizes = f"(n_sim={int(n_sim)}, n_real={int(n_real)})"
    small, large = sorted((int(n_sim), int(n_real)))
    if small == 0:
        return "effective-n WARNING: one side empty " + sizes
    ratio = large / small
    if ratio <= ratio_warn:
        return None
    return f"effective-n imbalance {ratio:.1f}x {sizes}; KS may reflect sample-count, not distribution, difference"


def _pooled_error(records) -> Tuple[float, int]:
    """the encounters' error sums and counts added in encounter order"""
    total, count = 0.0, 0
    for r in records:
        total += float(r["err_sum"])
        count += int(r["err_count"])
    return total, count


def rollout_ade(engine, encounters: Sequence, rollouts: Sequence, interaction_distance: Optional[float] = None) -> float:
    """``objective_rollout_ade`` on supplied roll-outs: the mean distance between simulated and recorded positions over
    every frame but the first and every (kept) pedestrian, pooled over the encounters; inf when nothing is counted."""
    total, count = _pooled_error(fidelity_batch(engine, encounters, rollouts, interaction_distance=interaction_distance)["records"])
    return total / count if count else float("inf")


def _per_encounter_onset(onset_arrays: Sequence[np.ndarray]) -> List[float]:
    """one number per encounter: the median of its finite onset distances, NaN for an encounter without any onset"""
    medians = []
    for onsets in onset_arrays:
        medians.append(float("nan") if np.size(onsets) == 0 else float(np.nanmedian(onsets)))
    return medians


class _Side:
    """what one library call says of one side (simulated or recorded) of a report, pooled as the report wants it"""

    def __init__(self, measured):
        self.records = measured["records"]
        self.closest = [float(v) for v in self.records["closest"]]
        self.per_encounter = [dist[step >= 0] for dist, step in zip(measured["onset_dist"], measured["onset_step"])]
        self.onsets = np.concatenate(self.per_encounter) if self.per_encounter else np.zeros(0)

    def mean_closest(self) -> float:
        return float(np.mean(self.closest)) if self.closest else float("nan")


def fidelity_report(engine, encounters: Sequence, rollouts: Sequence) -> Dict[str, object]:
    """The reference's ``fidelity_report(encounters, sigma, v0)`` on roll-outs the caller simulated: its dictionary, key for
    key (``REPORT_KEYS``).  Two library calls -- the simulated side with the recording as truth, and the recorded side --
    both measured from positions (no recorded velocity on either side, so that the two accelerations are differentiated
    alike)."""
    encounters = list(encounters)
    sides = {"sim": _Side(fidelity_batch(engine, encounters, rollouts)), "real": _Side(fidelity_batch(engine, encounters))}
    err_sum, err_count = _pooled_error(sides["sim"].records)
    values = {"n_encounters": len(encounters), "rollout_ade": err_sum / err_count if err_count else float("nan")}
    values["ks_closest"], values["p_closest"] = compare_distributions_ks(sides["sim"].closest, sides["real"].closest)
    values["ks_onset"], values["p_onset"] = compare_distributions_ks(sides["sim"].onsets, sides["real"].onsets)
    for name, side in sides.items():
        values["mean_closest_" + name] = side.mean_closest()
        values["n_onset_" + name] = int(side.onsets.size)
        values[f"closest_{name}_raw"] = list(side.closest)
        values[f"onset_{name}_raw"] = side.onsets.tolist()
        values[f"onset_per_enc_{name}_raw"] = _per_encounter_onset(side.per_encounter)
    return {key: values[key] for key in REPORT_KEYS}


def _history_arrays(history):
    """(ego_xy [T, 2], per-step pedestrian arrays) of a history of results -- the reference's (``ego_state``,
    ``ped_state.positions``) or this package's step records (``ego``, ``ped_positions``) -- or of a trajectory.npz."""
    if isinstance(history, (str, bytes)) or hasattr(history, "__fspath__"):
        with np.load(history, allow_pickle=True) as d:
            return np.stack([np.asarray(d["ego_x"], float), np.asarray(d["ego_y"], float)], axis=1), list(d["ped_positions"])
    ego, peds = [], []
    for r in history:
        e = r.ego_state if hasattr(r, "ego_state") else r.ego
        ego.append([e.x, e.y])
        peds.append(r.ped_state.positions if hasattr(r, "ped_state") else r.ped_positions)
    return np.array(ego, dtype=float).reshape(-1, 2), peds


def calculate_min_separation(engine, history_or_npz) -> Tuple[np.ndarray, float]:
    """Min-separation series and overall minimum of a history of results, or of a ``trajectory.npz`` that
    ``BatchedClosedLoop.save_results`` wrote.  Requires a fixed pedestrian population across the history.  One whole
    ``fot_fidelity_eval`` call (see ``min_separation_series``)."""
    ego_xy, peds = _history_arrays(history_or_npz)
    rows = [np.asarray(p, dtype=float).reshape(-1, 2) for p in peds]
    if len({r.shape[0] for r in rows}) > 1:
        raise ValueError("calculate_min_separation requires a fixed pedestrian population "
                         "across the history (pedestrian count varies between steps)")
    population = rows[0].shape[0] if rows else 0
    ped_xy = np.concatenate(rows).reshape(len(rows), population, 2) if rows else np.zeros((0, 0, 2))
    series = min_separation_series(engine, ego_xy, ped_xy)
    return series, (float(series.min()) if len(series) else float("inf"))
