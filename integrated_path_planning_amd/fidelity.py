"""Fidelity statistics of vehicle-pedestrian encounters (RQ2): how close pedestrians come to the vehicle and at what distance
they begin to evade it, simulated against recorded.

The reference's ``min_separation_series``, ``avoidance_onset_distance``, ``compare_distributions_ks``,
``ks_sample_imbalance`` and ``calculate_min_separation`` (src/core/metrics.py) and the measuring half of
``fidelity_report`` / ``objective_rollout_ade`` (src/simulation/calibration_harness.py), with ``engine`` (a
``BatchPlanner``) first.  The Social-Force roll-out is not part of this package: the caller brings the simulated positions
from wherever they were rolled out.  Everything measured on [T, N, 2] arrays -- distances, gradients, the onset search, the
error sums -- runs on the device in ``fot_fidelity_eval``, any number of ragged encounters per call; the pooling, the
medians and the KS test stay on the host, in the reference's order.

The encounters themselves come out of recorded clips (``extract_encounters``: the reference's
src/datasets/vci_encounter.py and the roll-out boundary conditions of calibration_harness.py): the vehicles are aligned
onto the pedestrian grid on the host, and one ``fot_encounters_extract`` call per clip finds the spans, populations and
closest approaches, measures the recorded side and forms cruise speeds and far goals where the clip lies."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .batch import FIDELITY_ENC_DT, PackedEncounters

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


REPORT_ONSET = dict(accel_threshold=0.3, max_distance=5.0)        # the onset parameters a report measures both sides with


def _carried_real(encounters: Sequence):
    """the recorded side as ``extract_encounters`` measured it, in ``fidelity_batch``'s form -- or None unless every
    encounter carries a ``real`` taken with the report's own onset parameters"""
    carried = [_get(e, "real") for e in encounters]
    if not carried or any(r is None or {k: r.get(k) for k in REPORT_ONSET} != REPORT_ONSET for r in carried):
        return None
    records = np.array([r["record"] for r in carried], dtype=FIDELITY_ENC_DT)
    return dict(records=records, onset_dist=[r["onset_dist"] for r in carried], onset_step=[r["onset_step"] for r in carried])


def fidelity_report(engine, encounters: Sequence, rollouts: Sequence) -> Dict[str, object]:
    """The reference's ``fidelity_report(encounters, sigma, v0)`` on roll-outs the caller simulated: its dictionary, key for
    key (``REPORT_KEYS``).  Two library calls -- the simulated side with the recording as truth, and the recorded side --
    both measured from positions (no recorded velocity on either side, so that the two accelerations are differentiated
    alike).  Encounters that ``extract_encounters`` cut with ``measure_real`` carry their recorded side already (the same
    kernels on the same positions): then one call, the simulated side."""
    encounters = list(encounters)
    real = _carried_real(encounters)
    sides = {"sim": _Side(fidelity_batch(engine, encounters, rollouts)),
             "real": _Side(fidelity_batch(engine, encounters) if real is None else real)}
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


# ---- encounters cut out of recorded clips (the reference's src/datasets/vci_encounter.py and the boundary conditions of
# src/simulation/calibration_harness.py): alignment on the host, everything on [T, A, 2] arrays in fot_encounters_extract ------
@dataclass
class RecordedClip:
    """One recorded clip as arrays: the pedestrian grid ``times`` [T] with ``ped_xy`` [T, A, 2] (NaN where a pedestrian is
    absent), ``ped_ids`` [A] and optionally the recorded ``ped_vel`` [T, A, 2]; the vehicles on their own sampling
    ``veh_times`` [Tv] with ``veh_xy`` [Tv, K, 2], ``veh_ids`` [K] and optionally ``veh_psi`` and ``veh_vel`` [Tv, K]."""
    name: str
    times: np.ndarray
    ped_xy: np.ndarray
    ped_ids: np.ndarray
    veh_times: np.ndarray
    veh_xy: np.ndarray
    veh_ids: np.ndarray
    ped_vel: Optional[np.ndarray] = None
    veh_psi: Optional[np.ndarray] = None
    veh_vel: Optional[np.ndarray] = None


@dataclass
class Encounter:
    """A fixed-population interaction window, the reference's fields first.  ``far_goals`` [N, 2] and ``cruise`` [N] are
    the roll-out's boundary conditions where a cruise mode was asked for; ``real`` is the recorded side of a fidelity
    report (``record``, ``onset_dist``, ``onset_step`` and the onset parameters they were measured with)."""
    clip: str
    times: np.ndarray
    ego_xy: np.ndarray
    ego_psi: np.ndarray
    ego_vel: np.ndarray
    ped_xy: np.ndarray
    ped_vel: np.ndarray
    ped_ids: np.ndarray
    dt: float
    min_separation: float
    goals: Optional[np.ndarray] = None
    far_goals: Optional[np.ndarray] = None
    cruise: Optional[np.ndarray] = None
    real: Optional[dict] = None


def _onto_grid(src_t: np.ndarray, src_v: np.ndarray, grid: np.ndarray, angular: bool = False) -> np.ndarray:
    """One channel of one vehicle interpolated onto the grid; NaN outside its support (1e-9 s of slack) and everywhere
    with fewer than two usable samples.  A sample is usable when its time and THIS channel's value are finite, so a gap
    inside the track is bridged.  Headings are unwrapped, interpolated and wrapped again."""
    usable = np.isfinite(src_t) & np.isfinite(src_v)
    out = np.full(grid.shape, np.nan)
    if np.count_nonzero(usable) < 2:
        return out
    t, v = src_t[usable], src_v[usable]
    order = np.argsort(t)                                          # (the reference's call, kind and all: NumPy decides ties)
    t, v = t[order], v[order]
    if angular:
        v = np.unwrap(v)
    inside = (grid >= t[0] - 1e-9) & (grid <= t[-1] + 1e-9)
    values = np.interp(grid[inside], t, v)
    out[inside] = (values + np.pi) % (2 * np.pi) - np.pi if angular else values
    return out


def align_vehicles(clip: RecordedClip) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """Every vehicle of ``clip`` on the pedestrian grid: ``ego_xy`` [K, T, 2], ``ego_psi`` [K, T], ``ego_vel`` [K, T] (NaN
    outside a vehicle's support) and ``dt``.  Without recorded headings or speeds they come from the gradient of the
    interpolated path, which leaves NaN at both ends of a vehicle's support."""
    grid = np.asarray(clip.times, dtype=float)
    dt = float(grid[1] - grid[0]) if len(grid) >= 2 else 0.4
    veh_t = np.asarray(clip.veh_times, dtype=float)
    veh_xy = np.asarray(clip.veh_xy, dtype=float)
    K, T = veh_xy.shape[1], len(grid)
    ego_xy, ego_psi, ego_vel = np.full((K, T, 2), np.nan), np.full((K, T), np.nan), np.full((K, T), np.nan)
    for k in range(K):
        ego_xy[k] = np.stack([_onto_grid(veh_t, veh_xy[:, k, c], grid) for c in (0, 1)], axis=1)
        slope = None
        if clip.veh_psi is None or clip.veh_vel is None:
            slope = np.gradient(ego_xy[k], dt, axis=0) if T >= 2 else np.full((T, 2), np.nan)
        ego_psi[k] = (np.arctan2(slope[:, 1], slope[:, 0]) if clip.veh_psi is None
                      else _onto_grid(veh_t, np.asarray(clip.veh_psi, dtype=float)[:, k], grid, angular=True))
        ego_vel[k] = (np.linalg.norm(slope, axis=1) if clip.veh_vel is None
                      else _onto_grid(veh_t, np.asarray(clip.veh_vel, dtype=float)[:, k], grid))
    return ego_xy, ego_psi, ego_vel, dt


def fallback_velocities(ped_xy: np.ndarray, dt: float) -> np.ndarray:
    """[T, A, 2] forward differences over the whole grid, the last frame repeating the one before; NaN with one frame"""
    vel = np.full_like(ped_xy, np.nan)
    if ped_xy.shape[0] >= 2:
        vel[:-1] = (ped_xy[1:] - ped_xy[:-1]) / dt
        vel[-1] = vel[-2]
    return vel


def _columns(array: np.ndarray, frames: slice, cols: np.ndarray) -> np.ndarray:
    """array[frames][:, cols]: a view where the columns are one run, else a copy"""
    if len(cols) and cols[-1] - cols[0] + 1 == len(cols):
        return array[frames, int(cols[0]):int(cols[-1]) + 1]
    return array[frames][:, cols]


CRUISE_Q = {"quantile": 0.85, "freewalk": 0.5}                    # cruise_upper_quantile's and cruise_freewalk's defaults


def extract_encounters(engine, clips: Sequence[RecordedClip], min_sep_threshold: float = 8.0, min_len: int = 5,
                       multivehicle: bool = True, cruise: Optional[str] = None, measure_real: bool = True,
                       cruise_q: Optional[float] = None, free_distance: float = 8.0, goal_distance: float = 50.0) -> List[Encounter]:
    """The reference's ``encounters_from_clips_multivehicle`` (``multivehicle=False``: ``encounters_from_clips``, which
    skips clips of several vehicles) with ``engine`` first: one ``fot_encounters_extract`` call per clip, its pedestrian
    scene sent once whatever the number of vehicles.  ``cruise`` in (None, 'median', 'quantile', 'freewalk') also fills
    ``Encounter.cruise`` and ``far_goals``; ``measure_real`` fills ``Encounter.real``, which ``fidelity_report`` uses
    instead of a second library call.  A clip of several vehicles names its encounters ``{name}#v{vehicle id}``."""
    q = CRUISE_Q.get(cruise, 0.85) if cruise_q is None else float(cruise_q)
    out: List[Encounter] = []
    for clip in clips:
        K = 0 if clip.veh_xy is None else np.shape(clip.veh_xy)[1]
        if clip.ped_xy is None or K == 0 or (K > 1 and not multivehicle):
            continue
        ego_xy, ego_psi, ego_vel, dt = align_vehicles(clip)
        ped_xy = np.ascontiguousarray(clip.ped_xy, dtype=np.float64)
        given_vel = None if clip.ped_vel is None else np.ascontiguousarray(clip.ped_vel, dtype=np.float64)
        got = engine.encounters_extract(ped_xy, given_vel, ego_xy, ego_psi, ego_vel, dt, min_sep_threshold=min_sep_threshold,
                                        min_len=min_len, cruise=cruise, cruise_q=q, free_distance=free_distance,
                                        goal_distance=goal_distance, measure_real=measure_real, **REPORT_ONSET)
        ped_vel = given_vel
        times, ids = np.asarray(clip.times), np.asarray(clip.ped_ids)
        for s in got["spans"]:
            if s["status"] != _abi.ENC_KEPT:
                continue
            if ped_vel is None:
                ped_vel = fallback_velocities(ped_xy, dt)
            k, frames = int(s["vehicle"]), slice(int(s["frame0"]), int(s["frame1"]))
            rows = slice(int(s["row_base"]), int(s["row_base"]) + int(s["n_ped"]))
            cols = got["cols"][rows]
            real = None
            if measure_real:
                real = dict(record=s["real"].copy(), onset_dist=got["onset_dist"][rows], onset_step=got["onset_step"][rows], **REPORT_ONSET)
            out.append(Encounter(
                clip=f"{clip.name}#v{int(clip.veh_ids[k])}" if K > 1 else clip.name, times=times[frames], ego_xy=ego_xy[k, frames],
                ego_psi=ego_psi[k, frames], ego_vel=ego_vel[k, frames], ped_xy=_columns(ped_xy, frames, cols),
                ped_vel=_columns(ped_vel, frames, cols), ped_ids=ids[cols], dt=dt, min_separation=float(s["min_separation"]),
                far_goals=None if cruise is None else got["goals"][rows], cruise=None if cruise is None else got["cruise"][rows], real=real))
    return out
