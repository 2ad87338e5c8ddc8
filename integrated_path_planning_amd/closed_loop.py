"""Batched closed-loop driver: many simulator episodes in lock-step on one GPU.

One episode is what ``IntegratedSimulator.step()/run()`` (src/simulation/integrated_simulator.py:678-892) does for one
ego vehicle: advance the pedestrians, sample the observer, predict, prepend the current positions, safety metrics,
the escalate-and-retry planning cycle, ego update or emergency stop, termination on collision / goal / timeout.  Here
N episodes that share planner parameters and reference path advance together, and every step issues

* ONE constant-velocity prediction launch over the pedestrians of all running episodes (row f1),
* ONE safety-metrics launch before planning and one after the ego update (row f3),
* ONE ``fot_plan_batch`` with the current configuration of every episode and, only in steps where some first attempt
  fails, ONE more with every further escalation level of the failed episodes (row f2),
* ONE nearest-point launch for the goal test,

instead of N x (1 + up to 3 retries) sequential ``plan()`` calls -- behind ONE library call per lock step
(``fot_loop_step``) on the library's own engine, as five separate calls where the prediction comes through the host (a
sample source, a stand-in engine, ``fused=False``), or with the whole run inside the library (``resident=True``).  The
forms end in one step record and one termination test.  All per-episode state (ego, state machine, planner
caches, pedestrian frame) lives in arrays; the reference's scalar control flow is restated as masked array updates (the
fail-safe transitions themselves once, in state_machine.py), and
the histories are recorded as per-step arrays that turn into ``StepRecord`` objects only when read.  Pedestrians are
replayed tracks -- the contract of the reference's ``ReplayPedestrianSource`` (src/simulation/replay_source.py:31-118);
the Social-Force simulator and the Social-GAN network are outside SURVEY 8.  ``save_results`` writes
``trajectory.npz`` with the reference's keys, dtypes and array shapes (integrated_simulator.py:906-982), so the
existing analysis scripts read it unchanged.

All arithmetic on candidate paths, predictions and metrics runs in libfot.
"""
from __future__ import annotations

import math
import os
import time
from collections import deque
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .batch import PlanRequest
from .data_structures import EgoVehicleState, FrenetPath, PedestrianState
from .footprint import EgoFootprint
from .planner import BatchPlanner
from .prediction import PredictionResampler
from . import _abi
from .state_machine import CONSTANTS, STATES, constants_of, sm_config, sm_update


class ReplayPedestrians:
    """Frame-by-frame replay of [T, N, 2] tracks: step()/get_state() of replay_source.py:31-118."""

    def __init__(self, trajectories, dt: float, velocities=None, goals=None, ids=None):
        traj = np.asarray(trajectories, dtype=float)
        if traj.ndim != 3 or traj.shape[2] != 2:
            raise ValueError(f"trajectories must be [T, N, 2], got shape {traj.shape}")
        self.trajectories = traj
        self.n_frames, self.n_peds, _ = traj.shape
        self.dt = float(dt)
        self.time = 0.0
        self._idx = 0
        if velocities is not None:
            self.velocities = np.asarray(velocities, dtype=float)
        else:                                            # forward difference, last step repeats (:77-84)
            vel = np.zeros_like(traj)
            if traj.shape[0] >= 2:
                vel[:-1] = (traj[1:] - traj[:-1]) / self.dt
                vel[-1] = vel[-2]
            self.velocities = vel
        self.goals = np.asarray(goals, dtype=float) if goals is not None else traj[-1].copy()
        self.ids = np.asarray(ids) if ids is not None else np.arange(self.n_peds)      # (replay_source.py:71-73)

    def step(self, ego_state=None, n: int = 1) -> None:
        """Advance n frames (the position holds at the last frame, the clock keeps running; the ego is ignored:
        replayed pedestrians do not react, replay_source.py:86-99)."""
        for _ in range(n):
            if self._idx < self.n_frames - 1:
                self._idx += 1
            self.time += self.dt

    def reset(self) -> None:
        self._idx, self.time = 0, 0.0

    @property
    def positions(self) -> np.ndarray:
        return self.trajectories[self._idx]

    @property
    def current_velocities(self) -> np.ndarray:
        return self.velocities[self._idx]

    def get_state(self) -> PedestrianState:
        """The current frame as the reference's carrier (replay_source.py:98-106): attribute access, ids included."""
        return PedestrianState(positions=self.positions.copy(), velocities=self.current_velocities.copy(),
                               goals=self.goals.copy(), ids=self.ids.copy(), timestamp=self.time)


class Observer:
    """Sliding window sampled every sgan_dt of pedestrian time (src/pedestrian/observer.py:28-102)."""

    def __init__(self, obs_len: int, dt: float, sgan_dt: float = 0.4):
        self.obs_len, self.dt, self.sgan_dt = obs_len, dt, sgan_dt
        self.history: deque = deque(maxlen=obs_len)
        self.timestamps: deque = deque(maxlen=obs_len)
        self.accumulated_time = 0.0
        self._last_update_timestamp: Optional[float] = None

    def update(self, positions: np.ndarray, timestamp: float) -> None:
        delta_t = self.dt if self._last_update_timestamp is None else max(timestamp - self._last_update_timestamp, 0.0)
        self._last_update_timestamp = timestamp
        self.accumulated_time += delta_t
        if self.accumulated_time + 1e-9 >= self.sgan_dt:
            self.history.append(positions.copy())
            self.timestamps.append(timestamp)
            self.accumulated_time = max(self.accumulated_time - self.sgan_dt, 0.0)

    def reset(self) -> None:
        self.history.clear(); self.timestamps.clear()
        self.accumulated_time = 0.0
        self._last_update_timestamp = None

    @property
    def is_ready(self) -> bool:
        return len(self.history) >= self.obs_len

    @property
    def last_sample_time(self) -> Optional[float]:
        return self.timestamps[-1] if self.timestamps else None


@dataclass
class StepRecord:
    """What SimulationResult holds of one step (data_structures.py:256-281), as plain arrays."""
    time: float
    ego: EgoVehicleState
    ped_positions: np.ndarray
    ped_velocities: np.ndarray
    ped_goals: np.ndarray
    predicted_trajectories: Optional[np.ndarray]
    planned_path: Optional[FrenetPath]
    metrics: Dict[str, Any]
    processing_times: Dict[str, float]


class _VectorStateMachine:
    """``FailSafeStateMachine`` (state_machine.py here, src/core/state_machine.py:29-278 in the reference) for all
    episodes at once: the state of every episode in arrays, moved by ``sm_update`` / ``sm_config``.  Codes 0 / 1 / 2 =
    NORMAL / CAUTION / EMERGENCY."""

    CONSTANTS = CONSTANTS
    constants_of = staticmethod(constants_of)

    def __init__(self, config, n: int, slot_scenario=None):
        """config: one configuration (every constant a scalar), or a sequence of configurations with
        ``slot_scenario[e]`` = the configuration of episode e (every constant an array of n, one entry per episode)."""
        if slot_scenario is None:
            for name, v in constants_of(config).items():
                setattr(self, name, v)
        else:
            per = [constants_of(c) for c in config]
            scen = np.asarray(slot_scenario, np.int64)
            if scen.shape != (n,):
                raise ValueError("slot_scenario: one configuration index per episode")
            for name in CONSTANTS:
                setattr(self, name, np.array([per[k][name] for k in scen], dtype=float))
        self.per_episode = slot_scenario is not None
        self.state = np.zeros(n, np.int64)
        self.fails = np.zeros(n, np.int64)
        self.clear = np.full(n, np.inf)                          # _last_clearance
        self.clear_ahead = np.full(n, np.inf)                    # _last_clearance_ahead

    def _constants(self, who) -> Dict[str, Any]:
        """the constants of the episodes ``who`` (the scalars themselves when there is one configuration)"""
        if not self.per_episode:
            return {name: getattr(self, name) for name in CONSTANTS}
        if who is None:
            raise ValueError("per-episode constants: say which episodes (who=)")
        return {name: getattr(self, name)[who] for name in CONSTANTS}

    def config(self, state: np.ndarray, clear_ahead: np.ndarray, who=None):
        """_get_planner_config (:181-247) -> target speed, overrides [n, 4] (NaN = absent), max_stop (NaN = None).
        who: the episode of every entry (needed when the constants are per episode)."""
        return sm_config(state, clear_ahead, self._constants(who))[:3]

    def update(self, sel: np.ndarray, found: np.ndarray, clearance: np.ndarray, clearance_ahead: np.ndarray,
               speed: np.ndarray) -> None:
        """update() (:116-179) for the episodes ``sel`` (index array): observe the metrics, then the transitions."""
        self.clear[sel], self.clear_ahead[sel] = clearance, clearance_ahead
        self.state[sel], self.fails[sel] = sm_update(self.state[sel], self.fails[sel], found, clearance, speed,
                                                     self._constants(sel))


class EpisodeHistory:
    """One episode's steps as a read-only sequence of ``StepRecord`` built on demand from the loop's per-step arrays
    (every episode takes part in every lock step from the first one until it ends: its step i is lock step i)."""

    def __init__(self, loop: "BatchedClosedLoop", e: int):
        self._loop, self._e = loop, e

    def __len__(self):
        return int(self._loop.step_counts[self._e])

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._loop._record(i, self._e)


_TERMINATION = (None, "collision", "goal", "timeout")


class _ResidentStep(dict):
    """Lock step k of one fot_loop_run call as the dictionary ``_step_native`` writes (same keys and dtypes), filled
    when somebody first reads it: the pedestrian frame and the observer's samples are looked up in the recording by the
    frame indices the library reported."""

    def __init__(self, loop: "BatchedClosedLoop", out: dict, k: int, t: float, keep_paths: bool):
        super().__init__()
        self._src = (loop, out, k, t, keep_paths)
        self.window_frames, self.lock_step = None, -1                # set by a loop whose sampler predicted at this step
        self.best = None                                             # ... and planned on the representative sample

    def _fill(self) -> None:
        if self._src is None:
            return
        loop, o, k, t, keep_paths = self._src
        self._src = None
        sel = np.flatnonzero(o["followed"][k] >= 0)
        n = len(sel)
        counts = (loop.ped_off[sel + 1] - loop.ped_off[sel]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(counts)])
        rows = None if n == len(loop.episodes) else loop._rows_of(sel)

        def frame(which, f):
            a = loop._ped_all[which]
            a = a[min(int(f), len(a) - 1)]
            return a if rows is None else a[rows]

        pred_src = None
        if o["obs_last_frame"][k] >= 0:
            o32 = np.stack([frame("trajectories", o["obs_prev_frame"][k]), frame("trajectories", o["obs_last_frame"][k])],
                           axis=0).astype(np.float32)
            pred_src = (o32, float(o["staleness"][k]))
            if self.window_frames is not None:                        # the loop's sampler predicted (every slot's step
                assert self.window_frames[-1] == int(o["obs_last_frame"][k])    # count is the lock step's index)
                window = np.stack([frame("trajectories", f) for f in self.window_frames], axis=0).astype(np.float32)
                pred_src = ("sgan", window, sel, np.full(n, self.lock_step, np.int64), o32, float(o["staleness"][k]))
                if self.best is not None:                             # the sample the device chose and planned on
                    pred_src = pred_src + (self.best[sel].astype(np.int64),)
                if loop._slot_samples is not None:                    # ... among the episodes' own sample counts
                    pred_src = pred_src + (() if self.best is not None else (np.full(n, -1, np.int64),)) + (loop._slot_samples[sel],)
        if keep_paths:
            paths = {f: o["paths"][k, j][sel] for j, f in enumerate(_abi.PATH_FIELDS)}
        else:
            paths = {f: np.zeros((n, int(o["keep"][k].max()) if n else 0)) for f in _abi.PATH_FIELDS}
        self.update(loop._step_record(
            time=t, sel=sel, off=off, ego=o["ego"][k][sel], jerk=o["jerk"][k][sel],
            state=o["state"][k][sel].astype(np.int64), pos=frame("trajectories", o["frame"][k]),
            vel=frame("velocities", o["frame"][k]), pred=None, pred_src=pred_src, after=o["after"][k][sel],
            stats=o["stats"][k][sel].astype(np.int64), has_path=o["followed"][k][sel] > 0,
            keep=o["keep"][k][sel].astype(np.int64), cost=o["cost"][k][sel], paths=paths, t_pred=0.0,
            t_plan=o["t_plan"]))

    def __missing__(self, key):
        if self._src is None:
            raise KeyError(key)
        self._fill()
        return self[key]

    def get(self, key, default=None):
        self._fill()
        return super().get(key, default)


class Episode:
    """View of one episode of the loop: its history, how many steps it ran and why it ended (None while it runs)."""

    def __init__(self, loop: "BatchedClosedLoop", e: int):
        self._loop, self._e = loop, e
        self.history = EpisodeHistory(loop, e)

    @property
    def step_count(self) -> int:
        return int(self._loop.step_counts[self._e])

    @property
    def termination_reason(self) -> Optional[str]:
        return _TERMINATION[int(self._loop.termination[self._e])]

    @termination_reason.setter
    def termination_reason(self, reason: Optional[str]) -> None:
        self._loop.termination[self._e] = _TERMINATION.index(reason)


def _cfg(config, name, default=None):
    return config.get(name, default) if isinstance(config, dict) else getattr(config, name, default)


class _Cfg:
    """getattr view of a dict (the reference's classes read their configuration with getattr)."""

    def __init__(self, d):
        self.__dict__.update(d)


def expand_static_obstacles(static_obstacles, step: float = 0.5) -> np.ndarray:
    """Rectangles [x_min, x_max, y_min, y_max] -> boundary points every `step` (integrated_simulator.py:805-832)."""
    if static_obstacles is None or len(static_obstacles) == 0:
        return np.empty((0, 2))
    points = []
    for rect in static_obstacles:
        if len(rect) != 4:
            continue
        x_min, x_max, y_min, y_max = rect
        xs = np.arange(x_min, x_max + step, step)
        ys = np.arange(y_min, y_max + step, step)
        for x in xs:
            points.append((x, y_min))
            points.append((x, y_max))
        for y in ys:
            points.append((x_min, y))
            points.append((x_max, y))
    if len(points) == 0:
        return np.empty((0, 2))
    return np.unique(np.array(points), axis=0)


def footprint_from_config(config) -> Optional[EgoFootprint]:
    """src/core/footprint.py footprint_from_config: None = legacy single circle."""
    mode = _cfg(config, "ego_footprint", None)
    if mode is None or mode == "circle":
        return None
    return EgoFootprint.multi_circle(_cfg(config, "vehicle_length"), _cfg(config, "vehicle_width"),
                                     int(_cfg(config, "ego_footprint_n_circles")))


def emergency_stop(x, y, yaw, v, clearance_ahead, dt, max_accel, emergency_decel=None):
    """``IntegratedSimulator._apply_emergency_stop`` (integrated_simulator.py:749-802) for arrays of egos: the position
    integrates along the heading at the OLD speed, the deceleration is what stopping 0.2 m short of the nearest
    pedestrian ahead needs (v^2 / (2 max(clearance - 0.2, 0.05))), bounded to [max_accel, emergency_decel]
    (``None`` = 2 x max_accel); with nothing ahead (non-finite clearance) the cap itself.  Returns the new x, y, v, a
    (a = 0 once the vehicle stands)."""
    x, y, yaw, v = (np.asarray(q, dtype=float) for q in (x, y, yaw, v))
    clr = np.asarray(clearance_ahead, dtype=float)
    cap = max_accel * 2.0 if emergency_decel is None else emergency_decel
    fin = np.isfinite(clr)
    required = np.where(fin, v ** 2 / (2.0 * np.maximum(np.where(fin, clr, 1.0) - 0.2, 0.05)), cap)
    max_dec = np.clip(required, max_accel, cap)
    nv = np.maximum(0.0, v - max_dec * dt)
    na = np.where(nv > 0, -max_dec, 0.0)
    # (the C library's cos / sin element by element -- what math.cos calls and what fot_loop_step's C++ calls: NumPy's
    #  array loops are a SIMD routine of their own that may differ from it in the last place)
    cy = np.array([math.cos(float(t)) for t in np.atleast_1d(yaw)]).reshape(np.shape(yaw))
    sy = np.array([math.sin(float(t)) for t in np.atleast_1d(yaw)]).reshape(np.shape(yaw))
    return x + v * cy * dt, y + v * sy * dt, nv, na


def planner_kwargs_from_config(c, footprint=None) -> dict:
    """The FrenetPlanner arguments a scenario configuration stands for (integrated_simulator.py:342-366)."""
    return dict(
        max_speed=c.ego_max_speed, max_accel=c.ego_max_accel, max_curvature=c.ego_max_curvature,
        max_lat_accel=getattr(c, "ego_max_lat_accel", 3.0), dt=c.dt, d_road_w=c.d_road_w,
        max_road_width=c.max_road_width, robot_radius=getattr(c, "ego_radius", 1.0), obstacle_radius=c.obstacle_radius,
        min_t=getattr(c, "min_t", 4.0), max_t=getattr(c, "max_t", 5.0), d_t_s=getattr(c, "d_t_s", 5.0 / 3.6),
        n_s_sample=getattr(c, "n_s_sample", 1), k_j=c.k_j, k_t=c.k_t, k_d=c.k_d, k_s_dot=c.k_s_dot, k_lat=c.k_lat,
        k_lon=c.k_lon, chance_epsilon=getattr(c, "chance_epsilon", 0.0),
        collision_margin_inflation=getattr(c, "collision_margin_inflation", 1.0), footprint=footprint)


def loop_config_from(c, k: Dict[str, float], max_replan: int) -> "_abi.LoopConfig":
    """fot_loop_config of one configuration; k: ``constants_of(c)``."""
    lc = _abi.LoopConfig()
    lc.dt, lc.target_speed, lc.max_accel = float(c.dt), float(k["target"]), float(c.ego_max_accel)
    dec = getattr(c, "ego_emergency_decel", None)
    lc.emergency_decel = float("nan") if dec is None else float(dec)
    lc.clearance_caution, lc.clearance_emergency = float(k["clr_caution"]), float(k["clr_emergency"])
    lc.trigger_clearance_caution, lc.trigger_time_headway = float(k["trig_c"]), float(k["trig_h"])
    lc.envelope_decel, lc.envelope_standoff = float(k["env_decel"]), float(k["env_standoff"])
    lc.caution_accel, lc.caution_speed, lc.caution_speed_mult = float(k["c_accel"]), float(k["c_speed"]), float(k["c_speed_mult"])
    lc.emergency_accel, lc.emergency_lat_accel = float(k["e_accel"]), float(k["e_lat"])
    lc.max_replan = int(max_replan)
    return lc


# what the episodes of one loop must agree on: one time grid per handle (dt, max_t), and what the frame / the replay
# carries once per loop (observer and predictor lengths, the metrics' radii), the run length and the predictor.
# (distribution_aware_planning is an episode's own: configurations that differ only in it share a scenario and differ in
# the plan mode of their slots, fot_loop_begin_sweep)
COMMON_FIELDS = (("dt", None), ("max_t", 5.0), ("obs_len", None), ("pred_len", None), ("ego_radius", 1.0),
                 ("ped_radius", 0.3), ("total_time", 0.0), ("prediction_method", "sgan"))


def scenario_key(c) -> tuple:
    """What makes two configurations the same scenario of a loop: the planner and loop fields actually used -- the
    planner's arguments, the reference path, the footprint, the static obstacle points and the fail-safe / simulator
    constants.  Fields nothing reads (output_path, visualisation, ...) and the per-episode ones (ego_initial_state) do
    not count."""
    fp = footprint_from_config(c)
    kw = planner_kwargs_from_config(c)
    kw.pop("footprint")
    k = constants_of(c)
    dec = getattr(c, "ego_emergency_decel", None)
    return (tuple(sorted((n, float(v)) for n, v in kw.items())),
            tuple(float(v) for v in c.reference_waypoints_x), tuple(float(v) for v in c.reference_waypoints_y),
            None if fp is None else (tuple(float(o) for o in fp.offsets), float(fp.radius)),
            expand_static_obstacles(getattr(c, "static_obstacles", None), step=0.5).tobytes(),
            tuple(float(k[n]) for n in CONSTANTS), None if dec is None else float(dec))


def merge_configs(configs: Sequence) -> tuple:
    """Per-episode configurations -> (the distinct scenarios in order of first appearance, scenario index per episode).
    Equal configurations (``scenario_key``) share a scenario; a difference in a field the episodes of one loop must
    agree on (``COMMON_FIELDS``) raises ValueError naming the field."""
    cfgs = [c if not isinstance(c, dict) else _Cfg(c) for c in configs]
    if not cfgs:
        raise ValueError("no configuration")
    for name, default in COMMON_FIELDS:
        v0 = getattr(cfgs[0], name, default)
        for i, c in enumerate(cfgs[1:], 1):
            if getattr(c, name, default) != v0:
                raise ValueError(f"the episodes of one loop must agree on {name}: episode 0 has {v0!r}, episode {i} "
                                 f"has {getattr(c, name, default)!r}")
    keys, distinct, slot = {}, [], np.zeros(len(cfgs), np.int32)
    for i, c in enumerate(cfgs):
        key = scenario_key(c)
        if key not in keys:
            keys[key] = len(distinct)
            distinct.append(c)
        slot[i] = keys[key]
    return distinct, slot, cfgs


class BatchedClosedLoop:
    """N episodes of the reference's closed loop in lock-step.

    config: the scenario dictionary (or an object with the same attributes) the reference's SimulationConfig is
    built from -- or a list of them, one per episode: equal ones share a scenario of the one handle, and episodes of
    different scenarios advance in the same lock step (one-call step or ``resident=True``); ped_tracks: one [T, N_i, 2] array of replayed pedestrian positions per episode (frame spacing
    config.dt, frame 0 = time 0 before warm-up); ego_initial_states: optional per-episode [x, y, yaw, v, a].

    The state of all episodes lives in arrays (ego, state machine, planner caches, pedestrian frames); a lock step is a
    fixed sequence of array operations and one libfot call (five where the prediction comes through the host), whatever
    the number of episodes.  Histories are recorded
    as per-step arrays and turned into ``StepRecord`` objects only when somebody reads them.
    """

    MAX_REPLAN = 3                                               # integrated_simulator.py:383
    GOAL_DISTANCE = 2.0                                          # integrated_simulator.py:873-883

    def __init__(self, config, ped_tracks: Sequence[np.ndarray], ego_initial_states: Optional[Sequence] = None,
                 device: int = -1, engine=None, resampler=None, sample_source=None, fused: Optional[bool] = None,
                 device_samples: bool = False, resident: bool = False, summaries: bool = False,
                 prediction_scores: bool = False, plan_on_representative_sample: bool = False, footprint_obs=None,
                 sample_capacity: Optional[int] = None):
        """sample_source: the multi-sample predictor in front of the planner -- a callable
        ``(obs_last [P, 2], obs_prev [P, 2]) -> raw samples [S, pred_len, P, 2]`` at the predictor's own time step
        (a source with the attribute ``needs_history = True``, such as ``prediction.SganSampler``, is called with the
        observer's whole window ``[obs_len, P, 2]`` float32 and the running episodes' pedestrian offsets instead)
        (what S forward passes of Social-GAN on PyTorch-ROCm return for the pedestrians of all running episodes; the
        tests script one).  With it the episodes plan against the whole distribution when the configuration says
        ``distribution_aware_planning`` (integrated_simulator.py:459-460, 514-525), otherwise against the sample closest
        to the mean (``predict_single_best``, trajectory_predictor.py:340-352).  None: the constant-velocity predictor.
        device_samples: the sample source returns a ``torch`` tensor in DEVICE memory ([S, pred_len, sum P, 2], float32 or
        float64) -- Social-GAN's own output on PyTorch-ROCm.  With ``distribution_aware_planning`` the samples then never
        leave the GPU: they are resampled into the planner's tensor inside the lock step's one call (fot_loop_step).
        resident: the whole episode inside the library (fot_loop_set_replay / fot_loop_run): the recording is uploaded to
        HBM once, and ``run(n)`` is a few calls that execute n lock steps each without coming back to Python in between;
        ``step()`` is ``run(1)``.  On the library's own engine, with the constant-velocity predictor -- or with a
        ``prediction.SganSampler`` in counter mode built without an engine (``SganSampler(None, weights, S,
        counter_seed=...)``, ``device_samples=True``, ``distribution_aware_planning``): window, noise, samples and the
        planner's tensor are then formed inside the library every step (fot_loop_set_sampler), nothing crosses the
        bus -- or with a ``prediction.RecordedSamples`` (any predictor's samples of the whole run, recorded once with
        ``prediction.record_samples``; ``device_samples=True``; with ``distribution_aware_planning`` or
        ``plan_on_representative_sample``): the tensor goes to the library once (fot_loop_set_samples; a CUDA tensor is
        used in place) and every step gathers its row there.  ``prediction_scores=True`` works with both.  The loop's arrays
        (``ego``, ``sm.state``, ``alive``, ...) are brought up to date after every call; the Python ``observer`` is not
        advanced (the handle owns the clock).
        summaries (resident loops only): the library accumulates every episode's summary metrics on the device while the
        loop runs -- the reference's ``calculate_aggregate_metrics``; ``aggregate_metrics()`` / ``save_summaries()`` read
        them, a few hundred bytes per episode whatever its length.  ``pred_samples`` reports the configuration's
        ``num_samples`` (trajectory_predictor's sample count, integrated_simulator.py:333: the constant-velocity
        predictor hands the metrics that many identical samples).
        prediction_scores (stepwise loops with a sample_source, and resident loops with their own sampler -- there the
        records are formed and folded inside the library, fot_loop_scores_enable, and ``aggregate_metrics()`` /
        ``save_summaries()`` give the whole summary row): every lock step the library scores the step's sample
        distribution of every running episode against the replayed tracks -- best-of-N ADE / FDE, scene level and per
        agent, and the KDE log-likelihood (``fot_loop_prediction_scores`` on the tensor in HBM with ``device_samples``,
        ``fot_prediction_scores`` on the host distribution otherwise, the "planned on the best sample" mode included);
        ``prediction_metrics()`` folds the records as the reference's ``calculate_aggregate_metrics`` does.  The element
        type of the planner's tensor is the one scored (float64 here; a float32 tensor would give the metrics of the
        rounded samples).
        plan_on_representative_sample: the reference's default (``distribution_aware_planning`` unset) with the samples
        staying in HBM: ``device_samples=True`` is then accepted without ``distribution_aware_planning`` -- the one-call
        step, or ``resident=True`` with a counter-seeded ``SganSampler``.  The library chooses every episode's
        representative sample on the device, lays it out as one fixed-shape [P, n_dense + 1, 2] block (the conditional
        prepend decided there, ``fot_loop_plan_sample``) and plans against it; a step's ``pred`` in the history is the
        sample the device chose.  Not together with ``distribution_aware_planning``.
        A list of configurations together with ``sample_source=..., device_samples=True`` is a SWEEP (fot_loop_begin_sweep):
        every episode on its own scenario and in its own plan mode -- ``distribution_aware_planning`` set: the whole
        distribution; unset: the representative sample (``plan_on_representative_sample=True`` is then required) -- in one
        lock step, on the one-call step or ``resident=True`` (a counter-seeded ``SganSampler`` or a ``RecordedSamples``,
        whose ``slot_col0`` lets the conditions over one crowd share its columns; a ``SganSampler(..., slot_crowd=...)``
        samples every crowd once per lock step for all its conditions, fot_loop_set_sampler_shared; built on several
        ``SganWeights`` with ``slot_model=...`` it gives every slot its own model, fot_loop_set_sampler_models).  A list of one
        distinct scenario and one mode is today's loop.
        A source built with ``slot_samples=[...]`` (``RecordedSamples``, ``SganSampler``) gives slot e the first
        ``slot_samples[e]`` samples of what it provides (fot_loop_set_slot_samples): a sweep as well, also with ONE
        configuration, which then stands for every slot.  ``pred_samples`` of ``prediction_metrics()``,
        ``aggregate_metrics()`` and ``save_summaries()`` is the slot's own count.  The five-call step and stand-in
        engines raise ValueError.
        footprint_obs: True, or a dictionary with any of ``vehicle_length``, ``vehicle_width``, ``n_circles``,
        ``ped_radius`` (the reference's fixed 4.5 / 2.0 / 3 / 0.2 where missing): every lock step also measures the new ego
        state against that step's pedestrians under three geometries that are the same whatever footprint the planner
        used -- the centre, the circle cover and the exact rectangle (fot_loop_footprint_enable; the reference's
        ``observational_footprint_metrics``) -- and ``footprint_metrics()`` returns the episodes' minima and violation
        steps; ``save_summaries()`` appends them.  Resident loops and the one-call step; the five-call step and stand-in
        engines raise ValueError.
        sample_capacity: the most samples of a distribution the loop's engine accepts, 64 (None) to 254: handed to the
        ``BatchPlanner`` the loop builds (``fot_set_sample_capacity``); with a caller's ``engine`` that engine's own
        capacity counts.  A sample source that declares more samples than that (``num_samples``: a ``SganSampler``, a
        ``RecordedSamples``) raises ValueError here, not at the first step.
        fused: True = the lock step behind one library call (fot_loop_step), False = five separate calls with the
        prediction through the host, None = one call where the engine and the predictor allow it."""
        if fused not in (None, False, True):
            raise ValueError("fused: None (automatic), False (five calls per step) or True (one call per step)")
        self._resident = bool(resident)
        self._summaries = bool(summaries)
        if self._summaries and not self._resident:
            raise ValueError("summaries=True needs resident=True (the summary is accumulated by the resident loop)")
        self._pred_scores = bool(prediction_scores)
        # a resident loop's sample source: prediction.SganSampler in counter mode, run inside the library
        # (fot_loop_set_sampler) on the loop's own engine, planning against the whole distribution
        self._resident_sampler = bool(self._resident and sample_source is not None and device_samples
                                      and getattr(sample_source, "counter_seed", None) is not None
                                      and hasattr(sample_source, "bind") and engine is None
                                      and getattr(sample_source, "engine", None) is None)
        # ... or recorded samples (prediction.RecordedSamples): the tensor goes to the library once (fot_loop_set_samples)
        self._resident_recording = bool(self._resident and sample_source is not None and device_samples
                                        and getattr(sample_source, "recorded", False) and engine is None)
        self._resident_dist = self._resident_sampler or self._resident_recording
        if self._pred_scores and self._resident and not self._resident_dist:
            raise ValueError("prediction_scores=True scores the stepwise loop's distributions (resident=False), or those "
                             "of a resident loop's own sampler (a counter-seeded sample_source with device_samples=True)")
        # a resident sampler loop scored inside the library (fot_loop_scores_enable): the summary with it
        self._resident_scores = bool(self._pred_scores and self._resident_dist)
        if self._pred_scores and sample_source is None:
            raise ValueError("prediction_scores=True needs a multi-sample predictor (sample_source)")
        if self._pred_scores and engine is not None and not hasattr(engine, "prediction_scores"):
            raise ValueError("prediction_scores=True needs the library's own engine (fot_prediction_scores)")
        if self._resident and ((sample_source is not None and not self._resident_dist) or engine is not None
                               or resampler is not None or fused not in (None, True)):
            raise ValueError("resident=True needs the constant-velocity predictor on the library's own engine "
                             "(no sample_source, engine or resampler; the one-call step)")
        if self._resident_dist and self._summaries:
            raise ValueError("summaries=True with a sampler: the resident loop's summaries read the constant-velocity "
                             "prediction (not supported yet)")
        # a sequence of configurations, one per episode: equal ones share a scenario of the ONE handle; more than one
        # distinct scenario runs through the one-call step or resident=True only
        self.scenarios, self.slot_scenario, per_episode = None, None, None
        self._sweep, self._slot_aware, any_aware = False, None, False
        # a sample count per slot (the source's slot_samples): a sweep loop whose slot e plans against the first
        # slot_samples[e] samples (fot_loop_set_slot_samples); ONE configuration is then the sweep of it for every slot
        counts = getattr(sample_source, "slot_samples", None)
        self._slot_samples = None if counts is None else np.asarray(counts, dtype=np.int64).reshape(-1)
        if self._slot_samples is not None:
            if len(self._slot_samples) != len(ped_tracks):
                raise ValueError(f"the sample source's slot_samples names {len(self._slot_samples)} slots, the loop has "
                                 f"{len(ped_tracks)} episodes")
            if not (device_samples and engine is None and resampler is None and fused in (None, True)):
                raise ValueError("slot_samples needs device_samples=True and the one-call step (fused=None / True) or "
                                 "resident=True on the library's own engine: the five-call step and stand-in engines plan "
                                 "against one sample count")
            if not isinstance(config, (list, tuple)):
                config = [config] * len(ped_tracks)
        if isinstance(config, (list, tuple)):
            if len(config) != len(ped_tracks):
                raise ValueError(f"{len(config)} configurations for {len(ped_tracks)} episodes: one configuration per episode")
            distinct, slot, per_episode = merge_configs(config)
            aware = np.array([bool(getattr(k, "distribution_aware_planning", False)) for k in per_episode])
            any_aware, mixed = bool(aware.any()), bool(aware.any() and not aware.all())
            # a sweep: more than one scenario and / or mixed plan modes over a sample source whose samples stay in HBM
            self._sweep = bool((len(distinct) > 1 or mixed or self._slot_samples is not None) and sample_source is not None and device_samples
                               and engine is None and resampler is None and fused in (None, True))
            config = distinct[0]
            if self._sweep:
                self.scenarios, self.slot_scenario, self._slot_aware = distinct, slot, aware
            elif len(distinct) > 1 or mixed:
                if engine is not None or resampler is not None or sample_source is not None or fused not in (None, True):
                    raise ValueError("the five-call step, stand-in engines and sample sources take one configuration: "
                                     "episodes of different configurations run through the one-call step "
                                     "(fused=None / True) or resident=True")
                self.scenarios, self.slot_scenario = distinct, slot
        self.config = config if not isinstance(config, dict) else _Cfg(config)
        c = self.config
        self.dt = float(c.dt)
        self.ego_radius = getattr(c, "ego_radius", 1.0)
        self.ped_radius = getattr(c, "ped_radius", 0.3)
        self.footprint = footprint_from_config(c)
        self.sample_source = sample_source
        # the capacity the loop's engine will have: a caller's engine brings its own (a stand-in without one: the keyword)
        cap = getattr(engine, "sample_capacity", None) if engine is not None else None
        if cap is None:
            cap = _abi.MAX_SAMPLES if sample_capacity is None else int(sample_capacity)
            if not _abi.MAX_SAMPLES <= cap <= _abi.MAX_PLAN_SAMPLES:
                raise ValueError(f"sample_capacity: {_abi.MAX_SAMPLES} .. {_abi.MAX_PLAN_SAMPLES}, got {sample_capacity}")
        n_src = getattr(sample_source, "num_samples", None)
        if n_src is not None and int(n_src) > int(cap):
            raise ValueError(f"the sample source has {int(n_src)} samples, the loop's engine accepts {int(cap)}: "
                             + ("raise the engine's own capacity (BatchPlanner(sample_capacity=...))" if engine is not None else
                                f"pass sample_capacity={int(n_src)} (up to {_abi.MAX_PLAN_SAMPLES}) to BatchedClosedLoop"))
        crowd = getattr(sample_source, "slot_crowd", None)            # a sampler whose slots share crowds: one id per episode
        if crowd is not None and len(crowd) != len(ped_tracks):
            raise ValueError(f"the sample source's slot_crowd names {len(crowd)} slots, the loop has {len(ped_tracks)} episodes")
        if getattr(sample_source, "recorded", False):                # a recording: of these tracks, this pred_len?
            sample_source.attach(np.concatenate([[0], np.cumsum([np.shape(tr)[1] for tr in ped_tracks])]),
                                 int(c.pred_len), bool(device_samples))
        if sample_source is None and getattr(c, "prediction_method", "sgan") != "cv":
            raise NotImplementedError("the Social-GAN / LSTM networks are not part of this build (SURVEY 8 f1): hand "
                                      "their samples in through sample_source, or use prediction_method='cv'")
        self.distribution_aware = bool(getattr(c, "distribution_aware_planning", False))
        if self._sweep:                                               # (per slot: _slot_aware; this one says "all of them")
            self.distribution_aware = bool(self._slot_aware.all())
        self._plan_rep = bool(plan_on_representative_sample)
        if self._plan_rep and self.distribution_aware:
            raise ValueError("plan_on_representative_sample plans against ONE sample of the distribution: not together "
                             "with distribution_aware_planning (choose one of the two)")
        if self._plan_rep and not device_samples:
            raise ValueError("plan_on_representative_sample needs device_samples=True (a sample source handing its "
                             "samples over on the host plans on the representative sample already)")
        if (self.distribution_aware or any_aware) and sample_source is None:
            raise ValueError("distribution_aware_planning needs a multi-sample predictor (sample_source): the "
                             "constant-velocity predictor yields one sample")
        self.static_obstacle_points = expand_static_obstacles(getattr(c, "static_obstacles", None), step=0.5)
        # engine / resampler: objects with BatchPlanner's / PredictionResampler's methods; the tests drive the
        # host logic with stand-ins when there is no GPU, the product always builds the libfot handle below
        self._owns_engine = engine is None
        self.engine = engine if engine is not None else BatchPlanner(
            waypoints=(np.asarray(c.reference_waypoints_x, float), np.asarray(c.reference_waypoints_y, float)),
            device=device, sample_capacity=sample_capacity, **planner_kwargs_from_config(c, self.footprint))
        self.s_end = float(self.engine.path_coeffs()[0][-1])
        if self.scenarios is not None:
            # scenario 0 is the first configuration; the other distinct ones join the same handle.  Per episode from here
            # on: the goal (its own path's end), the footprint flag, the static points, the state machine's constants
            self.scenario_footprints = [self.footprint] + [footprint_from_config(k) for k in self.scenarios[1:]]
            for k, fp_k in zip(self.scenarios[1:], self.scenario_footprints[1:]):
                self.engine.add_scenario(
                    waypoints=(np.asarray(k.reference_waypoints_x, float), np.asarray(k.reference_waypoints_y, float)),
                    **planner_kwargs_from_config(k, fp_k))
            s_end = np.array([float(self.engine.path_coeffs(i)[0][-1]) for i in range(len(self.scenarios))])
            self.s_end = s_end[self.slot_scenario]
            self.scenario_static_points = [expand_static_obstacles(getattr(k, "static_obstacles", None), step=0.5)
                                           for k in self.scenarios]
        if sample_source is not None and engine is None and hasattr(sample_source, "bind") and \
                getattr(sample_source, "engine", self.engine) is None:
            sample_source.bind(self.engine)                           # (a sampler built without an engine joins this one)
        if self._resident_dist and not self._sweep and (isinstance(config, (list, tuple)) or self.scenarios is not None):
            raise ValueError("resident=True with a sampler takes one configuration (a scenario loop plans against no "
                             "distribution)")
        self._device_samples = bool(device_samples)
        if self._device_samples and not (sample_source is not None and (self.distribution_aware or self._plan_rep)
                                         and engine is None and resampler is None):   # (a sweep: some slot plans on its sample)
            raise ValueError("device_samples needs a sample_source, distribution_aware_planning and the library's own engine")
        # the whole step behind ONE call (fot_loop_step: the episodes' state, the fail-safe machine and the retry loop live
        # in the handle, the prediction stays in HBM): the constant-velocity predictor -- or samples in device memory -- on
        # the library's own engine.  A sample source hands its samples over on the host and stand-in engines have no
        # device: those run the step of five separate calls, which the tests also hold the one-call step against
        can_fuse = (sample_source is None or self._device_samples) and resampler is None and hasattr(self.engine, "loop_step")
        if fused and not can_fuse:
            raise ValueError("fused=True needs the constant-velocity predictor on the library's own engine")
        self._native = can_fuse if fused is None else bool(fused)
        if self._device_samples and not self._native:
            raise ValueError("device_samples runs through the one-call step only")
        if self.scenarios is not None and not self._native:
            raise ValueError("episodes of different configurations need the one-call step: more than one configuration "
                             "is not supported by this engine")
        self._footprint_obs = None
        if footprint_obs is not None and footprint_obs is not False:
            if not self._native or not hasattr(self.engine, "loop_footprint_enable"):
                if self._owns_engine:
                    self.engine.close()
                raise ValueError("footprint_obs needs the one-call step or resident=True on the library's own engine (the "
                                 "five-call step and stand-in engines do not accumulate it)")
            from .safety import footprint_geometry
            self._footprint_obs = footprint_geometry(None if footprint_obs is True else dict(footprint_obs))
        if self.scenarios is not None:
            for i, pts in enumerate(self.scenario_static_points):
                self.engine.loop_set_scenario_static(i, pts)
        elif self._native:
            self.engine.loop_set_static(self.static_obstacle_points)
        self.sgan_dt = 0.4                                            # integrated_simulator.py:323-327
        self.resampler = resampler if resampler is not None else PredictionResampler(
            self.engine, pred_len=c.pred_len, sgan_dt=self.sgan_dt, sim_dt=c.dt, plan_horizon=getattr(c, "max_t", 5.0))
        n = len(ped_tracks)
        if ego_initial_states is None:
            ego_initial_states = [c.ego_initial_state] * n if per_episode is None else [k.ego_initial_state for k in per_episode]
        # ---- pedestrians: replayed tracks, every episode on the same clock (replay_source.py:31-118)
        self.peds = [ReplayPedestrians(tr, c.dt) for tr in ped_tracks]
        self.n_frames = np.array([p.n_frames for p in self.peds])
        self.ped_off = np.concatenate([[0], np.cumsum([p.n_peds for p in self.peds])]).astype(np.int64)
        # all episodes' tracks side by side, [T_max, sum P, 2] (a shorter replay holds its last frame, as step() does):
        # a frame of every running episode is then one row selection instead of a Python loop over the episodes
        t_max = int(self.n_frames.max()) if len(self.peds) else 0

        def side_by_side(which):
            out = np.zeros((t_max, int(self.ped_off[-1]), 2))
            for e, pd_ in enumerate(self.peds):
                a = getattr(pd_, which)
                out[: pd_.n_frames, self.ped_off[e]:self.ped_off[e + 1]] = a
                out[pd_.n_frames:, self.ped_off[e]:self.ped_off[e + 1]] = a[-1]
            return out
        self._ped_all = {"trajectories": side_by_side("trajectories"), "velocities": side_by_side("velocities")}
        self._rows_key, self._rows = None, None
        self.frame, self.ped_time = 0, 0.0
        self.observer = Observer(c.obs_len, c.dt, self.sgan_dt)      # one sampling clock; samples = all episodes' peds
        self._frame_clock = Observer(c.obs_len, c.dt, self.sgan_dt)  # the same clock on frame numbers (a resident loop's window)
        # ---- ego, state machine and planner caches as arrays
        e0 = np.array([np.asarray(v, float)[:5] for v in ego_initial_states], dtype=float).reshape(n, 5)
        self.ego = e0.copy()                                         # x, y, yaw, v, a
        self.jerk = np.array([float(np.asarray(v, float)[5]) if len(v) > 5 else 0.0 for v in ego_initial_states])
        self.sm = _VectorStateMachine(c, n) if self.scenarios is None else _VectorStateMachine(self.scenarios, n, self.slot_scenario)
        self.prev_s = np.full(n, np.nan)                             # planner.converter._prev_s (NaN: not set yet)
        self.last_kappa = np.zeros(n)                                # planner._last_kappa
        self.goal_prev_s = np.full(n, np.nan)                        # the simulator's own converter (:873)
        self.last_clearance = np.full(n, np.inf)
        self.last_stats = np.full((n, 8), -1, np.int64)              # last_check_stats (-1 row: None)
        self.time = 0.0
        self.alive = np.ones(n, bool)
        self._steps: List[dict] = []
        # Where the selected paths of every step are kept (15 arrays x episodes x samples per step): chunks of whole steps,
        # touched when they are allocated -- fresh pages cost the step that first writes them about as much as the device
        # work of the whole step.  The first chunk covers the configured duration.
        self._arena: List[np.ndarray] = []
        self._arena_steps = 0
        self._arena_slot = len(_abi.PATH_FIELDS) * max(n, 1) * int(getattr(self.engine, "n_total_samples", _abi.MAX_NT))
        if hasattr(self.engine, "gather_paths"):
            self._grow_arena(int(getattr(c, "total_time", 0.0) / self.dt) + 1)
        self.step_counts = np.zeros(n, np.int64)                     # lock steps each episode took part in
        self.termination = np.zeros(n, np.int8)                      # index into _TERMINATION
        self.episodes: List[Episode] = [Episode(self, e) for e in range(n)]
        self._score_dist, self._score_steps = None, []
        if self._pred_scores:
            ratio = self.sgan_dt / self.dt                            # _steps_for_interval (metrics.py:22-28)
            self._score_stride = int(round(ratio))
            if self._score_stride < 1 or not np.isclose(ratio, self._score_stride):
                raise ValueError(f"prediction_scores: the predictor's step {self.sgan_dt} must be a multiple of dt = {self.dt}")
        self._warmup()
        if self._native and self._sweep:
            self.engine.loop_begin_sweep(
                [loop_config_from(k, constants_of(k), self.MAX_REPLAN) for k in self.scenarios],
                [fp_k is not None for fp_k in self.scenario_footprints], self.slot_scenario,
                np.where(self._slot_aware, _abi.LOOP_PLAN_DISTRIBUTION, _abi.LOOP_PLAN_REPRESENTATIVE), self.ego)
            if self._slot_samples is not None and not self._resident:    # (a stepwise sweep: every frame brings the source's count)
                self.engine.loop_set_slot_samples(self._slot_samples)
        elif self._native and self.scenarios is not None:
            self.engine.loop_begin_scenarios(
                [loop_config_from(k, constants_of(k), self.MAX_REPLAN) for k in self.scenarios],
                [fp_k is not None for fp_k in self.scenario_footprints], self.slot_scenario, self.ego)
        elif self._native:
            self.engine.loop_begin(loop_config_from(c, constants_of(c), self.MAX_REPLAN), self.ego)
        if self._footprint_obs is not None:
            self.engine.loop_footprint_enable(self._footprint_obs)
        if self._resident:
            self.engine.loop_set_replay(
                self.ped_off, self.n_frames, self._ped_all["trajectories"], self._ped_all["velocities"],
                obs_len=c.obs_len, pred_len=self.resampler.pred_len, rp=self.resampler.params,
                warmup_frames=int(c.obs_len * self.sgan_dt / c.dt), ego_radius=self.ego_radius, ped_radius=self.ped_radius,
                use_footprint=self.footprint is not None, s_end=float(np.ravel(self.s_end)[0]),
                goal_distance=self.GOAL_DISTANCE)      # (a scenario loop: the library takes each slot's own path's end)
            if self._summaries:
                self.engine.loop_summary_enable(True, int(getattr(c, "num_samples", 1)))
            if self._resident_sampler:
                self.engine.loop_set_sampler(sample_source.num_samples, sample_source.counter_seed, sample_source.noise_kind,
                                             slot_crowd=getattr(sample_source, "slot_crowd", None),
                                             slot_model=getattr(sample_source, "slot_model", None),
                                             model_kinds=getattr(sample_source, "model_kinds", None))
            if self._resident_recording and getattr(sample_source, "slot_col0", None) is not None:
                self.engine.loop_set_samples(sample_source.samples, sample_source.first_step,
                                             n_rec_cols=sample_source.n_cols, slot_col0=sample_source.slot_col0)
            elif self._resident_recording:
                self.engine.loop_set_samples(sample_source.samples, sample_source.first_step)
            if self._slot_samples is not None:                        # (behind the source, whose S bounds the counts)
                self.engine.loop_set_slot_samples(self._slot_samples)
            if self._resident_scores:
                self.engine.loop_scores_enable(True)
        if self._plan_rep and not self._sweep:                        # (a sweep's modes were given per slot at begin)
            self.engine.loop_plan_sample(_abi.LOOP_PLAN_REPRESENTATIVE)

    def close(self) -> None:
        """Release the libfot handle (streams, workspace) now rather than at garbage collection."""
        if self.engine is not None:
            for s in self._steps:                                     # predictions of one-call steps nobody has read yet
                if s["pred"] is None and s.get("pred_src") is not None and not isinstance(s["pred_src"][0], str):
                    s["pred"] = self._materialise_prediction(s["pred_src"], s["off"])
                    s["pred_src"] = None                              # (a distribution's samples: only while somebody asks)
        if self._owns_engine and self.engine is not None:
            self.engine.close()
        self.engine = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------------------------------------------
    ARENA_CHUNK_BYTES = 1 << 28

    def _grow_arena(self, steps: int) -> None:
        steps = max(1, min(int(steps), self.ARENA_CHUNK_BYTES // (8 * self._arena_slot) or 1))
        chunk = np.empty((steps, self._arena_slot))
        chunk.fill(0.0)                                               # (touch the pages now, not inside a step)
        self._arena.append(chunk)
        self._arena_steps += steps

    def _arena_rows(self, k: int, count: int) -> np.ndarray:
        """The arena's rows of lock steps [k, k + count): as many of them as the chunk that holds step k has left."""
        while k >= self._arena_steps:
            self._grow_arena(64)
        for chunk in self._arena:
            if k < len(chunk):
                return chunk[k: k + count]
            k -= len(chunk)

    def _history_block(self, k: int, n: int, kmax: int) -> np.ndarray:
        """[15, n, kmax] block of lock step k in the arena."""
        return self._arena_rows(k, 1)[0, : len(_abi.PATH_FIELDS) * n * kmax].reshape(len(_abi.PATH_FIELDS), n, kmax)

    def _ped_frame(self, which: str, sel: np.ndarray) -> np.ndarray:
        """positions / velocities of the episodes ``sel`` at the current frame, concatenated [sum P, 2]."""
        frame = self._ped_all[which][min(self.frame, len(self._ped_all[which]) - 1)]
        return frame if len(sel) == len(self.peds) else frame[self._rows_of(sel)]

    def _rows_of(self, sel: np.ndarray) -> np.ndarray:
        """Pedestrian rows of the episodes ``sel`` (cached: the set of running episodes changes rarely)."""
        key = sel.tobytes()
        if key != self._rows_key:
            self._rows_key = key
            self._rows = (np.concatenate([np.arange(self.ped_off[e], self.ped_off[e + 1]) for e in sel])
                          if len(sel) else np.zeros(0, np.int64))
        return self._rows

    def _advance_pedestrians(self) -> None:
        self.frame += 1
        self.ped_time += self.dt
        every = np.arange(len(self.peds))
        self.observer.update(self._ped_frame("trajectories", every), self.ped_time)
        self._frame_clock.update(np.array([self.frame]), self.ped_time)

    def _warmup(self) -> None:
        """integrated_simulator.py:406-422: fill the observers before time 0."""
        c = self.config
        for _ in range(int(c.obs_len * self.sgan_dt / c.dt)):
            self._advance_pedestrians()

    @property
    def running(self) -> List[Episode]:
        return [ep for ep, a in zip(self.episodes, self.alive) if a]

    def _metrics(self, sel, off, pos, vel):
        egos = np.stack([self.ego[sel, 0], self.ego[sel, 1], self.ego[sel, 2], self.ego[sel, 3]], axis=1)
        return self.engine.safety_metrics_cat(egos, off, pos, vel, self.ego_radius, self.ped_radius,
                                              use_footprint=self.footprint is not None)

    def _draw_samples(self, obs_last, obs_prev, rows, off):
        """One call of the sample source.  A source with ``needs_history = True`` (``prediction.SganSampler``) is handed the
        observer's whole window for the running episodes' rows, [obs_len, n, 2] float32 as the observer hands it over
        (observer.py:126-135), and their pedestrian offsets; any other source the last two samples, as before."""
        if not getattr(self.sample_source, "needs_history", False):
            return self.sample_source(obs_last, obs_prev)
        window = np.stack([h[rows] for h in self.observer.history], axis=0).astype(np.float32)
        if getattr(self.sample_source, "counter_seed", None) is not None or getattr(self.sample_source, "recorded", False):
            # the counter mode: the noise is keyed by every running episode's slot and its own step count (a recording:
            # its row by the step count, its columns by the slots)
            sel = np.flatnonzero(self.alive)
            return self.sample_source(window, np.asarray(off, dtype=np.int32), slots=sel, steps=self.step_counts[sel])
        return self.sample_source(window, np.asarray(off, dtype=np.int32))

    def _predict(self, sel, off, pos):
        """_update_prediction (:424-527): one launch over the pedestrians of all running episodes.  Returns the
        prediction [sum P, T, 2] (None while the observer fills), per episode whether the current positions are
        prepended (:503-511), and the whole distribution [S, sum P, T, 2] (None unless a sample source predicts)."""
        t0 = time.perf_counter()
        pred, dist = None, None
        if self.observer.is_ready:
            rows = self._rows_of(sel)
            hist = self.observer.history
            obs = np.stack([hist[-2][rows], hist[-1][rows]], axis=0)          # the last two samples
            last = self.observer.last_sample_time
            stale = max(self.ped_time - last, 0.0) if last is not None else 0.0
            if self.sample_source is None:
                pred = self.resampler.predict_cv(obs, staleness=stale, float32_observations=True)
            else:
                # the observer hands over float32 tensors (observer.py:134); the samples are resampled to the
                # simulation step on the device (process_prediction, :233-313), all pedestrians in one launch
                o32 = obs.astype(np.float32).astype(np.float64)
                raw = self._draw_samples(o32[1], o32[0], rows, off)
                raw = np.asarray(raw.detach().cpu().numpy() if hasattr(raw, "detach") else raw, dtype=np.float64)   # [S, pred_len, sum P, 2]
                dist = self.resampler.process_prediction(raw, anchor_pos=o32[1], staleness=stale)
                self._score_dist = dist                               # (what the reference records of the step, :447)
                if raw.shape[0] == 1:
                    pred, dist = dist[0], None
                else:
                    # predict_single_best (:340-352), per episode: the sample closest to the sample mean over the
                    # episode's own pedestrians
                    pred = self._best_sample(dist, off)
        t_pred = (time.perf_counter() - t0) / len(sel)
        if pred is None:
            return None, np.zeros(len(sel), bool), t_pred, None
        # np.allclose(pred[:, 0], current) of the reference (rtol 1e-5, atol 1e-8; finite inputs), per episode
        close = np.all(np.abs(pred[:, 0, :] - pos) <= 1e-8 + 1e-5 * np.abs(pos), axis=1)
        # (counted through a running sum: np.logical_and.reduceat has no empty segment, and an episode without pedestrians
        #  at the END of the frame is an index past the array)
        n_far = np.concatenate([[0], np.cumsum(~close)])
        prepend = n_far[off[1:]] != n_far[off[:-1]]
        empty = off[1:] == off[:-1]
        if empty.any() and not empty.all():                          # no pedestrians: no block either way; agree with the rest
            prepend[empty] = prepend[~empty].all()
        return pred, prepend, t_pred, dist if self.distribution_aware else None

    # ------------------------------------------------------------------------------------------------------
    def step(self) -> int:
        """One lock step of every running episode (integrated_simulator.py:678-747); returns how many ran."""
        if self._resident:
            return self._run_resident(1)
        sel = np.flatnonzero(self.alive)
        if len(sel) == 0:
            return 0
        self._advance_pedestrians()                                   # 1. pedestrians + observer
        off = np.concatenate([[0], np.cumsum(self.ped_off[sel + 1] - self.ped_off[sel])])
        pos = self._ped_frame("trajectories", sel)
        vel = self._ped_frame("velocities", sel)
        form = self._step_native if self._native else self._step_five_calls
        self._score_dist = None
        n = form(sel, off, pos, vel)
        if self._pred_scores:
            self._score_step(sel, off)
        return n

    def _score_step(self, sel, off) -> None:
        """The step's distribution of every episode of ``sel`` scored against the replayed tracks: the truth of origin
        frame f is row min(f + stride j, frames - 1), j = 1 .. pred_len (a shorter recording holds its last frame); the
        records wait in ``_score_steps`` for ``prediction_metrics()``."""
        stride, E = self._score_stride, int(self.resampler.pred_len)
        host = self._score_dist
        ready = host is not None or (self._device_samples and self._steps[-1]["pred_src"] is not None)
        if not ready or stride * E - 1 >= self.resampler.n_dense:     # no prediction yet / no complete horizon (:78)
            return
        tracks = self._ped_all["trajectories"]
        rows = np.minimum(self.frame + stride * np.arange(1, E + 1), len(tracks) - 1)
        truth = np.ascontiguousarray(tracks[rows][:, self._rows_of(sel)].transpose(1, 0, 2))      # [sum P, E, 2]
        if host is None:
            rec = self.engine.loop_prediction_scores(len(sel), stride, E, truth)
        else:
            S_, T = host.shape[0], host.shape[2]
            blocks = [np.ascontiguousarray(host[:, off[i]:off[i + 1]]).reshape(-1, 2) for i in range(len(sel))]
            origins = [(S_ * int(off[i]) * T, S_, int(off[i + 1] - off[i]), T, False, 0) for i in range(len(sel))]
            rec = self.engine.prediction_scores(np.concatenate(blocks) if blocks else np.zeros((0, 2)), origins, truth,
                                                stride, E)
        self._score_steps.append((sel, self.step_counts[sel] - 1, rec))

    def prediction_metrics(self) -> List[Dict[str, Any]]:
        """Per episode the prediction keys of the reference's ``calculate_aggregate_metrics`` over the steps run so far:
        ``ade``, ``fde`` (scene-level best-of-N), ``ade_per_agent``, ``fde_per_agent`` (minADE / minFDE), ``pred_samples``,
        ``ade_eval_count``, ``nll``, ``nll_eval_count`` -- NaN / 0 where nothing counted.  An origin counts once its
        episode has stride * pred_len further steps (metrics.py:78); the records are folded in step order as the
        reference folds them.  Needs ``prediction_scores=True``; may be called between two steps."""
        if not self._pred_scores:
            raise ValueError("prediction_metrics() needs BatchedClosedLoop(..., prediction_scores=True)")
        if self._resident_scores:                                     # folded inside the library, record by record
            keys = ("ade", "fde", "ade_per_agent", "fde_per_agent", "pred_samples", "ade_eval_count", "nll", "nll_eval_count")
            return [{k: (int(r[k]) if k in self.SUMMARY_INT_KEYS else float(r[k])) for k in keys}
                    for r in self.engine.loop_score_summaries()]
        n = len(self.episodes)
        horizon = self._score_stride * int(self.resampler.pred_len)
        tot = np.zeros((n, 5))
        count, nll_count, samples = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for sel, index, rec in self._score_steps:
            for e, i, r in zip(sel, index, rec):
                if r["n_peds"] <= 0 or i + horizon >= self.step_counts[e]:
                    continue
                tot[e, 0] += float(r["ade_scene"]) * int(r["n_peds"])
                tot[e, 1] += float(r["fde_scene"]) * int(r["n_peds"])
                tot[e, 2] += float(r["ade_agent_sum"])
                tot[e, 3] += float(r["fde_agent_sum"])
                count[e] += int(r["n_peds"])
                samples[e] = max(samples[e], int(r["n_samples"]))
                if r["flags"] & _abi.PRED_NLL:
                    tot[e, 4] += float(r["log_lik_sum"])
                    nll_count[e] += int(r["nll_count"])
        nan = float("nan")
        out = []
        for e in range(n):
            c = int(count[e])
            m = [float(v) / c for v in tot[e, :4]] if c else [nan] * 4
            out.append(dict(ade=m[0], fde=m[1], ade_per_agent=m[2], fde_per_agent=m[3], pred_samples=int(samples[e]) if c else 0,
                            ade_eval_count=c, nll=-float(tot[e, 4]) / int(nll_count[e]) if nll_count[e] else nan,
                            nll_eval_count=int(nll_count[e])))
        return out

    def _step_five_calls(self, sel, off, pos, vel):
        """Steps 2-5 in five separate libfot calls, the prediction and the retry loop on the host: what a sample source
        or a stand-in engine runs, and what the tests hold the one-call step against."""
        n = len(sel)
        counts = np.diff(off)
        pred, prepend, t_pred, dist = self._predict(sel, off, pos)    # 2. prediction
        m = self._metrics(sel, off, pos, vel)                         # 3. planning cycle (:529-653)
        t0 = time.perf_counter()
        # --- obstacles: the same static points for every request; one dynamic tensor per episode, shared by its levels
        if pred is None:                                              # not ready: current positions only (:495-498)
            dyn, t_len = pos[:, None, :], np.ones(n, np.int64)
        elif prepend.all():
            dyn, t_len = np.concatenate([pos[:, None, :], pred], axis=1), np.full(n, pred.shape[1] + 1, np.int64)
        elif not prepend.any():
            dyn, t_len = pred, np.full(n, pred.shape[1], np.int64)
        else:                                                         # mixed: the shorter tensors end one sample early
            T1 = pred.shape[1] + 1
            dyn = np.concatenate([pos[:, None, :], pred], axis=1)
            ped_pre = np.repeat(prepend, counts)
            dyn[~ped_pre, :-1] = pred[~ped_pre]
            t_len = np.where(prepend, T1, T1 - 1)
        T_alloc = dyn.shape[1]
        n_smp = np.ones(n, np.int64)
        mode = np.where(counts > 0, 1, 0)
        if dist is not None:
            # the planner consumes the whole distribution (:622-630); the current positions lead EVERY sample,
            # whatever the single sample's prepend decided (:514-525): per episode a [S, P, T + 1, 2] block
            S_ = dist.shape[0]
            full = np.concatenate([np.broadcast_to(pos[None, :, None, :], (S_, len(pos), 1, 2)), dist], axis=2)
            blocks = [np.ascontiguousarray(full[:, off[i]:off[i + 1]]).reshape(-1, 2) for i in range(n)]
            d_xy = np.concatenate(blocks, axis=0) if blocks else np.empty((0, 2))
            t_len = np.full(n, full.shape[2], np.int64)
            d_off_ep = np.concatenate([[0], np.cumsum(S_ * counts * t_len)])[:-1]
            n_smp = np.full(n, S_, np.int64)
            mode = np.where(counts > 0, 2, 0)
        elif t_len.min() != T_alloc:                                  # mixed case: per-episode [P, t_len, 2] blocks
            blocks = [np.ascontiguousarray(dyn[off[i]:off[i + 1], :t_len[i]]).reshape(-1, 2) for i in range(n)]
            d_xy = np.concatenate(blocks, axis=0)
            d_off_ep = np.concatenate([[0], np.cumsum(counts * t_len)])[:-1]
        else:
            d_xy = np.ascontiguousarray(dyn).reshape(-1, 2)
            d_off_ep = off[:-1] * T_alloc
        dynamic = (d_xy, d_off_ep, np.stack([mode, n_smp, counts, t_len], axis=1))
        return self._finish_step(sel, off, pos, vel, pred, t_pred, t0, dynamic, m["clearance"].copy(),
                                 m["clearance_ahead"].copy())

    def _plan_entries(self, sel, who, state, clear_ahead, prev_s, chain, dynamic):
        """One plan() per entry: episode sel[who[i]] under the configuration of ``state[i]``; chain[i]: nearest-point
        cache handed over from the entry before (the next escalation level of the same episode).  dynamic: the step's
        obstacle tensor, every episode's offset into it and its dimensions."""
        tgt, ov, stop = self.sm.config(state, clear_ahead)
        r = len(who)
        ego = np.zeros(r, dtype=self.engine.EGO_DT)
        for col, f in enumerate(("x", "y", "yaw", "v", "a")):
            ego[f] = self.ego[sel, col][who]
        ego["last_kappa"] = self.last_kappa[sel][who]
        ego["has_prev_s"] = np.where(chain, 2, ~np.isnan(prev_s))
        ego["prev_s"] = np.where(chain | np.isnan(prev_s), 0.0, prev_s)
        pts = self.static_obstacle_points
        s_xy = np.tile(pts, (r, 1)) if len(pts) else None
        s_off = np.arange(r + 1, dtype=np.int64) * len(pts) if len(pts) else None
        d_xy, d_off_ep, d_dims = dynamic
        return self.engine.plan_arrays(ego, tgt, ov, stop, s_xy, s_off, d_xy, d_off_ep[who], d_dims[who])

    def _finish_step(self, sel, off, pos, vel, pred, t_pred, t0, dynamic, clearance, clearance_ahead):
        """The rest of the five-call step: the level-0 plans, replay of the retry loop, ego update, result metrics and
        goal test.  dynamic: the obstacles as ``_plan_entries`` takes them; clearance, clearance_ahead: the current
        metrics the fail-safe machine observes."""
        c, sm = self.config, self.sm
        n = len(sel)
        everyone = np.arange(n)
        self.last_clearance[sel] = clearance_ahead
        st0 = sm.state[sel]
        n_lvl = np.minimum(3 - st0, 1 + self.MAX_REPLAN)             # NORMAL -> CAUTION -> EMERGENCY, then no change
        speed = self.ego[sel, 3].copy()
        # --- level 0 of every episode = the current state's configuration (issued from LAST step's clearance)
        rec = self._plan_entries(sel, everyone, st0, sm.clear_ahead[sel], self.prev_s[sel], np.zeros(n, bool), dynamic)
        # --- replay of the retry loop (:576-653).  Episodes whose first attempt failed get every further escalation
        #     level they can reach planned in ONE more launch (the configurations update(False, ...) would issue on THIS
        #     step's metrics, nearest-point cache chained from attempt to attempt); the control flow is then replayed.
        found_all = rec["status"] == 0
        cur = everyone.copy()                                         # record of each episode's current attempt
        path_rec = np.full(n, -1, np.int64)
        failed = np.flatnonzero(~found_all[:n] & (n_lvl > 1))
        if len(failed):
            extra = n_lvl[failed] - 1
            who = np.repeat(failed, extra)
            base1 = np.concatenate([[0], np.cumsum(extra)])[:-1]
            lvl = 1 + np.arange(len(who)) - np.repeat(base1, extra)
            nps0 = rec["new_prev_s"][who]
            rec = np.concatenate([rec, self._plan_entries(sel, who, st0[who] + lvl, clearance_ahead[who],
                                                          np.where(np.isnan(nps0), self.prev_s[sel][who], nps0), lvl > 1,
                                                          dynamic)])
            found_all = rec["status"] == 0
            next_rec = np.full(n, -1, np.int64)                       # record of level 1 of each failed episode
            next_rec[failed] = n + base1
        t_plan = (time.perf_counter() - t0) / n

        def adopt(which, r):                                          # planner state after a plan() call
            nps = rec["new_prev_s"][r]
            e = sel[which]
            self.prev_s[e] = np.where(np.isnan(nps), self.prev_s[e], nps)
            self.last_stats[e] = np.where(rec["stats_valid"][r][:, None] != 0, rec["stats"][r], -1)
            ok = found_all[r]
            self.last_kappa[e[ok]] = rec["new_last_kappa"][r[ok]]
            path_rec[which[ok]] = r[ok]

        adopt(everyone, cur)
        found = found_all[cur]
        issued = st0.copy()                                           # state of the configuration the attempt ran under
        sm.update(sel, found, clearance, clearance_ahead, speed)
        retries = np.zeros(n, np.int64)
        active = ~found & (sm.state[sel] != issued) & (retries < self.MAX_REPLAN) & (retries + 1 < n_lvl)
        while active.any():
            w = np.flatnonzero(active)
            cur[w] = np.where(retries[w] == 0, next_rec[w], cur[w] + 1)
            retries[w] += 1
            adopt(w, cur[w])
            ok = found_all[cur[w]]
            found[w[ok]] = True
            issued[w] = sm.state[sel[w]]
            again = w[~ok]
            if len(again):
                sm.update(sel[again], np.zeros(len(again), bool), clearance[again], clearance_ahead[again], speed[again])
            active = np.zeros(n, bool)
            active[again] = (sm.state[sel[again]] != issued[again]) & (retries[again] < self.MAX_REPLAN) & \
                            (retries[again] + 1 < n_lvl[again])
        # --- 4. ego update (:655-676) or emergency stop (:749-802)
        old_a = self.ego[sel, 4].copy()
        keep = np.where(path_rec >= 0, rec["n_keep"][np.maximum(path_rec, 0)], 0)
        follow = keep >= 2
        new_ego = self.ego[sel].copy()
        jerk = np.zeros(n)
        if follow.any():
            r = path_rec[follow]
            for col, f in enumerate(("x", "y", "yaw", "v", "a")):
                new_ego[follow, col] = rec[f][r, 1]
            jerk[follow] = (new_ego[follow, 4] - old_a[follow]) / self.dt
        brake = ~follow
        if brake.any():
            x, y, yaw, v = (self.ego[sel, k][brake] for k in range(4))
            nx, ny, nv, na = emergency_stop(x, y, yaw, v, self.last_clearance[sel][brake], c.dt, c.ego_max_accel,
                                            getattr(c, "ego_emergency_decel", None))
            new_ego[brake, 0], new_ego[brake, 1] = nx, ny
            new_ego[brake, 3], new_ego[brake, 4] = nv, na
            jerk[brake] = (na - old_a[brake]) / c.dt
            self.last_kappa[sel[brake]] = 0.0                         # planner.reset_ego_curvature()
        self.ego[sel], self.jerk[sel] = new_ego, jerk
        # --- 5. result metrics on the new ego state, goal test (:864-883)
        after = self._metrics(sel, off, pos, vel)
        s_now = self.engine.nearest_s_arrays(new_ego[:, 0], new_ego[:, 1], new_ego[:, 2], new_ego[:, 3], new_ego[:, 4],
                                             self.goal_prev_s[sel])
        self.goal_prev_s[sel] = s_now
        chosen = np.maximum(path_rec, 0)
        kmax = int(keep.max()) if n else 0
        if hasattr(self.engine, "gather_paths"):                      # one dense block, copied by the library
            block = self.engine.gather_paths(rec, chosen, kmax, out=self._history_block(len(self._steps), n, kmax))
            paths = {f: block[j] for j, f in enumerate(_abi.PATH_FIELDS)}
        else:
            paths = {f: rec[f][chosen, :kmax].copy() for f in _abi.PATH_FIELDS}
        return self._close_step(
            s_now, sel=sel, off=off, ego=new_ego, jerk=jerk, state=sm.state[sel].copy(), pos=pos, vel=vel, pred=pred,
            pred_src=None, after=after, stats=self.last_stats[sel].copy(), has_path=path_rec >= 0, keep=keep,
            cost=rec["cost"][chosen], paths=paths, t_pred=t_pred, t_plan=t_plan)

    def _best_sample(self, dist: np.ndarray, off: np.ndarray, counts=None) -> np.ndarray:
        """predict_single_best (trajectory_predictor.py:340-352) per episode: the sample closest to the sample mean over
        the episode's own pedestrians -> [sum P, T, 2].  counts: episode i chooses among its first counts[i] samples."""
        if counts is not None:
            out = np.empty(dist.shape[1:])
            for i, k in enumerate(counts):
                lo, hi = int(off[i]), int(off[i + 1])
                if hi > lo:
                    out[lo:hi] = dist[0, lo:hi] if k == 1 else self._best_sample(np.ascontiguousarray(dist[:int(k), lo:hi]),
                                                                                 np.array([0, hi - lo]))
            return out
        n = len(off) - 1
        dev = np.linalg.norm(dist - dist.mean(axis=0)[None], axis=-1).sum(axis=2)      # [S, sum P]
        # (np.add.reduceat takes no index past the array: episodes without pedestrians at the END of the frame are left out)
        m = int(np.count_nonzero(off[:-1] < dev.shape[1]))
        per_ep = np.zeros((len(dist), n))
        if m:
            per_ep[:, :m] = np.add.reduceat(dev, off[:m], axis=1)
        per_ep[:, off[:-1] == off[1:]] = 0.0                                      # (episodes without pedestrians)
        best = np.argmin(per_ep, axis=0)                                         # [episodes]
        return dist[np.repeat(best, off[1:] - off[:-1]), np.arange(dist.shape[1])]

    def _planned_on(self, best: np.ndarray) -> np.ndarray:
        """[..., slots] chosen samples -> -1 where a sweep's slot planned on the whole distribution (a scored loop chooses
        a sample for those too; the history shows the host's ``predict_single_best`` there, as a uniform loop's does)."""
        return best if not self._sweep else np.where(self._slot_aware, -1, best)

    def _materialise_prediction(self, pred_src, off):
        """The prediction a one-call step left in HBM, computed again for whoever reads the step's record (same kernels,
        same numbers): the constant-velocity tracks, or the best sample of the distribution's raw samples."""
        if isinstance(pred_src[0], str) and pred_src[0] == "sgan":
            # a resident sampler step: the window, the running slots and their step counts -- the library's noise and
            # samples once more, then as a stepwise step's
            _, window, sel, steps, o32, stale = pred_src[:6]
            raw = self.sample_source.sample(window, np.asarray(off, dtype=np.int32), slots=sel, steps=steps)
            pred_src = ("dist", raw, o32, stale) + tuple(pred_src[6:])
        if isinstance(pred_src[0], str):                              # ("dist", raw samples in HBM, observations, staleness)
            _, raw, o32, stale = pred_src[:4]
            raw_h = raw.detach().cpu().numpy().astype(np.float64)
            dist = self.resampler.process_prediction(raw_h, anchor_pos=o32[1].astype(np.float64), staleness=stale)
            if len(pred_src) > 4:                                     # the sample the device chose and planned on, per episode
                off = np.asarray(off)
                chosen = dist[np.repeat(np.maximum(pred_src[4], 0), off[1:] - off[:-1]), np.arange(dist.shape[1])]
                whole = np.repeat(pred_src[4] < 0, off[1:] - off[:-1])     # a sweep's slots that planned on the distribution
                if whole.any() and raw_h.shape[0] > 1:                # (each among its own sample count, where the slots have one)
                    chosen[whole] = self._best_sample(dist, off, pred_src[5] if len(pred_src) > 5 else None)[whole]
                return chosen
            return dist[0] if raw_h.shape[0] == 1 else self._best_sample(dist, np.asarray(off))
        o32, stale = pred_src
        return self.resampler.predict_cv(o32, staleness=stale, float32_observations=True)

    def _loop_frame(self, sel, off, pos, vel):
        """The frame of fot_loop_step for the running episodes: pedestrians, the observer's last two
        samples, per episode whether the current positions lead the prediction (:503-511), staleness."""
        frame = dict(ped_off=off, ped_pos=pos, ped_vel=vel, ego=self.ego[sel, :4], ego_radius=self.ego_radius,
                     ped_radius=self.ped_radius, use_footprint=self.footprint is not None)
        pred_src = None
        if self.observer.is_ready:
            hist = self.observer.history
            if len(sel) == len(self.peds):                            # every episode still runs: the samples as they are
                o32 = np.empty((2,) + hist[-1].shape, np.float32)
                o32[0], o32[1] = hist[-2], hist[-1]
            else:
                rows = self._rows_of(sel)
                o32 = np.stack([hist[-2][rows], hist[-1][rows]], axis=0).astype(np.float32)
            last = self.observer.last_sample_time
            stale = max(self.ped_time - last, 0.0) if last is not None else 0.0
            if self._device_samples:
                prepend = np.ones(len(sel), bool)                     # (the current positions lead EVERY sample, :514-525)
            else:
                # np.allclose(pred[:, 0], current) (:503-511) needs the first predicted sample only: obs_last + v (dt + stale),
                # the velocity formed in float32 as the kernel (and the reference, trajectory_predictor.py:216) forms it
                vel32 = (o32[1] - o32[0]) / np.float32(self.sgan_dt)
                first = o32[1].astype(np.float64) + vel32.astype(np.float64) * ((self.dt + 0.0 * self.dt) + stale)
                far = np.any(np.abs(first - pos) > 1e-8 + 1e-5 * np.abs(pos), axis=1)
                n_far = np.concatenate([[0], np.cumsum(far)])
                prepend = n_far[off[1:]] != n_far[off[:-1]]           # per episode (False without pedestrians)
            frame.update(obs_last=o32[1], obs_prev=o32[0], prepend=prepend, staleness=stale,
                         pred_len=self.resampler.pred_len, rp=self.resampler.params)
            pred_src = (o32, stale)
            if self._device_samples:
                # the multi-sample predictor's raw output stays in HBM: handed to the step as a device pointer
                raw = self._draw_samples(o32[1].astype(np.float64), o32[0].astype(np.float64), self._rows_of(sel), off)
                if not (hasattr(raw, "data_ptr") and raw.is_cuda and raw.is_contiguous() and raw.dim() == 4):
                    raise TypeError("device_samples: the sample source must return a contiguous CUDA tensor [S, pred_len, sum P, 2]")
                import torch
                if raw.dtype not in (torch.float32, torch.float64):
                    raise TypeError("device_samples: float32 or float64 samples")
                torch.cuda.current_stream(raw.device).synchronize()   # (the library reads it on its own stream)
                frame.update(dist_raw=raw.data_ptr(), dist_S=int(raw.shape[0]),
                             dist_dtype=_abi.F32 if raw.dtype == torch.float32 else _abi.F64, _raw=raw)
                pred_src = ("dist", raw, o32, stale)

        return frame, pred_src

    def _step_native(self, sel, off, pos, vel):
        """Steps 2-5 behind ONE libfot call (fot_loop_step): the episodes' state -- ego, planner caches, fail-safe machine
        -- lives in the handle, the retry loop is replayed there; what is left here is the pedestrian frame, the
        observer, the history and the termination test."""
        n = len(sel)
        t0 = time.perf_counter()
        frame, pred_src = self._loop_frame(sel, off, pos, vel)
        frame.pop("ego")
        o = self.engine.loop_step(frame, sel)
        t_plan = (time.perf_counter() - t0) / n
        if self._plan_rep and pred_src is not None and isinstance(pred_src[0], str):
            pred_src = pred_src + (self._planned_on(self.engine.loop_last_best_sample())[sel].astype(np.int64),)   # what the step planned on
        if self._slot_samples is not None and pred_src is not None and isinstance(pred_src[0], str):
            pred_src = pred_src + (() if self._plan_rep else (np.full(n, -1, np.int64),)) + (self._slot_samples[sel],)
        rec, path_rec, keep = o["records"], o["record"].astype(np.int64), o["keep"].astype(np.int64)
        new_ego = o["ego"]
        self.ego[sel], self.jerk[sel] = new_ego, o["jerk"]
        self.sm.state[sel] = o["state"]
        self.last_stats[sel] = o["stats"]
        chosen = np.maximum(path_rec, 0)
        kmax = int(keep.max()) if n else 0
        block = self.engine.gather_paths(rec, chosen, kmax, out=self._history_block(len(self._steps), n, kmax))
        paths = {f: block[j] for j, f in enumerate(_abi.PATH_FIELDS)}
        return self._close_step(
            o["s_now"], sel=sel, off=off, ego=new_ego, jerk=o["jerk"], state=self.sm.state[sel].copy(), pos=pos, vel=vel,
            pred=None, pred_src=pred_src, after=o["after"], stats=self.last_stats[sel].copy(), has_path=path_rec >= 0,
            keep=keep, cost=o["cost"], paths=paths, t_pred=0.0, t_plan=t_plan)

    def _step_record(self, *, time, sel, off, ego, jerk, state, pos, vel, pred, pred_src, after, stats, has_path, keep,
                     cost, paths, t_pred, t_plan) -> dict:
        """What the history keeps of one lock step, one row per episode of ``sel`` (``slot``: episode -> row, -1 = it
        did not run); pos / vel / pred: the pedestrians of those episodes one after the other, episode i at
        off[i]:off[i + 1].  pred_src: what a prediction that stayed in HBM is computed again from when somebody reads it."""
        slot = np.full(len(self.episodes), -1, np.int64)
        slot[sel] = np.arange(len(sel))
        return dict(time=time, slot=slot, off=off, ego=ego, jerk=jerk, state=state, pos=pos, vel=vel, pred=pred,
                    pred_src=pred_src, after=after, stats=stats, has_path=has_path, keep=keep, cost=cost, paths=paths,
                    t_pred=t_pred, t_plan=t_plan, sel=sel)

    def _close_step(self, s_now, *, sel, **arrays) -> int:
        """The end of a lock step, whichever form ran it: its record into the history, then termination
        (integrated_simulator.py:864-883) -- collision first, then the goal within GOAL_DISTANCE of the path's end."""
        self._steps.append(self._step_record(time=self.time, sel=sel, **arrays))
        collided = arrays["after"]["collision"] != 0
        at_goal = (self.s_end if self.scenarios is None else self.s_end[sel]) - s_now < self.GOAL_DISTANCE
        self.step_counts[sel] += 1
        self.termination[sel[at_goal & ~collided]] = 2
        self.termination[sel[collided]] = 1
        self.alive[sel[collided | at_goal]] = False
        self.time += self.dt
        return len(sel)

    def _record(self, k: int, e: int) -> StepRecord:
        """StepRecord of episode e at lock step k, from the step's arrays."""
        s = self._steps[k]
        i = int(s["slot"][e])
        lo, hi = int(s["off"][i]), int(s["off"][i + 1])
        ego = EgoVehicleState(*(float(v) for v in s["ego"][i]), jerk=float(s["jerk"][i]), timestamp=s["time"] + self.dt)
        ego.state = STATES[int(s["state"][i])]
        path = None
        if s["has_path"][i]:
            kn = int(s["keep"][i])
            path = FrenetPath(**{f: s["paths"][f][i, :kn].copy() for f in _abi.PATH_FIELDS})
            path.cost = float(s["cost"][i])
        a = s["after"][i]
        m = {"min_distance": float(a["min_distance"]), "collision": bool(a["collision"]), "ttc": float(a["ttc"]),
             "clearance": float(a["clearance"]), "clearance_ahead": float(a["clearance_ahead"])}
        if s["stats"][i, 0] >= 0:
            m["n_collision_rejected"] = int(s["stats"][i, _abi.ST_COLLISION])
        p = self.peds[e]
        if s["pred"] is None and s.get("pred_src") is not None:       # one-call step: the prediction stayed in HBM
            s["pred"] = self._materialise_prediction(s["pred_src"], s["off"])
            s["pred_src"] = None
        return StepRecord(s["time"], ego, s["pos"][lo:hi].copy(), s["vel"][lo:hi].copy(), p.goals.copy(),
                          None if s["pred"] is None else s["pred"][lo:hi], path, m,
                          {"prediction": s["t_pred"], "planning": s["t_plan"]})

    def _run_resident(self, n_steps: int, keep_paths: bool = True) -> int:
        """n_steps lock steps inside the library (fot_loop_run), in calls whose history block fits the arena's current
        chunk; the loop's arrays follow the handle after every call.  Returns how many episodes ran the first step."""
        first, left = None, int(n_steps)
        while left > 0 and self.alive.any():
            paths_out = self._arena_rows(len(self._steps), left) if keep_paths else None
            ask = len(paths_out) if keep_paths else left
            t0 = time.perf_counter()
            o = self.engine.loop_run(ask, keep_paths=keep_paths, paths_out=paths_out)
            wall = time.perf_counter() - t0
            done = o["n_steps"]
            if done == 0:
                break
            ran = o["followed"] >= 0                                   # [done, slots]
            o["t_plan"] = wall / max(int(ran.sum()), 1)
            if first is None:
                first = int(ran[0].sum())
            # (planning on the representative sample: what every step of the call chose, for the history)
            best = self._planned_on(self.engine.loop_run_best_samples(done)) if self._plan_rep else None
            for k in range(done):
                self._steps.append(_ResidentStep(self, o, k, self.time, keep_paths))
                self.time += self.dt
                self.ped_time += self.dt
                self._frame_clock.update(np.array([self.frame + k + 1]), self.ped_time)
                if self._resident_dist and self._frame_clock.is_ready:
                    self._steps[-1].window_frames = [int(f[0]) for f in self._frame_clock.history]
                    self._steps[-1].lock_step = len(self._steps) - 1
                    if best is not None:
                        self._steps[-1].best = best[k]
            self.frame += done
            took = np.flatnonzero(ran.any(axis=0))
            last = done - 1 - np.argmax(ran[::-1, took], axis=0)      # the last step of the call each slot ran
            self.ego[took], self.jerk[took] = o["ego"][last, took], o["jerk"][last, took]
            self.sm.state[took], self.last_stats[took] = o["state"][last, took], o["stats"][last, took]
            self.step_counts += ran.sum(axis=0)
            code = o["termination"]
            self.termination[code != 0] = code[code != 0]
            self.alive[:] = code == 0
            left -= done
        return first or 0

    def run(self, n_steps: Optional[int] = None, keep_paths: bool = True) -> List[EpisodeHistory]:
        """keep_paths=False (resident loops only): the followed paths are not brought back from the device; a step's
        record then shows zeros in their place."""
        if n_steps is None:
            n_steps = int(self.config.total_time / self.config.dt)
        if self._resident:
            self._run_resident(n_steps, keep_paths)
            n_steps = 0
        elif not keep_paths:
            raise ValueError("keep_paths=False needs resident=True")
        for _ in range(n_steps):
            if self.step() == 0:
                break
        for ep in self.episodes:
            if ep.termination_reason is None:
                ep.termination_reason = "timeout"
        return [ep.history for ep in self.episodes]

    # ------------------------------------------------------------------------------------------------------
    @staticmethod
    def trajectory_arrays(history: List[StepRecord]) -> Dict[str, np.ndarray]:
        """The arrays of trajectory.npz (integrated_simulator.py:906-982): same keys, dtypes and shapes."""
        history = list(history)                                       # (a lazy EpisodeHistory builds its records once)

        def planned(f):
            return np.array([np.array(getattr(r.planned_path, f)) if r.planned_path is not None else np.array([])
                             for r in history], dtype=object)
        return dict(
            times=np.array([r.time for r in history]),
            ego_x=np.array([r.ego.x for r in history]), ego_y=np.array([r.ego.y for r in history]),
            ego_v=np.array([r.ego.v for r in history]), ego_yaw=np.array([r.ego.yaw for r in history]),
            ego_jerk=np.array([r.ego.jerk for r in history]),
            ego_state=np.array([r.ego.state.name for r in history]),
            min_distances=np.array([r.metrics.get("min_distance", float("inf")) for r in history]),
            ttc=np.array([r.metrics.get("ttc", float("inf")) for r in history]),
            proc_prediction=np.array([r.processing_times.get("prediction", 0.0) for r in history]),
            proc_planning=np.array([r.processing_times.get("planning", 0.0) for r in history]),
            ped_positions=np.array([r.ped_positions for r in history], dtype=object),
            ped_velocities=np.array([r.ped_velocities for r in history], dtype=object),
            ped_goals=np.array([r.ped_goals for r in history], dtype=object),
            predicted_trajectories=np.array([r.predicted_trajectories if r.predicted_trajectories is not None
                                             else np.empty((0,)) for r in history], dtype=object),
            planned_x=planned("x"), planned_y=planned("y"), planned_v=planned("v"), planned_a=planned("a"),
            planned_yaw=planned("yaw"),
            planned_cost=np.array([r.planned_path.cost if r.planned_path is not None else float("inf")
                                   for r in history]))

    # the reference's keys in the reference's order (calculate_aggregate_metrics, src/core/metrics.py:300-320)
    SUMMARY_KEYS = ("min_dist", "collision_count", "min_ttc", "max_jerk", "mean_jerk", "rms_jerk", "max_accel", "mean_accel",
                    "ade", "fde", "ade_per_agent", "fde_per_agent", "pred_samples", "ade_eval_count", "planning_ade",
                    "planning_fde", "planning_eval_count", "nll", "nll_eval_count")
    SUMMARY_INT_KEYS = ("collision_count", "pred_samples", "ade_eval_count", "planning_eval_count", "nll_eval_count")

    def aggregate_metrics(self) -> List[Dict[str, Any]]:
        """One dictionary per episode: the keys and value types of the reference's ``calculate_aggregate_metrics`` over the
        steps run so far (ints for the counts, ``inf`` / NaN where the reference has them) plus ``termination_reason``,
        ``steps``, ``total_time`` and ``collision``.  Accumulated on the device by the resident loop (``summaries=True``; a
        resident sampler loop: ``prediction_scores=True``, best-of-N and KDE keys over the whole distributions):
        no step record is read and no prediction recomputed.  May be called between two ``run()`` calls."""
        if not self._resident or not (self._summaries or self._resident_scores):
            raise ValueError("aggregate_metrics() needs BatchedClosedLoop(..., resident=True, summaries=True), or a resident "
                             "sampler loop with prediction_scores=True")
        rec = self.engine.loop_score_summaries() if self._resident_scores else self.engine.loop_summaries()
        out = []
        for e in range(len(self.episodes)):
            r = rec[e]
            d = {k: (int(r[k]) if k in self.SUMMARY_INT_KEYS else float(r[k])) for k in self.SUMMARY_KEYS}
            reason = _TERMINATION[int(r["termination"])] or _TERMINATION[int(self.termination[e])]
            d.update(termination_reason=reason, steps=int(r["steps"]), total_time=float(r["total_time"]),
                     collision=bool(r["collision_count"] > 0))
            out.append(d)
        return out

    def footprint_metrics(self) -> List[Dict[str, Any]]:
        """One dictionary per episode with the keys of the reference's ``observational_footprint_metrics`` over the lock
        steps run so far: ``legacy_min_dist``, ``multi_clearance``, ``multi_violation_steps``, ``rect_clearance``,
        ``rect_violation_steps`` (``inf`` where an episode never met a pedestrian).  Accumulated by the library
        (``footprint_obs=...``); may be called between two ``run()`` calls."""
        if self._footprint_obs is None:
            raise ValueError("footprint_metrics() needs BatchedClosedLoop(..., footprint_obs=True | {...})")
        from .safety import FOOTPRINT_METRIC_KEYS
        rec = self.engine.loop_footprint_obs(len(self.episodes))
        return [{k: (int(r[k]) if k.endswith("_steps") else float(r[k])) for k in FOOTPRINT_METRIC_KEYS} for r in rec]

    def save_summaries(self, output_path: str) -> str:
        """``metrics_summary.csv`` under output_path: one header, one row per episode, the reference's column names (its
        wall-clock columns avg_/max_*_time are left out); with ``footprint_obs`` the five columns of
        ``footprint_metrics()`` follow."""
        import csv
        rows = self.aggregate_metrics()
        os.makedirs(output_path, exist_ok=True)
        f = os.path.join(output_path, "metrics_summary.csv")
        # the reference's row (integrated_simulator.py:1008-1028): context, the metrics, then the collision flag
        cols = (["episode", "prediction_method", "ego_target_speed", "termination_reason", "total_time", "steps"]
                + list(self.SUMMARY_KEYS) + ["collision"])
        if self._footprint_obs is not None:
            from .safety import FOOTPRINT_METRIC_KEYS
            fp_rows = self.footprint_metrics()
            cols += list(FOOTPRINT_METRIC_KEYS)
            rows = [dict(d, **f) for d, f in zip(rows, fp_rows)]
        with open(f, "w", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=cols)
            w.writeheader()
            for i, d in enumerate(rows):
                c = self.config if self.scenarios is None else self.scenarios[int(self.slot_scenario[i])]
                w.writerow(dict(d, episode=i, prediction_method=getattr(c, "prediction_method", "unknown"),
                                ego_target_speed=getattr(c, "ego_target_speed", 0.0)))
        return f

    def save_results(self, output_path: str) -> List[str]:
        """One directory per episode (episode_000, ...), each with the reference's trajectory.npz."""
        files = []
        for i, ep in enumerate(self.episodes):
            d = os.path.join(output_path, f"episode_{i:03d}") if len(self.episodes) > 1 else output_path
            os.makedirs(d, exist_ok=True)
            f = os.path.join(d, "trajectory.npz")
            np.savez(f, **self.trajectory_arrays(ep.history))
            files.append(f)
        return files
