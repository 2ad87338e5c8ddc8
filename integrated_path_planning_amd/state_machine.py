"""Fail-safe state machine and the escalate-and-retry planning cycle.

``sm_update`` / ``sm_config`` restate the reference's control logic (src/core/state_machine.py:29-278) over arrays of
episodes: NORMAL / CAUTION / EMERGENCY, the transitions on plan success, failure and clearance, the planner
configuration each state issues.  ``FailSafeStateMachine`` is the reference's class as a view of one episode of them;
the closed-loop driver's vector machine calls them for all episodes at once.  ``SpeculativePlanningCycle`` restates
``IntegratedSimulator._execute_planning_cycle`` (integrated_simulator.py:529-653) the MI355X way: the configurations of every escalation level that the loop
could reach are known before planning (they depend only on the state and on the current safety metrics), so
all of them are planned in ONE launch -- same ego, same obstacles, chained nearest-point cache -- and the
reference's control flow is then replayed on the results.  A failing step costs one launch instead of up to four
sequential ``plan()`` calls.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass
from enum import Enum, auto
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .batch import PlanRequest
from .data_structures import FrenetPath


class VehicleState(Enum):
    NORMAL = auto()
    CAUTION = auto()
    EMERGENCY = auto()


@dataclass
class StateMachineOutput:
    state: VehicleState
    target_speed_override: Optional[float] = None
    constraint_overrides: Optional[Dict[str, float]] = None
    max_stop_distance: Optional[float] = None


STATES = tuple(VehicleState)                                   # array code 0, 1, 2 = NORMAL, CAUTION, EMERGENCY
OVERRIDES = ("max_speed", "max_accel", "max_curvature", "max_lat_accel")      # the columns of sm_config's overrides

# the machine's constants, under the names of fot_loop_config's fields in short
CONSTANTS = ("clr_caution", "clr_emergency", "trig_c", "trig_h", "env_decel", "env_standoff", "target", "c_accel",
             "c_speed_mult", "c_speed", "e_accel", "e_lat")


def constants_of(config) -> Dict[str, float]:
    """The machine's constants as the reference resolves them from one configuration read with getattr
    (state_machine.py:32-98, :181-247)."""
    c = config
    fp_mode = getattr(c, "ego_footprint", None)
    if fp_mode is not None and fp_mode != "circle":
        seg = c.vehicle_length / c.ego_footprint_n_circles                          # footprint.py:37-39
        ego_radius = float(np.hypot(seg / 2, c.vehicle_width / 2))
    else:
        ego_radius = getattr(c, "ego_radius", 1.0)
    combined = ego_radius + getattr(c, "ped_radius", 0.2)
    rc = getattr(c, "state_machine_recover_clearance_caution", None)
    re = getattr(c, "state_machine_recover_clearance_emergency", None)
    k = dict(clr_caution=rc if rc is not None else getattr(c, "state_machine_safe_distance_caution", 2.0) - combined,
             clr_emergency=re if re is not None else getattr(c, "state_machine_safe_distance_emergency", 3.0) - combined,
             trig_c=getattr(c, "state_machine_trigger_clearance_caution", 0.0),
             trig_h=getattr(c, "state_machine_trigger_time_headway", 0.0),
             env_decel=getattr(c, "state_machine_envelope_decel", 0.0),
             env_standoff=getattr(c, "state_machine_envelope_standoff", 0.5), target=float(c.ego_target_speed))
    k["c_accel"] = c.ego_max_accel * getattr(c, "state_machine_caution_accel_multiplier", 1.5)
    k["c_speed_mult"] = getattr(c, "state_machine_caution_speed_multiplier", 0.8)
    k["c_speed"] = c.ego_max_speed * k["c_speed_mult"]
    k["e_accel"] = c.ego_max_accel * getattr(c, "state_machine_emergency_accel_multiplier", 3.0)
    k["e_lat"] = getattr(c, "ego_max_lat_accel", 3.0) * getattr(c, "state_machine_emergency_lat_accel_multiplier", 2.0)
    return k


# The transitions and the planner configurations, once: over arrays with one entry per episode (state codes as in
# STATES; every constant of ``k`` a scalar or an array of the same shape).  They read side by side with sm_update /
# sm_config of csrc/fot_host_loop.cpp, which fot_loop_step and fot_loop_run run.

def sm_update(state, fails, found, clearance, speed, k):
    """The transition of update() (state_machine.py:116-179) -> new state, new count of consecutive failures."""
    trigger = k["trig_c"] + k["trig_h"] * np.maximum(speed, 0.0)
    nm, ca, em = state == 0, state == 1, state == 2
    preventive = found & (trigger > 0.0) & (clearance < trigger)
    recovered = found & (fails == 0) & (clearance > np.maximum(k["clr_caution"], trigger))
    new_state = np.where(nm & (~found | preventive), 1, state)
    new_state = np.where(ca & ~found, 2, np.where(ca & recovered, 0, new_state))
    new_state = np.where(em & found & (clearance > k["clr_emergency"]), 1, new_state)
    return new_state, np.where(em, fails, np.where(found, 0, fails + 1))


def sm_config(state, clear_ahead, k):
    """_get_planner_config (:181-247) on the clearance ahead the machine last observed -> target speed, the overrides
    [..., 4] in the order of OVERRIDES (NaN = absent), the stop room (NaN = None), and whether the target speed is an
    override (False: the configuration's own, which the reference issues as None)."""
    fin = np.isfinite(clear_ahead)
    has_env = fin & (k["env_decel"] > 0.0)
    ahead = np.where(fin, clear_ahead, 0.0)
    v_env = np.sqrt(2.0 * k["env_decel"] * np.maximum(ahead - k["env_standoff"], 0.0))      # _envelope_speed (:249-264)
    stop_room = np.where(fin, np.maximum(ahead - 0.2, 0.05), np.nan)             # _stop_room_to_pedestrian (:266-278)
    nm, ca, em = state == 0, state == 1, state == 2
    slowed = nm & has_env & (v_env < k["target"])
    t_ca = k["target"] * k["c_speed_mult"]
    target = np.where(slowed, v_env, k["target"])
    target = np.where(ca, np.where(has_env, np.minimum(t_ca, v_env), t_ca), target)
    target = np.where(em, 0.0, target)
    stop = np.where(ca & has_env & (v_env <= 0.0), stop_room, np.nan)
    stop = np.where(em & (k["env_decel"] > 0.0), stop_room, stop)
    absent = np.full(np.shape(state), np.nan)
    ov = np.stack([np.where(ca, k["c_speed"], absent), np.where(ca, k["c_accel"], np.where(em, k["e_accel"], absent)),
                   absent, np.where(em, k["e_lat"], absent)], axis=-1)
    return target, ov, stop, slowed | ~nm


class FailSafeStateMachine:
    """Same constructor contract as the reference: a config object read with getattr (state_machine.py:32-98).  One
    episode's view of sm_update / sm_config; its state is plain Python values (``SpeculativePlanningCycle`` runs its dry
    run on a shallow copy)."""

    THRESHOLDS = dict(clearance_caution="clr_caution", clearance_emergency="clr_emergency",
                      trigger_clearance_caution="trig_c", trigger_time_headway="trig_h", envelope_decel="env_decel",
                      envelope_standoff="env_standoff")

    def __init__(self, config) -> None:
        self.config = config
        self.current_state = VehicleState.NORMAL
        self.consecutive_failures = 0
        self._k = constants_of(config)
        for name, key in self.THRESHOLDS.items():
            setattr(self, name, self._k[key])
        self._last_clearance = float("inf")
        self._last_clearance_ahead = float("inf")

    def _constants(self) -> Dict[str, float]:
        """(the thresholds as the attributes hold them now)"""
        return dict(self._k, **{key: getattr(self, name) for name, key in self.THRESHOLDS.items()})

    def observe_metrics(self, safety_metrics: Dict[str, Any]) -> None:                # :99-113
        self._last_clearance = safety_metrics.get("clearance", float("inf"))
        self._last_clearance_ahead = safety_metrics.get("clearance_ahead", self._last_clearance)

    def update(self, plan_found: bool, safety_metrics: Dict[str, Any], ego_speed: float = 0.0) -> StateMachineOutput:
        self.observe_metrics(safety_metrics)
        state, fails = sm_update(np.int64(STATES.index(self.current_state)), np.int64(self.consecutive_failures),
                                 np.bool_(plan_found), np.float64(self._last_clearance), np.float64(ego_speed),
                                 self._constants())
        self.current_state, self.consecutive_failures = STATES[int(state)], int(fails)
        return self._get_planner_config()

    def _get_planner_config(self) -> StateMachineOutput:
        target, ov, stop, overridden = sm_config(np.int64(STATES.index(self.current_state)),
                                                 np.float64(self._last_clearance_ahead), self._constants())
        overrides = {name: float(v) for name, v in zip(OVERRIDES, ov) if not np.isnan(v)}
        return StateMachineOutput(self.current_state, float(target) if overridden else None, overrides or None,
                                  None if np.isnan(stop) else float(stop))


@dataclass
class CycleResult:
    planned_path: Optional[FrenetPath]
    attempts: int                         # plan() calls the reference would have made this step
    retries: int                          # of which escalation retries
    states: List[VehicleState]            # state each attempt was planned in
    final_output: StateMachineOutput      # what the state machine issues after the step


class SpeculativePlanningCycle:
    """One step of _execute_planning_cycle with every reachable escalation level planned in a single launch."""

    def __init__(self, planner, state_machine: FailSafeStateMachine, ego_target_speed: float,
                 max_replan_attempts: int = 3):
        self.planner = planner                    # integrated_path_planning_amd.FrenetPlanner
        self.sm = state_machine
        self.ego_target_speed = ego_target_speed
        self.max_replan_attempts = max_replan_attempts
        self._path_kw = {}                        # BatchedClosedLoop asks for NumPy rows instead of lists

    def _ladder(self, metrics, ego_speed) -> List[StateMachineOutput]:
        """Configurations the retry loop would issue if every attempt failed (dry run on a copy)."""
        sm = copy.copy(self.sm)
        out = [sm._get_planner_config()]
        retries = 0
        cur = out[0]
        nxt = sm.update(False, metrics, ego_speed)
        while nxt.state != cur.state and retries < self.max_replan_attempts:
            out.append(nxt)
            retries += 1
            cur = nxt
            nxt = sm.update(False, metrics, ego_speed)
        return out

    def prepare(self, ego_state, static_obstacles, dynamic_obstacles, current_metrics: Dict[str, Any],
                dynamic_obstacles_distribution=None, replan_attempts_used: int = 0):
        """The requests of every escalation level this step can reach (first = the current state's), and the ladder
        they were built from.  Requests after the first chain their nearest-point cache on the one before."""
        pl = self.planner
        budget = max(self.max_replan_attempts - replan_attempts_used, 0)
        ladder = self._ladder(current_metrics, ego_state.v)[: 1 + budget]
        reqs = []
        for j, cfg in enumerate(ladder):
            target = cfg.target_speed_override if cfg.target_speed_override is not None else self.ego_target_speed
            reqs.append(PlanRequest(
                x=float(ego_state.x), y=float(ego_state.y), yaw=float(ego_state.yaw), v=float(ego_state.v),
                a=float(ego_state.a), target_speed=float(target), last_kappa=float(pl._last_kappa),
                prev_s=None if j else getattr(pl.converter, "_prev_s", None), chain_prev_s=bool(j),
                overrides=cfg.constraint_overrides, max_stop_distance=cfg.max_stop_distance,
                static=static_obstacles, dyn=dynamic_obstacles, dist=dynamic_obstacles_distribution))
        return ladder, reqs, budget

    def finish(self, ladder, budget, res, base: int, ego_state, current_metrics: Dict[str, Any]) -> CycleResult:
        """Replay of integrated_simulator.py:576-653 on the speculative results res.records[base + j]."""
        pl = self.planner

        def adopt(j):
            rec = res.records[base + j]
            if not np.isnan(rec.new_prev_s):
                pl.converter._prev_s = float(rec.new_prev_s)
            pl.last_check_stats = res.stats(base + j)
            path = res.path(base + j, **self._path_kw)
            if path is not None:
                pl._last_kappa = float(rec.new_last_kappa)
            return path

        states = [ladder[0].state]
        path = adopt(0)
        sm_output = ladder[0]
        new_output = self.sm.update(path is not None, current_metrics, ego_speed=ego_state.v)
        retries, j = 0, 0
        while path is None and new_output.state != sm_output.state and retries < budget:
            j += 1
            retries += 1
            states.append(new_output.state)
            path = adopt(j)
            if path is not None:
                break
            sm_output = new_output
            new_output = self.sm.update(False, current_metrics, ego_speed=ego_state.v)
        return CycleResult(path, 1 + retries, retries, states, new_output)

    def execute(self, ego_state, static_obstacles, dynamic_obstacles, current_metrics: Dict[str, Any],
                dynamic_obstacles_distribution=None, replan_attempts_used: int = 0) -> CycleResult:
        ladder, reqs, budget = self.prepare(ego_state, static_obstacles, dynamic_obstacles, current_metrics,
                                            dynamic_obstacles_distribution, replan_attempts_used)
        res = self.planner.engine.plan_batch(reqs)
        return self.finish(ladder, budget, res, 0, ego_state, current_metrics)
