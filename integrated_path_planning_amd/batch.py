"""Packing of independent ego/scenario instances into one ``fot_batch`` (include/fot.h).

One instance = the arguments of one ``FrenetPlanner.plan()`` call of the
reference (frenet_planner.py:227-236).  Obstacle tensors of all instances are
concatenated; shapes travel as host metadata.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi


@dataclass
class PlanRequest:
    """Arguments of one plan() call plus the planner's cross-call state."""
    x: float
    y: float
    yaw: float
    v: float
    a: float
    target_speed: float = 30.0 / 3.6
    last_kappa: float = 0.0
    prev_s: Optional[float] = None
    chain_prev_s: bool = False                   # prev_s := new_prev_s of the previous request (next call on the same planner)
    is_frenet: bool = False                      # x, y, yaw, v, a, last_kappa hold s, s_d, s_dd, d, d_d, d_dd (FOT_EGO_IS_FRENET)
    overrides: Optional[dict] = None
    max_stop_distance: Optional[float] = None
    static: Optional[np.ndarray] = None          # [Ns, 2]
    dyn: Optional[np.ndarray] = None             # [P, T, 2]
    dist: Optional[np.ndarray] = None            # [S, P, T, 2]
    scenario: int = 0                            # planner configuration + reference path (BatchPlanner.add_scenario)


def _dyn_of(req: PlanRequest):
    """Which dynamic tensor plan() would use (frenet_planner.py:1043-1047, 1205-1208).  Passed on as it is: the
    reference's rule for NaN coordinates (a pedestrian whose track holds one is ignored at every time step,
    frenet_planner.py:1211-1219) is applied by the library itself, for every producer of the tensor."""
    if req.dist is not None and np.size(req.dist) > 0:
        d = np.asarray(req.dist)
        if d.ndim != 4 or d.shape[-1] != 2:
            raise ValueError(f"distribution must be [S, P, T, 2], got {d.shape}")
        return _abi.DYN_DISTRIBUTION, d
    if req.dyn is not None and np.size(req.dyn) > 0 and np.shape(req.dyn)[-1] == 2:
        d = np.asarray(req.dyn)
        if d.ndim != 3:
            raise ValueError(f"dynamic obstacles must be [P, T, 2], got {d.shape}")
        return _abi.DYN_SINGLE, d[None]
    return _abi.DYN_NONE, None


class PackedBatch:
    """Host-side ``fot_batch`` with the NumPy buffers that back its pointers."""

    def __init__(self, requests: Sequence[PlanRequest], obstacle_dtype=np.float64, dyn_layout_tsp: bool = False):
        """dyn_layout_tsp: pack every dynamic tensor time-major, [T][S][P][2] (``FOT_DYN_LAYOUT_TSP``) -- the layout the
        broad phase reads with fully coalesced loads and the device-side resampler can write directly."""
        n = len(requests)
        self.dyn_layout_tsp = bool(dyn_layout_tsp)
        self.n = n
        self.np_dtype = np.dtype(obstacle_dtype)
        if self.np_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("obstacle_dtype must be float32 or float64")
        self.ego = (_abi.Ego * max(n, 1))()
        self.target = np.zeros(max(n, 1), dtype=np.float64)
        self.overrides = (_abi.Overrides * max(n, 1))()
        self.max_stop = np.full(max(n, 1), np.nan, dtype=np.float64)
        self.static_off = np.zeros(n + 1, dtype=np.int32)
        self.dyn_off = np.zeros(max(n, 1), dtype=np.int64)
        self.dyn_dims = np.zeros((max(n, 1), 4), dtype=np.int32)
        self.scenario = np.zeros(max(n, 1), dtype=np.int32)     # fot_plan_batch_scenarios' scenario[n_inst]
        statics: List[np.ndarray] = []
        dyns: List[np.ndarray] = []
        dyn_cursor = 0
        nan = float("nan")
        shared = {}                                  # (id(array), mode) -> offset: requests passing the SAME dynamic tensor
                                                     # object (escalation retries of one step) share one copy of it
        for i, r in enumerate(requests):
            e = self.ego[i]
            e.x, e.y, e.yaw, e.v, e.a = float(r.x), float(r.y), float(r.yaw), float(r.v), float(r.a)
            e.last_kappa = float(r.last_kappa)
            if r.is_frenet:
                e.has_prev_s, e.prev_s = _abi.EGO_IS_FRENET, 0.0
            elif r.chain_prev_s:
                if i == 0:
                    raise ValueError("the first request of a batch cannot chain its nearest-point cache")
                e.has_prev_s, e.prev_s = 2, 0.0
            else:
                e.has_prev_s = 0 if r.prev_s is None else 1
                e.prev_s = 0.0 if r.prev_s is None else float(r.prev_s)
            self.target[i] = float(r.target_speed)
            self.scenario[i] = int(r.scenario)
            ov = r.overrides or {}
            o = self.overrides[i]
            o.max_speed = float(ov.get("max_speed", nan))
            o.max_accel = float(ov.get("max_accel", nan))
            o.max_curvature = float(ov.get("max_curvature", nan))
            o.max_lat_accel = float(ov.get("max_lat_accel", nan))
            if r.max_stop_distance is not None:
                self.max_stop[i] = float(r.max_stop_distance)
            st = np.empty((0, 2)) if r.static is None or len(r.static) == 0 else np.asarray(r.static).reshape(-1, 2)
            statics.append(st.astype(self.np_dtype, copy=False))
            self.static_off[i + 1] = self.static_off[i] + st.shape[0]
            mode, d = _dyn_of(r)
            self.dyn_off[i] = dyn_cursor
            if mode != _abi.DYN_NONE:
                S, P, T = d.shape[0], d.shape[1], d.shape[2]
                self.dyn_dims[i] = (mode | (_abi.DYN_LAYOUT_TSP if self.dyn_layout_tsp else 0), S, P, T)
                src = r.dist if mode == _abi.DYN_DISTRIBUTION else r.dyn
                key = (id(src), mode)
                if key in shared:
                    self.dyn_off[i] = shared[key]
                else:
                    shared[key] = dyn_cursor
                    if self.dyn_layout_tsp:
                        d = np.transpose(d, (2, 0, 1, 3))                  # [S, P, T, 2] -> [T, S, P, 2]
                    dyns.append(np.ascontiguousarray(d, dtype=self.np_dtype).reshape(-1, 2))
                    dyn_cursor += S * P * T
        self.static_xy = (np.concatenate(statics, axis=0) if statics else np.empty((0, 2))).astype(self.np_dtype)
        self.static_xy = np.ascontiguousarray(self.static_xy)
        self.dyn_xy = np.ascontiguousarray(np.concatenate(dyns, axis=0) if dyns else np.empty((0, 2), self.np_dtype))
        self.mixed = bool(n and np.any(self.scenario[:n] != 0))   # some instance is not on scenario 0
        self.n_candidates_hint = None
        self.c = self._make_struct(self.static_xy.ctypes.data if self.static_xy.size else None,
                                   self.dyn_xy.ctypes.data if self.dyn_xy.size else None)

    def _make_struct(self, static_ptr, dyn_ptr) -> _abi.Batch:
        b = _abi.Batch()
        b.n_inst = self.n
        b.obstacle_dtype = _abi.F32 if self.np_dtype == np.dtype(np.float32) else _abi.F64
        b.ego = C.cast(self.ego, C.POINTER(_abi.Ego))
        b.target_speed = self.target.ctypes.data_as(C.POINTER(C.c_double))
        b.overrides = C.cast(self.overrides, C.POINTER(_abi.Overrides))
        b.max_stop_distance = self.max_stop.ctypes.data_as(C.POINTER(C.c_double))
        b.static_xy = static_ptr
        b.static_off = self.static_off.ctypes.data_as(C.POINTER(C.c_int32)) if static_ptr else None
        b.dyn_xy = dyn_ptr
        b.dyn_off = self.dyn_off.ctypes.data_as(C.POINTER(C.c_int64)) if dyn_ptr else None
        b.dyn_dims = self.dyn_dims.ctypes.data_as(C.POINTER(C.c_int32)) if dyn_ptr else None
        return b

    def scenario_ptr(self):
        """The ``scenario`` argument of ``fot_plan_batch_scenarios[_device]``: NULL when every instance is on scenario 0."""
        return self.scenario.ctypes.data_as(C.POINTER(C.c_int32)) if self.mixed else None

    def with_device_obstacles(self, static_dev_ptr: Optional[int], dyn_dev_ptr: Optional[int]) -> _abi.Batch:
        """Same batch with the obstacle coordinates already resident in HBM."""
        return self._make_struct(static_dev_ptr if self.static_xy.size else None,
                                 dyn_dev_ptr if self.dyn_xy.size else None)


FIDELITY_ENC_DT = np.dtype(_abi.FidelityEnc)


class PackedEncounters:
    """Ragged encounters as ``fot_fidelity_eval`` takes them: the step offsets, the pedestrian counts and the time steps,
    the ego rows [steps, 2] and every encounter's [T, N, 2] arrays back to back."""

    def __init__(self, ego_xy: Sequence, ped_xy: Sequence, dt: Sequence[float], ped_vel: Optional[Sequence] = None,
                 truth_xy: Optional[Sequence] = None):
        egos = [np.asarray(e, dtype=np.float64) for e in ego_xy]
        peds = [np.asarray(p, dtype=np.float64) for p in ped_xy]
        for e, p in zip(egos, peds):
            if p.ndim != 3 or p.shape[2] != 2 or e.ndim != 2 or e.shape[1] != 2:
                raise ValueError(f"an encounter is ego_xy [T, 2] and ped_xy [T, N, 2], got {e.shape} and {p.shape}")
            if e.shape[0] != p.shape[0]:
                raise ValueError(f"ego_xy T={e.shape[0]} != ped_xy T={p.shape[0]}")
        self.n = len(peds)
        if len(egos) != self.n or len(dt) != self.n:
            raise ValueError("one ego_xy, ped_xy and dt per encounter")
        self.steps = np.array([p.shape[0] for p in peds], dtype=np.int64)
        self.n_ped = np.array([p.shape[1] for p in peds], dtype=np.int32)
        if self.steps.sum() > np.iinfo(np.int32).max:
            raise ValueError("more steps than int32 offsets hold")
        self.step_off = np.concatenate([[0], np.cumsum(self.steps)]).astype(np.int32)
        self.ped_base = np.concatenate([[0], np.cumsum(self.n_ped, dtype=np.int64)])
        self.dt = np.asarray(dt, dtype=np.float64).reshape(self.n)
        self.ego = self._flat(egos)
        self.ped = self._flat(peds)
        self.vel = self._same_shape(ped_vel, peds, "ped_vel")
        self.truth = self._same_shape(truth_xy, peds, "truth_xy")

    @staticmethod
    def _flat(arrays) -> np.ndarray:
        flat = [a.reshape(-1) for a in arrays]
        out = np.concatenate(flat) if flat else np.zeros(0)
        return np.ascontiguousarray(out if out.size else np.zeros(2))     # (never a NULL pointer: an empty set is not refused)

    def _same_shape(self, arrays, peds, name):
        if arrays is None:
            return None
        arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
        if len(arrays) != self.n:
            raise ValueError(f"one {name} per encounter")
        for a, p in zip(arrays, peds):
            if a.shape != p.shape:
                raise ValueError(f"{name} shape {a.shape} != ped_xy shape {p.shape}")
        return self._flat(arrays)


def fidelity_eval(lib, handle, enc: PackedEncounters, accel_threshold: float = 0.3, max_distance: float = 5.0,
                  interaction_distance: Optional[float] = None):
    """``fot_fidelity_eval`` on packed encounters, one call.  Returns ``(records, series, onset_dist, onset_step)``:
    ``FIDELITY_ENC_DT`` per encounter, the separation per step, and per pedestrian the onset distance (NaN: none) and
    step (-1: none)."""
    p = _abi.FidelityParams(float(accel_threshold), float(max_distance),
                            float("nan") if interaction_distance is None else float(interaction_distance))
    n, steps, peds = enc.n, int(enc.step_off[-1]), int(enc.ped_base[-1])
    out = np.zeros(max(n, 1), dtype=FIDELITY_ENC_DT)
    series = np.zeros(max(steps, 1))
    dist = np.full(max(peds, 1), np.nan)
    step = np.full(max(peds, 1), -1, dtype=np.int32)
    addr = lambda a: None if a is None else a.ctypes.data
    n_ped, dt = (enc.n_ped, enc.dt) if n else (np.zeros(1, np.int32), np.ones(1))
    _abi.check(handle, lib.fot_fidelity_eval(handle, C.byref(p), n, addr(enc.step_off), addr(n_ped), addr(dt), addr(enc.ego),
                                             addr(enc.ped), addr(enc.vel), addr(enc.truth), addr(series), addr(dist),
                                             addr(step), addr(out)))
    return out[:n], series[:steps], dist[:peds], step[:peds]


ENCOUNTER_SPAN_DT = np.dtype(_abi.EncounterSpan)


def encounter_span_counts(ego_xy: np.ndarray, ego_psi: np.ndarray, ego_vel: np.ndarray, min_len: int) -> Tuple[int, int]:
    """(candidate spans, those of at least ``min_len`` frames) of aligned ego channels [K, T(, 2)]: the capacities an
    ``encounters_extract`` call needs, counted as the library finds its spans (maximal runs with all four channels finite)."""
    here = np.isfinite(ego_xy).all(axis=2) & np.isfinite(ego_psi) & np.isfinite(ego_vel)             # [K, T]
    edge = np.diff(np.pad(here.astype(np.int8), ((0, 0), (1, 1))), axis=1)
    starts, stops = np.nonzero(edge == 1), np.nonzero(edge == -1)           # row-major: a row's starts and stops pair up
    return int(starts[0].size), int(np.count_nonzero(stops[1] - starts[1] >= int(min_len)))


def encounters_extract(lib, handle, ped_xy, ped_vel, ego_xy, ego_psi, ego_vel, dt: float, min_sep_threshold: float = 8.0,
                       min_len: int = 5, accel_threshold: float = 0.3, max_distance: float = 5.0, cruise: Optional[str] = None,
                       cruise_q: float = 0.85, free_distance: float = 8.0, goal_distance: float = 50.0, measure_real: bool = True,
                       want_series: bool = False, max_spans: Optional[int] = None, max_rows: Optional[int] = None) -> dict:
    """``fot_encounters_extract`` on one clip: ``ped_xy`` [T, A, 2] (``ped_vel`` alike, or None: the forward-difference
    fallback), host arrays or device tensors of float64, and the aligned ego channels ``ego_xy`` [K, T, 2], ``ego_psi``
    and ``ego_vel`` [K, T].  Returns a dictionary: ``spans`` (``ENCOUNTER_SPAN_DT`` per candidate span), and per row (the
    kept spans' pedestrians back to back) ``cols``, ``cruise`` and ``goals`` (None without a cruise mode), ``onset_dist``
    and ``onset_step`` (None without ``measure_real``); ``series`` with ``want_series``.  The capacities default to what
    the ego channels' runs can need at most."""
    if cruise not in _abi.ENC_CRUISE:
        raise ValueError(f"cruise is one of {sorted(k for k in _abi.ENC_CRUISE if k)} or None, got {cruise!r}")
    ego_xy = np.ascontiguousarray(ego_xy, dtype=np.float64)
    ego_psi, ego_vel = (np.ascontiguousarray(a, dtype=np.float64) for a in (ego_psi, ego_vel))
    if ego_xy.ndim != 3 or ego_xy.shape[2] != 2 or ego_psi.shape != ego_xy.shape[:2] or ego_vel.shape != ego_xy.shape[:2]:
        raise ValueError(f"ego_xy [K, T, 2], ego_psi and ego_vel [K, T], got {ego_xy.shape}, {ego_psi.shape}, {ego_vel.shape}")
    K, T = ego_xy.shape[:2]
    on_device = hasattr(ped_xy, "data_ptr")
    keep = []

    def scene(a, name):
        if a is None:
            return None
        if on_device != hasattr(a, "data_ptr"):
            raise ValueError("ped_xy and ped_vel lie both on the host or both on the device")
        if on_device:
            if str(a.dtype).rsplit(".", 1)[-1] != "float64" or not a.is_contiguous():
                raise ValueError(f"a device {name} is a contiguous float64 tensor")
        else:
            a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 3 or a.shape[0] != T or a.shape[2] != 2:
            raise ValueError(f"{name} is [T={T}, A, 2], got {tuple(a.shape)}")
        keep.append(a)
        return a

    xy, vel = scene(ped_xy, "ped_xy"), scene(ped_vel, "ped_vel")
    if vel is not None and tuple(vel.shape) != tuple(xy.shape):
        raise ValueError(f"ped_vel shape {tuple(vel.shape)} != ped_xy shape {tuple(xy.shape)}")
    A = int(xy.shape[1])
    ptr = (lambda a: None if a is None else a.data_ptr()) if on_device else (lambda a: None if a is None else a.ctypes.data)
    mode = _abi.ENC_CRUISE[cruise]
    flags = (_abi.ENC_SCENE_DEVICE if on_device else 0) | (_abi.ENC_MEASURE_REAL if measure_real else 0)
    p = _abi.EncounterParams(float(min_sep_threshold), float(dt), float(accel_threshold), float(max_distance), float(cruise_q),
                             float(free_distance), float(goal_distance), int(min_len), mode, flags, 0)
    if max_spans is None or max_rows is None:
        n_all, n_long = encounter_span_counts(ego_xy, ego_psi, ego_vel, min_len) if K and T else (0, 0)
        max_spans = n_all if max_spans is None else max_spans
        max_rows = n_long * A if max_rows is None else max_rows
    max_spans, max_rows = int(max_spans), int(max_rows)
    series_on = bool(want_series and measure_real)
    max_steps = max_spans * T if series_on else 0
    spans = np.zeros(max(max_spans, 1), dtype=ENCOUNTER_SPAN_DT)
    cols = np.full(max(max_rows, 1), -1, dtype=np.int32)
    speed = np.full(max(max_rows, 1), np.nan) if mode else None
    goals = np.full((max(max_rows, 1), 2), np.nan) if mode else None
    dist = np.full(max(max_rows, 1), np.nan) if measure_real else None
    step = np.full(max(max_rows, 1), -1, dtype=np.int32) if measure_real else None
    series = np.zeros(max(max_steps, 1)) if series_on else None
    n_spans, n_rows = C.c_int32(0), C.c_int64(0)
    addr = lambda a: None if a is None else a.ctypes.data
    _abi.check(handle, lib.fot_encounters_extract(handle, C.byref(p), T, A, K, ptr(xy), ptr(vel), addr(ego_xy), addr(ego_psi),
                                                  addr(ego_vel), max_spans, max_rows, C.addressof(n_spans), C.addressof(n_rows),
                                                  addr(spans), addr(cols), addr(speed), addr(goals), addr(dist), addr(step),
                                                  addr(series), max_steps))
    ns, nr = n_spans.value, n_rows.value
    spans = spans[:ns]
    kept = spans[spans["status"] == _abi.ENC_KEPT]
    steps = int(np.sum(kept["frame1"] - kept["frame0"]))
    cut = lambda a: None if a is None else a[:nr]
    return dict(spans=spans, cols=cols[:nr], cruise=cut(speed), goals=cut(goals), onset_dist=cut(dist), onset_step=cut(step),
                series=None if series is None else series[:steps])


def request_from_instance(inst, **kw) -> PlanRequest:
    """plan() arguments of a ``synthetic.Instance`` (the distribution wins over the single sample, as in the
    reference: frenet_planner.py:1043-1047)."""
    e = inst.ego
    return PlanRequest(x=e[0], y=e[1], yaw=e[2], v=e[3], a=e[4], target_speed=inst.target_speed,
                       static=inst.static, dyn=None if inst.dist is not None else inst.dyn, dist=inst.dist, **kw)
