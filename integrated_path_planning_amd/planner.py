"""Host side of the MI355X Frenet planner.

``BatchPlanner`` owns one libfot handle (one GPU) and plans many independent
ego/scenario instances per call.  ``FrenetPlanner`` keeps the call surface of the
reference class (src/planning/frenet_planner.py:125-304) on top of it, so it
drops into ``IntegratedSimulator`` (integrated_simulator.py:342-366, 576-584,
622-630, 732, 802) unchanged.  All planning arithmetic runs in the gfx950
kernels; nothing here computes a trajectory.
"""
from __future__ import annotations

import ctypes as C
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _abi
from . import batch as _batch
from .batch import PackedBatch, PlanRequest
from .data_structures import EgoVehicleState, FrenetPath, FrenetState
from .params import (D_ROAD_W, D_T_S, DT, MAX_ACCEL, MAX_CURVATURE, MAX_ROAD_WIDTH, MAX_SPEED, MAX_T, MIN_T,
                     N_S_SAMPLE, ROBOT_RADIUS, TARGET_SPEED, make_params)

from dataclasses import dataclass

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


# carrier types of the reference's polynomial builders (frenet_planner.py:95-123), for the shim's views of them
@dataclass(frozen=True)
class TimeCache:
    t: np.ndarray
    t2: np.ndarray
    t3: np.ndarray
    t4: np.ndarray
    t5: np.ndarray
    quartic_A_inv: np.ndarray
    quintic_A_inv: np.ndarray


@dataclass(frozen=True)
class LongitudinalProfile:
    t: np.ndarray
    s: np.ndarray
    s_d: np.ndarray
    s_dd: np.ndarray
    s_ddd: np.ndarray


@dataclass(frozen=True)
class LateralProfile:
    d: np.ndarray
    d_d: np.ndarray
    d_dd: np.ndarray
    d_ddd: np.ndarray


def _as_dp(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def _addr(a: np.ndarray) -> int:
    """Address of a C-contiguous array.  Plain dtypes: through ``__array_interface__`` (``ndarray.ctypes`` builds a
    helper object per access); record dtypes: through ``ndarray.ctypes`` (the interface spells out the whole record
    description on every access: 10-25 us for the ego / result records, against 1-2 us)."""
    return a.ctypes.data if a.dtype.names else a.__array_interface__["data"][0]


_vp = C.c_void_p
_FAST = {}


def _fast(lib, name, *argtypes):
    """The same exported function with untyped pointer arguments (addresses as ints)."""
    f = _FAST.get(name)
    if f is None:
        f = _FAST[name] = C.CFUNCTYPE(C.c_int, *argtypes)((name, lib))
    return f


def spline_arrays(path) -> List[np.ndarray]:
    """Knots and CubicSpline1D coefficients of a CubicSpline2D-like object
    (reference attributes: .s, .sx.{a,b,c,d}, .sy.{a,b,c,d}; cubic_spline.py:30-45, 201-204)."""
    s = np.ascontiguousarray(np.asarray(path.s, dtype=np.float64))
    out = [s]
    for sp1 in (path.sx, path.sy):
        for name in "abcd":
            out.append(np.ascontiguousarray(np.asarray(getattr(sp1, name), dtype=np.float64)))
    n = len(s)
    want = [n, n, n - 1, n, n - 1, n, n - 1, n, n - 1]
    for arr, w in zip(out, want):
        if arr.shape != (w,):
            raise ValueError(f"spline coefficient array has shape {arr.shape}, expected ({w},)")
    return out


class BatchResult:
    """Results of one batch: the raw ``fot_result`` records plus convenient views."""

    def __init__(self, records, n: int, with_stop: Sequence[bool]):
        self.records = records
        self.n = n
        self._with_stop = list(with_stop)
        self._paths = None

    def __len__(self):
        return self.n

    def status(self, i: int) -> int:
        return int(self.records[i].status)

    def stats(self, i: int) -> Optional[Dict[str, int]]:
        """``last_check_stats`` of instance i (None where the reference leaves it None)."""
        r = self.records[i]
        if not r.stats_valid:
            return None
        d = {_abi.STATUS_NAMES[k]: int(r.stats[k]) for k in range(7)}
        if self._with_stop[i]:
            d["stop_distance_error"] = int(r.stats[7])
        return d

    def _path_block(self) -> np.ndarray:
        """[n, 15, FOT_MAX_NT] float64 view of the path arrays of all records (no copy)."""
        if self._paths is None:
            raw = np.frombuffer(self.records, dtype=np.uint8).reshape(-1, _abi.RESULT_BYTES)
            off = getattr(_abi.Result, _abi.PATH_FIELDS[0]).offset
            self._paths = raw[:, off:].view(np.float64).reshape(raw.shape[0], len(_abi.PATH_FIELDS), -1)
        return self._paths

    def path(self, i: int, as_arrays: bool = False) -> Optional[FrenetPath]:
        """The selected path of instance i as the reference's FrenetPath (lists); as_arrays=True: NumPy rows, for
        callers that take thousands of paths per second (closed_loop.py)."""
        r = self.records[i]
        if r.status != _abi.PLAN_OK:
            return None
        n = int(r.n_keep)
        block = self._path_block()[i, :, :n]
        fp = FrenetPath()
        for j, f in enumerate(_abi.PATH_FIELDS):
            setattr(fp, f, block[j].copy() if as_arrays else block[j].tolist())
        fp.cost = float(r.cost)
        return fp


def _params_from_kwargs(planner_kwargs: dict) -> "_abi.Params":
    """``fot_params`` of a FrenetPlanner's keyword arguments (``footprint=`` an EgoFootprint, the rest make_params')."""
    kw = dict(planner_kwargs)
    fp = kw.pop("footprint", None)
    if fp is not None:
        kw["footprint_offsets"] = np.asarray(fp.offsets, dtype=float).tolist()
        kw["footprint_radius"] = float(fp.radius)
    return make_params(**kw)


class BatchPlanner:
    """One libfot handle: planner parameters + reference path on one GPU (scenario 0), and any further scenarios
    (``add_scenario``) that one plan call may mix."""

    def __init__(self, reference_path=None, waypoints=None, device: int = -1, sample_capacity: Optional[int] = None,
                 **planner_kwargs):
        """``sample_capacity``: the most samples S of a prediction distribution the handle accepts -- in plan calls, the
        closed loop's frames, recordings and samplers, the Social-GAN generator and the prediction scores --,
        ``_abi.MAX_SAMPLES`` (64, the default: ``None`` makes no call) to ``_abi.MAX_PLAN_SAMPLES`` (254); see
        ``set_sample_capacity``."""
        self._lib = _abi.lib()
        self.params = _params_from_kwargs(planner_kwargs)
        self.scenario_params = [self.params]     # [id]: fot_params of scenario id (0: the handle's own)
        h = C.c_void_p()
        _abi.check(None, self._lib.fot_create(C.byref(self.params), int(device), C.byref(h)))
        self._h = h
        _abi.register_owner(self)                # closed by _abi's atexit hook if the caller never does
        if sample_capacity is not None:
            self.set_sample_capacity(sample_capacity)
        if reference_path is not None:
            self.set_path(reference_path)
        elif waypoints is not None:
            self.set_waypoints(*waypoints)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        """Release the handle (idempotent).  ``fot_destroy`` polls the handle's streams for a bounded time and never
        blocks on a caller's stream; planners nobody closed are closed by ``_abi``'s atexit hook, which runs before
        the interpreter starts tearing modules down."""
        h, self._h = getattr(self, "_h", None), None
        if h:
            _abi.unregister_owner(self)
            self._lib.fot_destroy(h)

    def __del__(self):
        # Collected while the program runs: close.  During interpreter finalisation the atexit hook has already closed
        # every planner that was still registered (``_h`` is None then), so nothing calls into HIP from here.
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- capacities -------------------------------------------------------
    @property
    def sample_capacity(self) -> int:
        """Most samples of a prediction distribution any entry of the handle accepts -- ``plan_batch``,
        ``paths_collision_free``, ``check_paths``, the loop's frames, ``loop_set_samples``, ``loop_set_sampler``,
        ``sgan_noise``, the generator and ``prediction_scores`` (``fot_get_sample_capacity``); 64 unless raised."""
        n = C.c_int32(0)
        _abi.check(self._h, self._lib.fot_get_sample_capacity(self._h, C.byref(n)))
        return n.value

    def set_sample_capacity(self, n: int) -> None:
        """``fot_set_sample_capacity``: ``_abi.MAX_SAMPLES <= n <= _abi.MAX_PLAN_SAMPLES``, for all scenarios of the handle.
        A plan call with an instance of more than 64 samples runs evaluation kernels of its own ("lean-wide" /
        "general-wide" in ``last_eval_form``); every other call runs what it ran before.  The capacity is that of every
        entry that takes a sample distribution: the closed loop (five-call, one-call, resident, sweep), recorded samples,
        the Social-GAN sampler and the prediction scores accept S <= n too, and more than 64 samples run wide forms of
        the score and selection kernels.  Lowering it below the samples of a loop that is set up raises.  Out of scope:
        ``openloop_eval`` keeps 64, and the slots of one sweep share one sample count."""
        _abi.check(self._h, self._lib.fot_set_sample_capacity(self._h, int(n)))

    # -- reference path ---------------------------------------------------
    def set_path(self, path, scenario: int = 0):
        arrs = spline_arrays(path)
        if scenario == 0:
            _abi.check(self._h, self._lib.fot_set_path_coeffs(self._h, len(arrs[0]), *[_as_dp(a) for a in arrs]))
        else:
            _abi.check(self._h, self._lib.fot_set_scenario_path_coeffs(self._h, int(scenario), len(arrs[0]),
                                                                       *[_as_dp(a) for a in arrs]))

    def set_waypoints(self, wx, wy, scenario: int = 0):
        wx = np.ascontiguousarray(wx, dtype=np.float64)
        wy = np.ascontiguousarray(wy, dtype=np.float64)
        if wx.shape != wy.shape or wx.ndim != 1:
            raise ValueError("waypoints must be two 1-D arrays of equal length")
        if scenario == 0:
            _abi.check(self._h, self._lib.fot_set_path_waypoints(self._h, len(wx), _as_dp(wx), _as_dp(wy)))
        else:
            _abi.check(self._h, self._lib.fot_set_scenario_path_waypoints(self._h, int(scenario), len(wx), _as_dp(wx),
                                                                          _as_dp(wy)))

    def add_scenario(self, reference_path=None, waypoints=None, **planner_kwargs) -> int:
        """A further planner configuration + reference path (what one more reference ``FrenetPlanner`` object is) on this
        handle; same keyword arguments as the constructor.  Returns the id a ``PlanRequest.scenario`` names.  dt and
        max_t must be the handle's (one time grid per handle)."""
        params = _params_from_kwargs(planner_kwargs)
        sid = C.c_int32(-1)
        _abi.check(self._h, self._lib.fot_add_scenario(self._h, C.byref(params), C.byref(sid)))
        self.scenario_params.append(params)
        if reference_path is not None:
            self.set_path(reference_path, scenario=sid.value)
        elif waypoints is not None:
            self.set_waypoints(*waypoints, scenario=sid.value)
        return sid.value

    def path_coeffs(self, scenario: int = 0) -> List[np.ndarray]:
        n = C.c_int32(0)
        if scenario == 0:
            get = lambda *a: self._lib.fot_get_path_coeffs(self._h, *a)
        else:
            get = lambda *a: self._lib.fot_get_scenario_path_coeffs(self._h, int(scenario), *a)
        _abi.check(self._h, get(C.byref(n), *([None] * 9)))
        k = n.value
        out = [np.zeros(k), np.zeros(k), np.zeros(k - 1), np.zeros(k), np.zeros(k - 1),
               np.zeros(k), np.zeros(k - 1), np.zeros(k), np.zeros(k - 1)]
        _abi.check(self._h, get(C.byref(n), *[_as_dp(a) for a in out]))
        return out

    @property
    def n_scenarios(self) -> int:
        """Scenarios of this handle (scenario 0 and every ``add_scenario``)."""
        return len(self.scenario_params)

    def spline_eval(self, s):
        s = np.ascontiguousarray(np.atleast_1d(s), dtype=np.float64)
        out = [np.zeros_like(s) for _ in range(5)]
        _abi.check(self._h, self._lib.fot_spline_eval(self._h, len(s), _as_dp(s), *[_as_dp(a) for a in out]))
        return out      # x, y, yaw, curvature, curvature_rate

    # -- planning ---------------------------------------------------------
    def plan_packed(self, pb: PackedBatch) -> BatchResult:
        out = (_abi.Result * max(pb.n, 1))()
        if pb.mixed:
            _abi.check(self._h, self._lib.fot_plan_batch_scenarios(self._h, C.byref(pb.c), pb.scenario_ptr(), out))
        else:                                    # (= fot_plan_batch_scenarios with no scenario ids)
            _abi.check(self._h, self._lib.fot_plan_batch(self._h, C.byref(pb.c), out))
        return BatchResult(out, pb.n, [not np.isnan(v) for v in pb.max_stop[: pb.n]])

    def plan_batch(self, requests: Sequence[PlanRequest], obstacle_dtype=np.float64) -> BatchResult:
        return self.plan_packed(PackedBatch(requests, obstacle_dtype))

    def plan_packed_device(self, batch_struct: _abi.Batch, out_dev_ptr: int, stream: Optional[int] = None,
                           scenario=None):
        """Obstacles and results resident in HBM; enqueues on ``stream`` (a hipStream_t handle) and returns immediately.
        ``None`` / 0 = the handle's own stream, which no other stream waits for (torch's default stream has handle 0:
        pass an explicit ``torch.cuda.Stream`` and follow up on that stream, or call ``synchronize()``).
        ``scenario``: the instances' scenario ids (a ``PackedBatch`` -- its ``scenario`` array --, an int32 array of
        n_inst, or None = scenario 0 for all)."""
        if scenario is None:
            _abi.check(self._h, self._lib.fot_plan_batch_device(self._h, C.byref(batch_struct), C.c_void_p(out_dev_ptr),
                                                                C.c_void_p(stream) if stream else None))
            return
        if isinstance(scenario, PackedBatch):
            scen_ptr = scenario.scenario_ptr()
        else:
            scen = np.ascontiguousarray(scenario, dtype=np.int32)          # (read while the call enqueues)
            if scen.shape != (batch_struct.n_inst,):
                raise ValueError("scenario must hold one id per instance")
            scen_ptr = scen.ctypes.data_as(C.POINTER(C.c_int32))
        _abi.check(self._h, self._lib.fot_plan_batch_scenarios_device(self._h, C.byref(batch_struct), scen_ptr,
                                                                      C.c_void_p(out_dev_ptr),
                                                                      C.c_void_p(stream) if stream else None))

    @property
    def n_total_samples(self) -> int:
        """round(max_t / dt) + 1: samples per full-length candidate (the wire form's array length)."""
        return int(self._lib.fot_wire_n_total(self._h))

    def pack_records_device(self, n: int, records_dev_ptr: int, wire_dev_ptr: int, stream: Optional[int] = None):
        """fot_result[n] in HBM -> compact wire records in HBM (fot_pack_records_device), enqueued on ``stream``."""
        _abi.check(self._h, self._lib.fot_pack_records_device(self._h, int(n), C.c_void_p(records_dev_ptr),
                                                              C.c_void_p(wire_dev_ptr),
                                                              C.c_void_p(stream) if stream else None))

    # -- array interfaces: whole batches as NumPy arrays, no per-request Python objects (closed_loop.py) -----------
    RESULT_DT = np.dtype(_abi.Result)
    EGO_DT = np.dtype(_abi.Ego)
    SAFETY_DT = np.dtype(_abi.Safety)

    def plan_arrays(self, ego: np.ndarray, target_speed: np.ndarray, overrides: np.ndarray, max_stop: np.ndarray,
                    static_xy: Optional[np.ndarray], static_off: Optional[np.ndarray], dyn_xy: Optional[np.ndarray],
                    dyn_off: Optional[np.ndarray], dyn_dims: Optional[np.ndarray]) -> np.ndarray:
        """n plan() calls given column-wise (``fot_plan_batch`` with host arrays): ``ego`` structured [n] of ``EGO_DT``
        (has_prev_s 2 = chained on the request before), ``overrides`` [n, 4] float64 (NaN = key absent; max_speed,
        max_accel, max_curvature, max_lat_accel), ``max_stop`` [n] (NaN = None), obstacles as in ``fot_batch`` (float64).
        Returns the records as a structured array of ``RESULT_DT``."""
        n = int(ego.shape[0])
        out = np.zeros(max(n, 1), dtype=self.RESULT_DT)
        if n == 0:
            return out[:0]
        b = _abi.Batch()
        b.n_inst = n
        b.obstacle_dtype = _abi.F64
        ego = np.ascontiguousarray(ego, dtype=self.EGO_DT)
        tgt = np.ascontiguousarray(target_speed, dtype=np.float64)
        ov = np.ascontiguousarray(overrides, dtype=np.float64).reshape(n, 4)
        ms = np.ascontiguousarray(max_stop, dtype=np.float64)
        b.ego = C.cast(_addr(ego), C.POINTER(_abi.Ego))
        b.target_speed = C.cast(_addr(tgt), _dp)
        b.overrides = C.cast(_addr(ov), C.POINTER(_abi.Overrides))
        b.max_stop_distance = C.cast(_addr(ms), _dp)
        keep = [ego, tgt, ov, ms]
        if static_xy is not None and static_off is not None and len(static_xy):
            sx = np.ascontiguousarray(static_xy, dtype=np.float64)
            so = np.ascontiguousarray(static_off, dtype=np.int32)
            b.static_xy, b.static_off = _addr(sx), C.cast(_addr(so), _ip)
            keep += [sx, so]
        if dyn_xy is not None and dyn_off is not None and len(dyn_xy):
            dx = np.ascontiguousarray(dyn_xy, dtype=np.float64)
            do = np.ascontiguousarray(dyn_off, dtype=np.int64)
            dd = np.ascontiguousarray(dyn_dims, dtype=np.int32).reshape(n, 4)
            b.dyn_xy, b.dyn_off = _addr(dx), C.cast(_addr(do), C.POINTER(C.c_int64))
            b.dyn_dims = C.cast(_addr(dd), _ip)
            keep += [dx, do, dd]
        f = _fast(self._lib, "fot_plan_batch", _vp, _vp, _vp)
        _abi.check(self._h, f(self._h, C.addressof(b), _addr(out)))
        return out

    def safety_metrics_cat(self, egos: np.ndarray, ped_off: np.ndarray, ped_pos: np.ndarray, ped_vel: np.ndarray,
                           ego_radius: float, ped_radius: float, use_footprint: bool = True) -> np.ndarray:
        """``safety_metrics`` with the pedestrians of all egos concatenated: ego i owns rows [ped_off[i], ped_off[i+1])."""
        ego = np.ascontiguousarray(egos, dtype=np.float64).reshape(-1, 4)
        n = ego.shape[0]
        off = np.ascontiguousarray(ped_off, dtype=np.int32)
        pos = np.ascontiguousarray(ped_pos, dtype=np.float64)
        vel = np.ascontiguousarray(ped_vel, dtype=np.float64)
        out = np.zeros(max(n, 1), dtype=self.SAFETY_DT)
        f = _fast(self._lib, "fot_safety_metrics_batch", _vp, C.c_int32, _vp, _vp, _vp, _vp, C.c_double, C.c_double,
                  C.c_int32, _vp)
        _abi.check(self._h, f(self._h, n, _addr(ego), _addr(off), _addr(pos) if pos.size else None,
                              _addr(vel) if vel.size else None, float(ego_radius), float(ped_radius),
                              int(bool(use_footprint)), _addr(out)))
        return out[:n]

    def nearest_s_arrays(self, x, y, yaw, v, a, prev_s) -> np.ndarray:
        """new_prev_s of ``fot_frenet_state_batch`` for n egos given column-wise (prev_s NaN = no cached arc length)."""
        n = len(x)
        ego = np.zeros(max(n, 1), dtype=self.EGO_DT)
        ego["x"][:n], ego["y"][:n], ego["yaw"][:n], ego["v"][:n], ego["a"][:n] = x, y, yaw, v, a
        ps = np.asarray(prev_s, dtype=np.float64)
        ego["has_prev_s"][:n] = ~np.isnan(ps)
        ego["prev_s"][:n] = np.where(np.isnan(ps), 0.0, ps)
        nps = np.zeros(max(n, 1))
        f = _fast(self._lib, "fot_frenet_state_batch", _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp)
        _abi.check(self._h, f(self._h, n, _addr(ego), None, None, _addr(nps), None))
        return nps[:n]

    # -- one closed-loop step in two calls (fot_loop_*): the prediction tensor stays in HBM -------------------------
    LOOP_REQUEST_DT = np.dtype(_abi.LoopRequest)

    def loop_set_static(self, points: Optional[np.ndarray]) -> None:
        """The static obstacle points every request of the loop sees (``fot_loop_set_static``)."""
        pts = np.ascontiguousarray(np.empty((0, 2)) if points is None else points, dtype=np.float64).reshape(-1, 2)
        _abi.check(self._h, self._lib.fot_loop_set_static(self._h, len(pts), _addr(pts) if len(pts) else None))

    def loop_plan(self, requests: np.ndarray, frame: Optional[dict] = None, view: bool = False):
        """``fot_loop_plan``: constant-velocity prediction of the frame's pedestrians into the handle's own tensor,
        safety metrics of the current ego states, and the requests' plan() calls against that tensor -- one
        synchronisation.  ``requests``: structured [r] of ``LOOP_REQUEST_DT``.  ``frame`` (None = the tensor of the
        previous call): ped_off [n+1], ped_pos / ped_vel [sum P, 2], obs_last / obs_prev [sum P, 2] float32 or None
        (predictor not ready), prepend [n] bool, ego [n, 4] (x, y, yaw, v) or None, staleness, pred_len, rp
        (``_abi.ResampleParams``), ego_radius, ped_radius, use_footprint; optionally dist_raw (device pointer to raw
        samples [dist_S][pred_len][sum P][2]), dist_S, dist_dtype: the requests then plan against the distribution.
        Returns (records, metrics): the records as a structured array of ``RESULT_DT`` -- a COPY by default; with
        ``view=True`` a view of the handle's pinned block, valid only until the next ``loop_plan`` or ``close()`` on this
        planner (the lock-step driver reads it at once and keeps nothing) -- and the metrics [n] of ``SAFETY_DT`` (None
        without a frame or egos)."""
        req = np.ascontiguousarray(requests, dtype=self.LOOP_REQUEST_DT)
        r = int(req.shape[0])
        fr_addr, metrics, keep = None, None, []
        if frame is not None:
            f = _abi.LoopFrame()
            off = np.ascontiguousarray(frame["ped_off"], dtype=np.int32)
            n = len(off) - 1
            f.n_episodes, f.pred_len = n, int(frame.get("pred_len", 1))
            f.use_footprint = int(bool(frame.get("use_footprint", True)))
            pos = np.ascontiguousarray(frame["ped_pos"], dtype=np.float64)
            vel = np.ascontiguousarray(frame["ped_vel"], dtype=np.float64)
            f.ped_off, f.ped_pos, f.ped_vel = _addr(off), _addr(pos) if pos.size else None, _addr(vel) if vel.size else None
            keep += [off, pos, vel]
            if frame.get("obs_last") is not None:
                last = np.ascontiguousarray(frame["obs_last"], dtype=np.float32)
                pre = np.ascontiguousarray(frame["prepend"], dtype=np.uint8)
                f.obs_last, f.prepend = _addr(last), _addr(pre) if pre.size else None
                keep += [last, pre]
                if frame.get("obs_prev") is not None:
                    prev = np.ascontiguousarray(frame["obs_prev"], dtype=np.float32)
                    f.obs_prev = _addr(prev)
                    keep.append(prev)
                f.rp = frame["rp"]
            if frame.get("dist_raw") is not None:                      # raw samples of a multi-sample predictor, in HBM
                f.dist_raw, f.dist_S, f.dist_dtype = int(frame["dist_raw"]), int(frame["dist_S"]), int(frame["dist_dtype"])
            if frame.get("ego") is not None:
                ego = np.ascontiguousarray(frame["ego"], dtype=np.float64).reshape(n, 4)
                f.ego = _addr(ego)
                keep.append(ego)
                metrics = np.zeros(max(n, 1), dtype=self.SAFETY_DT)
            f.staleness = float(frame.get("staleness", 0.0))
            f.ego_radius, f.ped_radius = float(frame["ego_radius"]), float(frame["ped_radius"])
            fr_addr = C.addressof(f)
        rec_ptr = C.c_void_p(0)
        fn = _fast(self._lib, "fot_loop_plan", _vp, _vp, C.c_int32, _vp, _vp, _vp)
        _abi.check(self._h, fn(self._h, fr_addr, r, _addr(req) if r else None,
                               _addr(metrics) if metrics is not None else None, C.addressof(rec_ptr)))
        if r and rec_ptr.value:
            buf = (C.c_char * (r * _abi.RESULT_BYTES)).from_address(rec_ptr.value)
            records = np.frombuffer(buf, dtype=self.RESULT_DT, count=r)
            if not view:
                records = records.copy()
        else:
            records = np.zeros(0, dtype=self.RESULT_DT)
        return records, (metrics[:n] if metrics is not None else None)

    def loop_begin(self, config: "_abi.LoopConfig", ego5: np.ndarray) -> None:
        """``fot_loop_begin``: n episode slots (ego5 [n, 5] = x, y, yaw, v, a), every fail-safe machine NORMAL."""
        ego = np.ascontiguousarray(ego5, dtype=np.float64).reshape(-1, 5)
        self._loop_n = len(ego)
        self._plan_sample_mode, self._loop_sweep = _abi.LOOP_PLAN_DISTRIBUTION, False   # (fot_loop_begin* resets them)
        _abi.check(self._h, self._lib.fot_loop_begin(self._h, len(ego), C.addressof(config), _addr(ego) if len(ego) else None))

    def loop_begin_scenarios(self, configs: Sequence["_abi.LoopConfig"], use_footprint: Sequence[bool],
                             slot_scenario: np.ndarray, ego5: np.ndarray) -> None:
        """``fot_loop_begin_scenarios``: ``loop_begin`` with a scenario per episode slot.  ``configs[s]`` /
        ``use_footprint[s]``: the fail-safe constants and the metrics' footprint flag of scenario ``s``;
        ``slot_scenario[e]``: the scenario of slot e."""
        ego = np.ascontiguousarray(ego5, dtype=np.float64).reshape(-1, 5)
        scen = np.ascontiguousarray(slot_scenario, dtype=np.int32)
        if scen.shape != (len(ego),) or len(configs) != len(use_footprint) or not len(configs):
            raise ValueError("loop_begin_scenarios: one scenario id per slot, one footprint flag per configuration")
        cfgs = (_abi.LoopConfig * len(configs))(*configs)
        ufp = np.ascontiguousarray([bool(u) for u in use_footprint], dtype=np.int32)
        self._loop_n = len(ego)
        self._plan_sample_mode, self._loop_sweep = _abi.LOOP_PLAN_DISTRIBUTION, False   # (fot_loop_begin* resets them)
        _abi.check(self._h, self._lib.fot_loop_begin_scenarios(
            self._h, len(ego), len(configs), C.addressof(cfgs), _addr(ufp), _addr(scen) if len(ego) else None,
            _addr(ego) if len(ego) else None))

    _loop_sweep = False

    def loop_begin_sweep(self, configs: Sequence["_abi.LoopConfig"], use_footprint: Sequence[bool],
                         slot_scenario: np.ndarray, slot_plan_mode: Optional[np.ndarray], ego5: np.ndarray) -> None:
        """``fot_loop_begin_sweep``: ``loop_begin_scenarios`` whose lock steps may carry a distribution, planned against in
        each slot's own mode -- ``slot_plan_mode[e]``: ``_abi.LOOP_PLAN_DISTRIBUTION`` or ``_abi.LOOP_PLAN_REPRESENTATIVE``
        (None: every slot plans against the whole distribution)."""
        ego = np.ascontiguousarray(ego5, dtype=np.float64).reshape(-1, 5)
        scen = np.ascontiguousarray(slot_scenario, dtype=np.int32)
        if scen.shape != (len(ego),) or len(configs) != len(use_footprint) or not len(configs):
            raise ValueError("loop_begin_sweep: one scenario id per slot, one footprint flag per configuration")
        mode = None if slot_plan_mode is None else np.ascontiguousarray(slot_plan_mode, dtype=np.int32)
        if mode is not None and mode.shape != (len(ego),):
            raise ValueError("loop_begin_sweep: one plan mode per slot")
        cfgs = (_abi.LoopConfig * len(configs))(*configs)
        ufp = np.ascontiguousarray([bool(u) for u in use_footprint], dtype=np.int32)
        _abi.check(self._h, self._lib.fot_loop_begin_sweep(
            self._h, len(ego), len(configs), C.addressof(cfgs), _addr(ufp), _addr(scen) if len(ego) else None,
            _addr(mode) if mode is not None and len(ego) else None, _addr(ego) if len(ego) else None))
        self._loop_n = len(ego)
        self._plan_sample_mode, self._loop_sweep = _abi.LOOP_PLAN_DISTRIBUTION, True

    def loop_set_scenario_static(self, scenario: int, points: Optional[np.ndarray]) -> None:
        """The static obstacle points the loop's requests on ``scenario`` see (``fot_loop_set_scenario_static``)."""
        pts = np.ascontiguousarray(np.empty((0, 2)) if points is None else points, dtype=np.float64).reshape(-1, 2)
        _abi.check(self._h, self._lib.fot_loop_set_scenario_static(self._h, int(scenario), len(pts),
                                                                   _addr(pts) if len(pts) else None))

    def loop_step(self, frame: dict, episode: np.ndarray) -> dict:
        """``fot_loop_step``: the whole lock step of the frame's episodes (``episode[i]`` = slot of episode i) in one
        call -- prediction, metrics, level-0 plans, escalation levels of the failed ones, the retry loop, ego update /
        emergency stop, metrics of the new states and their nearest path point.  ``frame`` as for ``loop_plan`` (no
        ``ego``).  Returns the per-episode outputs as arrays plus ``records``: a structured VIEW of the step's records in
        the handle's pinned block, valid until the next loop call."""
        f, keep = self._loop_frame(frame)
        ep = np.ascontiguousarray(episode, dtype=np.int32)
        n = len(ep)
        o = dict(ego=np.zeros((n, 5)), jerk=np.zeros(n), state=np.zeros(n, np.int32), stats=np.zeros((n, 8), np.int32),
                 record=np.zeros(n, np.int32), keep=np.zeros(n, np.int32), cost=np.zeros(n),
                 before=np.zeros(max(n, 1), dtype=self.SAFETY_DT), after=np.zeros(max(n, 1), dtype=self.SAFETY_DT),
                 s_now=np.zeros(n))
        so = _abi.LoopStepOut()
        for name, arr in o.items():
            setattr(so, name, _addr(arr) if arr.size else None)
        fn = _fast(self._lib, "fot_loop_step", _vp, _vp, _vp, _vp)
        _abi.check(self._h, fn(self._h, C.addressof(f), _addr(ep) if n else None, C.addressof(so)))
        if so.n_records and so.records:
            buf = (C.c_char * (so.n_records * _abi.RESULT_BYTES)).from_address(so.records)
            o["records"] = np.frombuffer(buf, dtype=self.RESULT_DT, count=so.n_records)
        else:
            o["records"] = np.zeros(0, dtype=self.RESULT_DT)
        o["before"], o["after"] = o["before"][:n], o["after"][:n]
        return o

    def loop_set_replay(self, ped_off, n_frames, positions, velocities, *, obs_len: int, pred_len: int, rp,
                        warmup_frames: int, ego_radius: float, ped_radius: float, use_footprint: bool, s_end: float,
                        goal_distance: float = 2.0) -> None:
        """``fot_loop_set_replay``: hands the recording of every episode slot of ``loop_begin`` to the library, which
        keeps it in HBM and runs the warm-up.  positions / velocities [n_frames_max, sum P, 2] (slot e owns columns
        ``ped_off[e]:ped_off[e + 1]`` and ``n_frames[e]`` recorded frames, its last one held afterwards); rp: the
        predictor's ``ResampleParams``.  Constant-velocity predictor unless ``loop_set_sampler`` follows."""
        off = np.ascontiguousarray(ped_off, dtype=np.int32)
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        vel = np.ascontiguousarray(velocities, dtype=np.float64)
        n = len(off) - 1
        if len(nf) != n or pos.shape != vel.shape or pos.ndim != 3 or pos.shape[1:] != (int(off[-1]), 2):
            raise ValueError("loop_set_replay: positions / velocities [n_frames_max, ped_off[-1], 2], one n_frames per slot")
        r = _abi.LoopReplay()
        r.n_slots, r.n_frames_max, r.obs_len, r.pred_len = n, int(pos.shape[0]), int(obs_len), int(pred_len)
        r.warmup_frames, r.use_footprint = int(warmup_frames), int(bool(use_footprint))
        r.ped_off, r.n_frames = _addr(off), _addr(nf) if n else None
        r.pos, r.vel = (_addr(pos), _addr(vel)) if pos.size else (None, None)
        r.rp = rp
        r.ego_radius, r.ped_radius, r.s_end, r.goal_distance = float(ego_radius), float(ped_radius), float(s_end), float(goal_distance)
        _abi.check(self._h, self._lib.fot_loop_set_replay(self._h, C.addressof(r)))
        self._replay_slots = n
        self._replay_shape = (int(pred_len), int(off[-1]))           # what a recorded sample tensor must match

    def loop_run(self, max_steps: int, keep_paths: bool = True, paths_out: Optional[np.ndarray] = None) -> dict:
        """``fot_loop_run``: up to ``max_steps`` lock steps of every running episode inside the library.  Returns the
        arrays of ``fot_loop_run_out`` cut to the ``n_steps`` executed: per step and slot ``ego`` [k, n, 5], ``jerk``,
        ``state``, ``stats`` [k, n, 8], ``followed`` (1 path, 0 emergency stop, -1 the slot did not run), ``keep``,
        ``cost``, ``after`` (``SAFETY_DT``), ``s_now``; per step ``frame``, ``obs_last_frame``, ``obs_prev_frame``,
        ``staleness``; per slot ``steps``, ``termination`` (0 runs, 1 collision, 2 goal); with ``keep_paths`` ``paths``
        [k, 15, n, n_total], zero beyond ``keep`` and for slots without a path (written into ``paths_out``, a
        C-contiguous float64 array of max_steps * 15 * n * n_total elements, if given)."""
        n, k = int(self._replay_slots), int(max_steps)
        i32, m = np.int32, max(n, 1)
        o = dict(ego=np.zeros((k, n, 5)), jerk=np.zeros((k, n)), state=np.zeros((k, n), i32), stats=np.zeros((k, n, 8), i32),
                 followed=np.full((k, n), -1, i32), keep=np.zeros((k, n), i32), cost=np.zeros((k, n)),
                 after=np.zeros((k, m), dtype=self.SAFETY_DT), s_now=np.zeros((k, n)), frame=np.zeros(k, i32),
                 obs_last_frame=np.zeros(k, i32), obs_prev_frame=np.zeros(k, i32), staleness=np.zeros(k),
                 steps=np.zeros(m, i32), termination=np.zeros(m, i32))
        if keep_paths:
            shape = (k, len(_abi.PATH_FIELDS), n, self.n_total_samples)
            if paths_out is None:
                paths_out = np.empty(shape)
            elif paths_out.size != int(np.prod(shape)) or paths_out.dtype != np.float64 or not paths_out.flags.c_contiguous:
                raise ValueError(f"paths_out must be a C-contiguous float64 array of {int(np.prod(shape))} elements")
            o["paths"] = paths_out.reshape(shape)
        ro = _abi.LoopRunOut()
        for name, arr in o.items():
            setattr(ro, name, _addr(arr) if arr.size else None)
        fn = _fast(self._lib, "fot_loop_run", _vp, C.c_int32, _vp)
        done = fn(self._h, k, C.addressof(ro))
        if done < 0:
            _abi.check(self._h, done)
        for name in _abi.LOOP_RUN_OUT_FIELDS:
            if name in o and name not in ("steps", "termination"):
                o[name] = o[name][:done]
        o["after"] = o["after"][:, :n]
        o["steps"], o["termination"] = o["steps"][:n], o["termination"][:n]
        o["n_steps"] = int(done)
        return o

    LOOP_SUMMARY_DT = np.dtype(_abi.LoopSummary)

    def loop_set_sampler(self, num_samples: int, seed: int, kind: int = _abi.NOISE_GAUSSIAN, slot_crowd=None, slot_model=None,
                         model_kinds=None) -> None:
        """``fot_loop_set_sampler``: the resident loop predicts with the model of ``fot_sgan_load`` and the library's own
        counter-based noise (between ``loop_set_replay`` and the first ``loop_run``).
        slot_crowd (``fot_loop_set_sampler_shared``): one crowd id >= 0 per slot of the replay; the slots of a crowd replay
        the same pedestrians, the library samples every crowd once per lock step with noise keyed by the crowd's id and
        all its slots plan against those samples.
        slot_model, model_kinds (``fot_loop_set_sampler_models``, with slot_crowd): the id of a loaded model
        (``fot_sgan_load_model``) per slot and the noise kind of every model id 0 .. len(model_kinds) - 1; every active
        (crowd, model) pair is sampled once per lock step and ``kind`` is not read."""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if (slot_model is None) != (model_kinds is None) or (slot_model is not None and slot_crowd is None):
            raise ValueError("loop_set_sampler: slot_model, model_kinds and slot_crowd go together")
        if slot_model is not None:
            crowd, model, kinds = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (slot_crowd, slot_model, model_kinds))
            if not len(crowd) == len(model) == int(getattr(self, "_replay_slots", len(crowd))):
                raise ValueError("loop_set_sampler: slot_crowd and slot_model name one crowd and one model per slot of the replay")
            _abi.check(self._h, self._lib.fot_loop_set_sampler_models(
                self._h, int(num_samples), seed, len(kinds), _addr(kinds) if len(kinds) else None,
                int(crowd.max()) + 1 if len(crowd) else 1, _addr(crowd) if len(crowd) else None, _addr(model) if len(model) else None))
            return
        if slot_crowd is None:
            _abi.check(self._h, self._lib.fot_loop_set_sampler(self._h, int(num_samples), seed, int(kind)))
            return
        crowd = np.ascontiguousarray(slot_crowd, dtype=np.int32).reshape(-1)
        if len(crowd) != int(getattr(self, "_replay_slots", len(crowd))):
            raise ValueError("loop_set_sampler: slot_crowd names one crowd per slot of the replay")
        _abi.check(self._h, self._lib.fot_loop_set_sampler_shared(
            self._h, int(num_samples), seed, int(kind), int(crowd.max()) + 1 if len(crowd) else 1, _addr(crowd) if len(crowd) else None))

    def debug_loop_sampler_shape(self):
        """``fot_debug_loop_sampler_shape`` (tests): (scenes, pedestrian rows) the most recent lock step of a resident sampler
        loop handed to the generator; (0, 0) if that step did not sample."""
        n_scenes, n_rows = C.c_int32(-1), C.c_int32(-1)
        _abi.check(self._h, self._lib.fot_debug_loop_sampler_shape(self._h, C.addressof(n_scenes), C.addressof(n_rows)))
        return n_scenes.value, n_rows.value

    def debug_loop_sampler_shapes(self, n_models: Optional[int] = None):
        """``fot_debug_loop_sampler_shapes`` (tests): per model id 0 .. n_models - 1 (default: every id a handle holds) the
        (scenes, pedestrian rows) the most recent lock step handed to that model; (0, 0) for one that launched nothing."""
        cap = int(self._lib.fot_sgan_max_models()) if n_models is None else int(n_models)
        n_scenes, n_rows = np.full(cap, -1, np.int32), np.full(cap, -1, np.int32)
        _abi.check(self._h, self._lib.fot_debug_loop_sampler_shapes(self._h, cap, _addr(n_scenes), _addr(n_rows)))
        return [(int(a), int(b)) for a, b in zip(n_scenes, n_rows)]

    def loop_set_samples(self, samples, first_step: int = 0, n_rec_cols: Optional[int] = None, slot_col0=None) -> None:
        """``fot_loop_set_samples``: the resident loop predicts from a recorded sample tensor ``[n_steps, S, pred_len,
        sum P, 2]`` (float32 or float64; row r belongs to lock step ``first_step + r``), between ``loop_set_replay`` and
        the first ``loop_run``.  A NumPy array is copied to HBM by the call; a contiguous ``torch`` CUDA tensor is used
        in place and never written -- the engine keeps a reference to it until the next ``loop_begin*`` /
        ``loop_set_replay`` / ``loop_set_samples``.
        slot_col0 (``fot_loop_set_samples_shared``): the tensor is ``[n_steps, S, pred_len, n_rec_cols, 2]`` and pedestrian
        p of slot e reads column ``slot_col0[e] + p``; several slots may name the same columns.  n_rec_cols: None -- the
        tensor's own fourth extent."""
        if slot_col0 is None and n_rec_cols is not None:
            raise ValueError("loop_set_samples: n_rec_cols goes with slot_col0")
        on_device = hasattr(samples, "data_ptr")
        if on_device:
            import torch
            if not (samples.is_cuda and samples.is_contiguous() and samples.dtype in (torch.float32, torch.float64)):
                raise TypeError("loop_set_samples: a contiguous CUDA tensor of float32 or float64")
            code, ptr = (_abi.F32 if samples.dtype == torch.float32 else _abi.F64), samples.data_ptr()
            torch.cuda.current_stream(samples.device).synchronize()   # (the library reads it on its own stream)
        else:
            samples = np.asarray(samples)
            if samples.dtype not in (np.float32, np.float64):
                raise TypeError("loop_set_samples: float32 or float64 samples")
            samples = np.ascontiguousarray(samples)
            code, ptr = (_abi.F32 if samples.dtype == np.float32 else _abi.F64), samples.ctypes.data
        if samples.ndim != 5 or samples.shape[-1] != 2:
            raise ValueError("loop_set_samples: samples are [n_steps, S, pred_len, sum P, 2]")
        # (the library takes pred_len and the columns from the replay: a tensor of another shape would be read out of bounds)
        want = getattr(self, "_replay_shape", None)
        if slot_col0 is not None:
            # (the library takes the columns from the call: they must be the tensor's, or it would be read out of bounds)
            if n_rec_cols is not None and int(n_rec_cols) != int(samples.shape[3]):
                raise ValueError(f"loop_set_samples: n_rec_cols = {int(n_rec_cols)}, the samples are {tuple(samples.shape)}")
            if want is not None and int(samples.shape[2]) != want[0]:
                raise ValueError(f"loop_set_samples: the replay has pred_len = {want[0]}, the samples are {tuple(samples.shape)}")
            col0 = np.ascontiguousarray(slot_col0, dtype=np.int32).reshape(-1)
            if len(col0) != int(getattr(self, "_replay_slots", len(col0))):
                raise ValueError("loop_set_samples: slot_col0 names one first column per slot of the replay")
            _abi.check(self._h, self._lib.fot_loop_set_samples_shared(
                self._h, int(samples.shape[1]), int(samples.shape[0]), int(first_step), C.c_void_p(ptr) if ptr else None, code,
                _abi.OUT_DEVICE if on_device else 0, int(samples.shape[3]), _addr(col0) if len(col0) else None))
            self._loop_samples = samples if on_device else None
            return
        if want is not None and tuple(int(v) for v in samples.shape[2:4]) != want:
            raise ValueError(f"loop_set_samples: the replay has pred_len = {want[0]} and {want[1]} pedestrian columns, the "
                             f"samples are {tuple(samples.shape)}")
        _abi.check(self._h, self._lib.fot_loop_set_samples(
            self._h, int(samples.shape[1]), int(samples.shape[0]), int(first_step), C.c_void_p(ptr) if ptr else None, code,
            _abi.OUT_DEVICE if on_device else 0))
        self._loop_samples = samples if on_device else None

    def loop_set_slot_samples(self, slot_samples) -> None:
        """``fot_loop_set_slot_samples``: slot e of a sweep loop uses the first ``slot_samples[e]`` samples of what its
        source provides (after ``loop_set_samples`` / ``loop_set_sampler`` of a resident loop, before the first step; a
        stepwise sweep: before its first ``loop_step``, whose frames then carry the source's count)."""
        counts = np.ascontiguousarray(slot_samples, dtype=np.int32).reshape(-1)
        _abi.check(self._h, self._lib.fot_loop_set_slot_samples(self._h, len(counts), _addr(counts) if len(counts) else None))

    def debug_loop_slot_samples(self) -> np.ndarray:
        """``fot_debug_loop_slot_samples`` (tests): the sample count of every running episode of the most recent frame (0:
        it carried no distribution)."""
        out = np.full(max(int(self._loop_n), 1), -1, np.int32)
        _abi.check(self._h, self._lib.fot_debug_loop_slot_samples(self._h, len(out), _addr(out)))
        return out[out >= 0]

    def sgan_noise(self, seed: int, kind: int, num_samples: int, noise_dim: int, row_slot, row_step, row_index, out=None,
                   stream: Optional[int] = None):
        """``fot_sgan_noise``: the counter-based noise [S, rows, noise_dim] of the rows (slot, that slot's step count, index
        within the slot).  out: None -- a new NumPy array (uint32 for ``NOISE_RAW``, float32 otherwise); a NumPy array
        of that shape; or a ``torch`` device tensor, written where it lies on ``stream``."""
        slot, step, idx = (np.ascontiguousarray(v, dtype=np.int32) for v in (row_slot, row_step, row_index))
        rows = len(slot)
        if len(step) != rows or len(idx) != rows:
            raise ValueError("sgan_noise: one slot, step and index per row")
        shape = (int(num_samples), rows, int(noise_dim))
        if out is None:
            out = np.zeros(shape, dtype=np.uint32 if kind == _abi.NOISE_RAW else np.float32)
        on_device = hasattr(out, "data_ptr")
        if tuple(out.shape) != shape or (on_device and not out.is_contiguous()) or (not on_device and not out.flags.c_contiguous):
            raise ValueError(f"sgan_noise: out is a contiguous [S, rows, noise_dim] = {shape}")
        if out.element_size() != 4 if on_device else out.dtype.itemsize != 4:
            raise ValueError("sgan_noise: 32-bit elements")
        ptr = out.data_ptr() if on_device else out.ctypes.data
        _abi.check(self._h, self._lib.fot_sgan_noise(
            self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(kind), shape[0], rows, shape[2], slot.ctypes.data, step.ctypes.data,
            idx.ctypes.data, _abi.OUT_DEVICE if on_device else 0, C.c_void_p(ptr) if ptr else None,
            C.c_void_p(stream) if stream else None))
        return out

    def loop_summary_enable(self, on: bool = True, num_samples: int = 1) -> None:
        """``fot_loop_summary_enable``: the resident loop accumulates every slot's episode summary while it runs (between
        ``loop_set_replay`` and the first ``loop_run``).  num_samples: what ``pred_samples`` reports (the reference's
        constant-velocity predictor hands its metrics ``num_samples`` identical samples)."""
        _abi.check(self._h, self._lib.fot_loop_summary_enable(self._h, int(bool(on)), int(num_samples)))

    def loop_summaries(self) -> np.ndarray:
        """``fot_loop_summaries``: one ``fot_loop_summary`` record per slot (``LOOP_SUMMARY_DT``) of the steps run so far;
        the run may go on afterwards."""
        n = int(self._replay_slots)
        out = np.zeros(max(n, 1), dtype=self.LOOP_SUMMARY_DT)
        _abi.check(self._h, self._lib.fot_loop_summaries(self._h, n, _addr(out)))
        return out[:n]

    def loop_scores_enable(self, on: bool = True) -> None:
        """``fot_loop_scores_enable``: a resident sampler loop scores every step's distribution where it lies in HBM and
        accumulates the episode summaries while it runs (between ``loop_set_sampler`` and the first ``loop_run``)."""
        _abi.check(self._h, self._lib.fot_loop_scores_enable(self._h, int(bool(on))))

    def loop_score_summaries(self) -> np.ndarray:
        """``fot_loop_score_summaries``: one ``fot_loop_summary`` record per slot (``LOOP_SUMMARY_DT``) of the steps run so
        far -- best-of-N ADE / FDE and KDE-NLL over the origins with a complete horizon, the planning keys of the
        representative samples, the safety and comfort keys; the run may go on afterwards."""
        n = int(self._replay_slots)
        out = np.zeros(max(n, 1), dtype=self.LOOP_SUMMARY_DT)
        _abi.check(self._h, self._lib.fot_loop_score_summaries(self._h, n, _addr(out)))
        return out[:n]

    def loop_last_best_sample(self) -> np.ndarray:
        """``fot_loop_last_best_sample``: per slot the representative sample the most recent lock step chose (-1: the slot
        did not run, did not predict or has no pedestrians)."""
        # (planning on the representative sample: the slots of loop_begin, a stepwise loop's too)
        planned = self._plan_sample_mode == _abi.LOOP_PLAN_REPRESENTATIVE or self._loop_sweep
        n = int(self._loop_n if planned else getattr(self, "_replay_slots", getattr(self, "_loop_n", 0)))
        out = np.full(max(n, 1), -1, np.int32)
        _abi.check(self._h, self._lib.fot_loop_last_best_sample(self._h, n, _addr(out)))
        return out[:n]

    _plan_sample_mode = _abi.LOOP_PLAN_DISTRIBUTION

    def loop_plan_sample(self, mode: int) -> None:
        """``fot_loop_plan_sample``: what a step whose frame carries a distribution plans against --
        ``_abi.LOOP_PLAN_DISTRIBUTION`` (the default: the whole distribution under the chance constraint) or
        ``_abi.LOOP_PLAN_REPRESENTATIVE`` (every episode's representative sample, chosen and laid out on the device as
        one fixed-shape [P, n_dense + 1, 2] block).  After ``loop_begin``; with a replay set before the first ``loop_run``.
        ``loop_last_best_sample`` then answers for stepwise loops too, per slot of ``loop_begin``."""
        _abi.check(self._h, self._lib.fot_loop_plan_sample(self._h, int(mode)))
        self._plan_sample_mode = int(mode)

    def loop_run_best_samples(self, n_steps: int) -> np.ndarray:
        """``fot_loop_run_best_samples``: [n_steps, slots] -- ``loop_last_best_sample`` of every lock step of the most recent
        ``loop_run`` call (``n_steps``: the steps that call executed), for a resident run that plans on the representative
        sample."""
        n, k = int(self._replay_slots), int(n_steps)
        out = np.full((k, n), -1, np.int32)
        _abi.check(self._h, self._lib.fot_loop_run_best_samples(self._h, k, n, _addr(out) if out.size else None))
        return out

    def debug_loop_block(self, episode: int, samples: int = 1, cap_points: int = 1 << 17):
        """``fot_debug_loop_block`` (tests): (block, prepended) -- the tensor episode ``episode`` of the most recent frame
        plans against, [samples, P, T, 2] (``samples``: 1, or the frame's dist_S where the loop plans against the whole
        distribution), and the prepend flag (-1 where there is none)."""
        xy = np.zeros((max(int(cap_points), 1), 2))
        P, T, pre = C.c_int32(0), C.c_int32(0), C.c_int32(-1)
        _abi.check(self._h, self._lib.fot_debug_loop_block(self._h, int(episode), int(cap_points), _addr(xy), C.addressof(P),
                                                          C.addressof(T), C.addressof(pre)))
        n = int(samples) * P.value * T.value
        return xy[:n].reshape(int(samples), P.value, T.value, 2).copy(), pre.value

    PRED_SCORE_DT = np.dtype(_abi.PredScore)
    PRED_ORIGIN_DT = np.dtype(_abi.PredOrigin)

    def prediction_scores(self, tensor, origins, truth, stride: int, E: int, stream: Optional[int] = None) -> np.ndarray:
        """``fot_prediction_scores``: one ``fot_pred_score`` record (``PRED_SCORE_DT``) per prediction origin -- best-of-N
        ADE / FDE terms, scene level and per agent, and the KDE log-likelihood of the truth under the samples.

        tensor: the samples, a NumPy array or a contiguous ``torch`` CUDA tensor (float32 or float64; any shape, read as a
        flat run of points); origins: ``(offset, S, P, T, t_major, skip)`` per origin -- its block starts at point
        ``offset``, laid out [S, P, T, 2] or, with ``t_major``, [T, S, P, 2]; ``skip`` 1: entry 0 of every track is the
        prepended current position; truth: [sum P, E, 2], the origins' pedestrians one after the other; evaluation indices
        ``stride * j - 1``, j = 1 .. E, of the dense track.  A float32 tensor gives the scores of the rounded samples."""
        on_device = hasattr(tensor, "data_ptr")
        if on_device:
            import torch
            if not (tensor.is_cuda and tensor.is_contiguous() and tensor.dtype in (torch.float32, torch.float64)):
                raise TypeError("prediction_scores: a contiguous CUDA tensor of float32 or float64")
            code, n_points, ptr = (_abi.F32 if tensor.dtype == torch.float32 else _abi.F64), tensor.numel() // 2, tensor.data_ptr()
            if stream is None:
                torch.cuda.current_stream(tensor.device).synchronize()   # (the library reads it on its own stream)
        else:
            tensor = np.ascontiguousarray(tensor, dtype=np.float32 if np.asarray(tensor).dtype == np.float32 else np.float64)
            code, n_points, ptr = (_abi.F32 if tensor.dtype == np.float32 else _abi.F64), tensor.size // 2, tensor.ctypes.data
        desc = np.zeros(len(origins), dtype=self.PRED_ORIGIN_DT)
        for i, (offset, S, P, T, t_major, skip) in enumerate(origins):
            desc[i] = (int(offset), int(S), int(P), int(T), _abi.DYN_LAYOUT_TSP if t_major else 0, int(skip), 0)
            if offset >= 0 and min(S, P, T) > 0 and int(offset) + int(S) * int(P) * int(T) > n_points:
                raise ValueError(f"prediction_scores: origin {i} reaches past the tensor ({n_points} points)")
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        rows = int(desc["P"].clip(min=0).sum())
        if truth.size != rows * max(int(E), 0) * 2:
            raise ValueError(f"prediction_scores: truth must be [sum P = {rows}, E = {E}, 2]")
        out = np.zeros(max(len(desc), 1), dtype=self.PRED_SCORE_DT)
        _abi.check(self._h, self._lib.fot_prediction_scores(
            self._h, len(desc), _addr(desc) if len(desc) else None, C.c_void_p(ptr) if n_points else None, code,
            int(on_device), int(stride), int(E), _addr(truth) if truth.size else None, _addr(out),
            C.c_void_p(stream) if stream else None))
        return out[:len(desc)]

    def loop_prediction_scores(self, n_episodes: int, stride: int, E: int, truth: np.ndarray) -> np.ndarray:
        """``fot_loop_prediction_scores``: the records of the distribution blocks the last ``loop_step`` / ``loop_plan``
        frame with ``dist_raw`` left in the handle's tensor (the samples stay in HBM); truth [sum P, E, 2] in the frame's
        pedestrian order."""
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        out = np.zeros(max(int(n_episodes), 1), dtype=self.PRED_SCORE_DT)
        _abi.check(self._h, self._lib.fot_loop_prediction_scores(self._h, int(n_episodes), int(stride), int(E),
                                                                 _addr(truth) if truth.size else None, _addr(out)))
        return out[:int(n_episodes)]

    def openloop_eval(self, scene, win_frame0, ped_off, row_col, obs_len: int, pred_len: int, dt: float, method: int,
                      model: int = 0, num_samples: int = 1, noise=None, seed: int = 0, noise_kind: int = _abi.NOISE_GAUSSIAN,
                      win_id0: int = 0, max_rows: int = 0, want_records: bool = True, want_raw: bool = False,
                      stream: Optional[int] = None):
        """``fot_openloop_eval``: the open-loop prediction evaluation of the windows (win_frame0, ped_off, row_col) of
        ``scene`` [n_frames, n_cols, 2] -- a NumPy array or a contiguous ``torch`` CUDA tensor, float32 or float64 -- in one
        call.  method: ``_abi.OPENLOOP_CV`` or ``_abi.OPENLOOP_SGAN`` with the loaded ``model``; noise: None (the counter
        noise of ``seed`` / ``noise_kind`` / ``win_id0``), a NumPy array or a CUDA tensor [S, rows, noise_dim] float32.
        Returns ``(totals, records, raw)``: the ``_abi.OpenLoopTotals``, the windows' ``PRED_SCORE_DT`` records (None
        without ``want_records``) and, with ``want_raw``, the generator's raw samples [S, pred_len, rows, 2] float32."""
        f0, off, col = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (win_frame0, ped_off, row_col))
        n_win = len(f0)
        if len(off) != n_win + 1 or (len(off) and len(col) != max(int(off[-1]), 0)):
            raise ValueError("openloop_eval: ped_off holds n_windows + 1 offsets and row_col one column per row")
        flags = 0
        if hasattr(scene, "data_ptr"):
            import torch
            if not (scene.is_cuda and scene.is_contiguous() and scene.dtype in (torch.float32, torch.float64)):
                raise TypeError("openloop_eval: a contiguous CUDA tensor of float32 or float64")
            code, shape, s_ptr = (_abi.F32 if scene.dtype == torch.float32 else _abi.F64), tuple(scene.shape), scene.data_ptr()
            flags |= _abi.OPENLOOP_SCENE_DEVICE
            if stream is None:
                torch.cuda.current_stream(scene.device).synchronize()    # (the library reads it on its own stream)
        else:
            scene = np.ascontiguousarray(scene, dtype=np.float32 if np.asarray(scene).dtype == np.float32 else np.float64)
            code, shape, s_ptr = (_abi.F32 if scene.dtype == np.float32 else _abi.F64), scene.shape, scene.ctypes.data
        if len(shape) != 3 or shape[2] != 2:
            raise ValueError(f"openloop_eval: a scene is [n_frames, n_cols, 2], got {tuple(shape)}")
        n_ptr = None
        if noise is not None:
            if hasattr(noise, "data_ptr"):
                import torch
                if not (noise.is_cuda and noise.is_contiguous() and noise.dtype == torch.float32):
                    raise TypeError("openloop_eval: noise is a contiguous float32 CUDA tensor or a NumPy array")
                n_ptr = noise.data_ptr()
                flags |= _abi.OPENLOOP_NOISE_DEVICE
                if stream is None:
                    torch.cuda.current_stream(noise.device).synchronize()
            else:
                noise = np.ascontiguousarray(noise, dtype=np.float32)
                n_ptr = noise.ctypes.data
            if len(noise.shape) != 3 or noise.shape[0] != int(num_samples):
                raise ValueError(f"openloop_eval: noise is [S = {int(num_samples)}, rows, noise_dim], got {tuple(noise.shape)}")
        prm = _abi.OpenLoopParams(int(shape[0]), int(shape[1]), n_win, code, int(obs_len), int(pred_len), int(method), int(model),
                                  int(num_samples), int(noise_kind), int(win_id0), int(max_rows), flags, 0, float(dt),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF)
        rows = int(off[-1]) if len(off) else 0
        records = np.zeros(max(n_win, 1), dtype=self.PRED_SCORE_DT) if want_records else None
        raw = np.zeros((int(num_samples), int(pred_len), max(rows, 0), 2), np.float32) if want_raw else None
        totals = _abi.OpenLoopTotals()
        _abi.check(self._h, self._lib.fot_openloop_eval(
            self._h, C.byref(prm), C.c_void_p(s_ptr) if s_ptr else None, _addr(f0) if n_win else None, _addr(off),
            _addr(col) if len(col) else None, C.c_void_p(n_ptr) if n_ptr else None,
            _addr(records) if want_records else None, _addr(raw) if want_raw and raw.size else None, C.byref(totals),
            C.c_void_p(stream) if stream else None))
        return totals, (records[:n_win] if want_records else None), raw

    FOOTPRINT_STEP_DT = np.dtype(_abi.FootprintStep)
    FOOTPRINT_OBS_DT = np.dtype(_abi.FootprintObs)

    def footprint_recheck(self, geom: "_abi.FootprintGeom", step_off, xy, yaw, ped_off, ped_xy, want_series: bool = False,
                          want_yaw: bool = False):
        """``fot_footprint_recheck``: the trajectories (step_off [n + 1]) of poses xy [steps, 2] with the headings yaw
        [steps] (None: reconstructed on the device) and every step's pedestrians (ped_off [steps + 1], ped_xy [rows, 2])
        measured against the centre, the circle cover and the exact rectangle of ``geom`` in one call.  Returns
        ``(records, series, yaw_used)``: ``FOOTPRINT_OBS_DT`` per trajectory, ``FOOTPRINT_STEP_DT`` per step (None without
        ``want_series``) and the headings used (None without ``want_yaw``)."""
        s_off = np.ascontiguousarray(step_off, dtype=np.int32).reshape(-1)
        p_off = np.ascontiguousarray(ped_off, dtype=np.int32).reshape(-1)
        pose = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        peds = np.ascontiguousarray(ped_xy, dtype=np.float64).reshape(-1, 2)
        n, steps = len(s_off) - 1, pose.shape[0]
        if n < 0 or len(p_off) != steps + 1:
            raise ValueError("footprint_recheck: step_off holds n + 1 offsets and ped_off one more than there are steps")
        head = None if yaw is None else np.ascontiguousarray(yaw, dtype=np.float64).reshape(-1)
        if head is not None and len(head) != steps:
            raise ValueError("footprint_recheck: one heading per step")
        if s_off[-1] != steps or (len(p_off) and max(int(p_off[-1]), 0) != peds.shape[0]):
            raise ValueError("footprint_recheck: the offsets' last entries are the number of steps and of pedestrian rows")
        out = np.zeros(max(n, 1), dtype=self.FOOTPRINT_OBS_DT)
        series = np.zeros(max(steps, 1), dtype=self.FOOTPRINT_STEP_DT) if want_series else None
        used = np.zeros(max(steps, 1)) if want_yaw else None
        _abi.check(self._h, self._lib.fot_footprint_recheck(
            self._h, C.byref(geom), n, _addr(s_off), _addr(pose) if steps else None, _addr(head) if head is not None else None,
            _addr(p_off), _addr(peds) if peds.size else None, _addr(series) if want_series else None,
            _addr(used) if want_yaw else None, _addr(out)))
        return out[:n], (series[:steps] if want_series else None), (used[:steps] if want_yaw else None)

    def loop_footprint_enable(self, geom: Optional["_abi.FootprintGeom"]) -> None:
        """``fot_loop_footprint_enable``: every lock step of this loop (one-call step or resident) also measures the new ego
        states against the fixed observational geometries; None switches it off.  Between ``loop_begin*`` and the first step."""
        _abi.check(self._h, self._lib.fot_loop_footprint_enable(self._h, C.byref(geom) if geom is not None else None))

    def loop_footprint_obs(self, n_slots: int) -> np.ndarray:
        """``fot_loop_footprint_obs``: one ``FOOTPRINT_OBS_DT`` record per slot over the lock steps run so far."""
        n = int(n_slots)
        out = np.zeros(max(n, 1), dtype=self.FOOTPRINT_OBS_DT)
        _abi.check(self._h, self._lib.fot_loop_footprint_obs(self._h, n, _addr(out)))
        return out[:n]

    def fidelity_eval(self, encounters: "_batch.PackedEncounters", **thresholds):
        """``fot_fidelity_eval`` (``batch.fidelity_eval``): separation, avoidance onset and roll-out error of packed
        encounters in one call."""
        if not hasattr(self._lib, "fot_fidelity_eval"):
            raise RuntimeError("this libfot.so has no fot_fidelity_eval: rebuild it")
        return _batch.fidelity_eval(self._lib, self._h, encounters, **thresholds)

    def encounters_extract(self, ped_xy, ped_vel, ego_xy, ego_psi, ego_vel, dt: float, **options):
        """``fot_encounters_extract`` (``batch.encounters_extract``): the candidate spans of one clip's vehicles, their
        populations and closest approaches, the kept encounters' recorded-side statistics and roll-out boundary
        conditions, in one call.  ``ped_xy`` / ``ped_vel`` may be device tensors [T, A, 2] of float64."""
        if not hasattr(self._lib, "fot_encounters_extract"):
            raise RuntimeError("this libfot.so has no fot_encounters_extract: rebuild it")
        return _batch.encounters_extract(self._lib, self._h, ped_xy, ped_vel, ego_xy, ego_psi, ego_vel, dt, **options)

    def _loop_frame(self, frame: dict):
        """fot_loop_frame from the dictionary ``loop_plan`` / ``loop_step`` take (+ the arrays it points into)."""
        f, keep = _abi.LoopFrame(), []
        off = np.ascontiguousarray(frame["ped_off"], dtype=np.int32)
        n = len(off) - 1
        f.n_episodes, f.pred_len = n, int(frame.get("pred_len", 1))
        f.use_footprint = int(bool(frame.get("use_footprint", True)))
        pos = np.ascontiguousarray(frame["ped_pos"], dtype=np.float64)
        vel = np.ascontiguousarray(frame["ped_vel"], dtype=np.float64)
        f.ped_off, f.ped_pos, f.ped_vel = _addr(off), _addr(pos) if pos.size else None, _addr(vel) if vel.size else None
        keep += [off, pos, vel]
        if frame.get("obs_last") is not None:
            last = np.ascontiguousarray(frame["obs_last"], dtype=np.float32)
            pre = np.ascontiguousarray(frame["prepend"], dtype=np.uint8)
            f.obs_last, f.prepend = _addr(last), _addr(pre) if pre.size else None
            keep += [last, pre]
            if frame.get("obs_prev") is not None:
                prev = np.ascontiguousarray(frame["obs_prev"], dtype=np.float32)
                f.obs_prev = _addr(prev)
                keep.append(prev)
            f.rp = frame["rp"]
        if frame.get("dist_raw") is not None:                          # raw samples of a multi-sample predictor, in HBM
            f.dist_raw, f.dist_S, f.dist_dtype = int(frame["dist_raw"]), int(frame["dist_S"]), int(frame["dist_dtype"])
        f.staleness = float(frame.get("staleness", 0.0))
        f.ego_radius, f.ped_radius = float(frame["ego_radius"]), float(frame["ped_radius"])
        f._keep = keep                                               # (the arrays live as long as the structure)
        return f, keep

    def gather_paths(self, records: np.ndarray, index: np.ndarray, kmax: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The first ``kmax`` samples of the 15 path arrays of ``records[index]`` as one dense [15, n, kmax] block
        (``fot_gather_paths``; ``_abi.PATH_FIELDS`` order), written into ``out`` (C-contiguous, that shape) if given."""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        shape = (len(_abi.PATH_FIELDS), len(idx), int(kmax))
        if out is None:
            out = np.empty(shape)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float64 array of shape {shape}")
        if out.size:
            fn = _fast(self._lib, "fot_gather_paths", _vp, C.c_int32, _vp, C.c_int32, _vp)
            rc = fn(_addr(records), len(idx), _addr(idx), int(kmax), _addr(out))
            if rc != 0:
                raise _abi.FotError(rc, "fot_gather_paths: bad index or length")
        return out

    def loop_observe(self, ego5: np.ndarray, prev_s: np.ndarray):
        """``fot_loop_observe``: safety metrics of the new ego states [n, 5] (x, y, yaw, v, a; ego i = episode i of
        the frame) against the frame's pedestrians, and the arc length of their nearest path point (prev_s NaN = no
        cached arc length) -- one synchronisation.  Returns (metrics [n] of ``SAFETY_DT``, s [n])."""
        ego = np.ascontiguousarray(ego5, dtype=np.float64).reshape(-1, 5)
        n = ego.shape[0]
        ps = np.ascontiguousarray(prev_s, dtype=np.float64)
        metrics = np.zeros(max(n, 1), dtype=self.SAFETY_DT)
        s = np.zeros(max(n, 1))
        fn = _fast(self._lib, "fot_loop_observe", _vp, C.c_int32, _vp, _vp, _vp, _vp)
        _abi.check(self._h, fn(self._h, n, _addr(ego), _addr(ps), _addr(metrics), _addr(s)))
        return metrics[:n], s[:n]

    def loop_observe_begin(self, ego5: np.ndarray, prev_s: np.ndarray):
        """``loop_observe`` in two halves: enqueues the launches and returns a callable that waits for them and returns
        (metrics, s) -- host work in between overlaps with the device.  No other call on this planner before it."""
        ego = np.ascontiguousarray(ego5, dtype=np.float64).reshape(-1, 5)
        n = ego.shape[0]
        ps = np.ascontiguousarray(prev_s, dtype=np.float64)
        fn = _fast(self._lib, "fot_loop_observe_begin", _vp, C.c_int32, _vp, _vp)
        _abi.check(self._h, fn(self._h, n, _addr(ego), _addr(ps)))

        def collect():
            metrics = np.zeros(max(n, 1), dtype=self.SAFETY_DT)
            s = np.zeros(max(n, 1))
            fe = _fast(self._lib, "fot_loop_observe_end", _vp, _vp, _vp)
            _abi.check(self._h, fe(self._h, _addr(metrics), _addr(s)))
            return metrics[:n], s[:n]
        return collect

    def synchronize(self):
        _abi.check(self._h, self._lib.fot_synchronize(self._h))

    def profile(self, on: bool):
        """Bracket every kernel launch with HIP events on its stream (fot_profile_enable)."""
        _abi.check(self._h, self._lib.fot_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, reset: bool = True) -> Dict[str, Dict[str, float]]:
        """Per kernel: launches and summed device ms since the last reset (waits for the work)."""
        n = _abi.PROFILE_KERNELS
        launches = np.zeros(n, np.int32)
        ms = np.zeros(n)
        rc = self._lib.fot_profile_read(self._h, 1 if reset else 0, n, launches.ctypes.data_as(_ip), _as_dp(ms))
        if rc < 0:
            _abi.check(self._h, rc)
        return {self._lib.fot_profile_kernel_name(k).decode(): {"launches": int(launches[k]), "total_ms": float(ms[k])}
                for k in range(n)}

    def candidates(self, inst: int = 0, cap: int = 1 << 16):
        """Per-candidate (cost, status, keep, n_t) of an instance of the last plan call."""
        cost = np.zeros(cap)
        status = np.zeros(cap, np.int32)
        keep = np.zeros(cap, np.int32)
        nt = np.zeros(cap, np.int32)
        n = self._lib.fot_debug_candidates(self._h, inst, cap, _as_dp(cost), status.ctypes.data_as(_ip),
                                           keep.ctypes.data_as(_ip), nt.ctypes.data_as(_ip))
        if n < 0:
            _abi.check(self._h, n)
        n = min(n, cap)
        return cost[:n], status[:n], keep[:n], nt[:n]

    def margins(self, inst: int = 0, cap: int = 1 << 16) -> np.ndarray:
        """[n_cand, 8] smallest relative distance to a threshold per candidate and decision group
        (``_abi.MARGIN_NAMES``) of an instance of the last plan call; +inf where no such decision was made."""
        out = np.full((cap, _abi.MARGIN_GROUPS), np.inf)
        n = self._lib.fot_debug_margins(self._h, inst, cap, _as_dp(out))
        if n < 0:
            _abi.check(self._h, n)
        return out[: min(n, cap)]

    def set_eval_segments(self, n_seg: int) -> None:
        """Test hook (``fot_debug_set_eval_segments``): time segments per candidate in the evaluation kernel,
        1..4 forced, 0 = chosen by batch size."""
        _abi.check(self._h, self._lib.fot_debug_set_eval_segments(self._h, int(n_seg)))

    def set_tile_cut(self, cut) -> None:
        """Test hook (``fot_debug_set_tile_cut``): 0 / "auto", 1 / "wave" (k_evaluate, per-wave rows), 2 / "group"
        (k_evaluate_group, four tiles per row table)."""
        cut = {"auto": 0, "wave": 1, "group": 2}.get(cut, cut)
        _abi.check(self._h, self._lib.fot_debug_set_tile_cut(self._h, int(cut)))

    def set_eval_form(self, form) -> int:
        """Test hook (``fot_debug_set_eval_form``): 0 / "auto" (the lean evaluation kernels where a launch is eligible:
        at most 64 samples, the single centre circle, epsilon = 0 on every instance), 1 / "general" (the general form
        always), -1 / "query".  Returns the forms the most recent plan call's launches took: 0 none yet, 1 general,
        2 lean, 3 both; a wide launch (an instance of more than 64 samples) adds 4 (general) or 8 (lean) instead."""
        form = {"auto": 0, "general": 1, "query": -1}.get(form, form)
        rc = self._lib.fot_debug_set_eval_form(self._h, int(form))
        if rc < 0:
            _abi.check(self._h, rc)
        return rc

    def set_flat(self, on) -> bool:
        """Test hook (``fot_debug_set_flat``): 1 / "auto" (the flat form of the lean evaluation kernels where every path
        of a lean-eligible launch is exactly straight; the default), 0 / "off" (never), -1 / "query".  Returns whether a
        launch of the most recent plan call took a flat kernel."""
        on = {"auto": 1, "off": 0, "query": -1}.get(on, on)
        rc = self._lib.fot_debug_set_flat(self._h, int(on))
        if rc < 0:
            _abi.check(self._h, rc)
        return bool(rc)

    def last_eval_form(self) -> str:
        """Which evaluation kernels the most recent plan call ran: "none", "general", "lean" or "both"; "general-wide" or
        "lean-wide" for a call with an instance of more than 64 samples ("both" when its lanes took different forms)."""
        return {0: "none", 1: "general", 2: "lean", 3: "both", 4: "general-wide", 8: "lean-wide"}.get(self.set_eval_form(-1), "both")

    def time_info(self, time: float):
        """(n_t, quartic inverse [2, 2], quintic inverse [3, 3]) the library solves a horizon of ``time`` seconds with
        (``fot_debug_time_info``)."""
        n_t = C.c_int32(0)
        qa, qi = np.zeros(4), np.zeros(9)
        _abi.check(self._h, self._lib.fot_debug_time_info(self._h, float(time), C.byref(n_t), _as_dp(qa), _as_dp(qi)))
        return int(n_t.value), qa.reshape(2, 2), qi.reshape(3, 3)

    def candidate_path(self, index: int, inst: int = 0) -> FrenetPath:
        """Candidate ``index`` of the last plan call as generated + converted, before truncation."""
        arr = np.zeros((15, _abi.MAX_NT))
        nt = C.c_int32(0)
        _abi.check(self._h, self._lib.fot_debug_candidate_path(self._h, inst, int(index), _as_dp(arr), C.byref(nt)))
        fp = FrenetPath()
        for k, f in enumerate(_abi.PATH_FIELDS):
            setattr(fp, f, arr[k, : nt.value].tolist())
        return fp

    def frenet_states(self, egos: Sequence[PlanRequest]):
        n = len(egos)
        arr = (_abi.Ego * max(n, 1))()
        for i, r in enumerate(egos):
            e = arr[i]
            e.x, e.y, e.yaw, e.v, e.a, e.last_kappa = r.x, r.y, r.yaw, r.v, r.a, r.last_kappa
            e.has_prev_s = 0 if r.prev_s is None else 1
            e.prev_s = 0.0 if r.prev_s is None else r.prev_s
        fr = np.zeros((max(n, 1), 6))
        ref = np.zeros((max(n, 1), 6))
        nps = np.zeros(max(n, 1))
        ok = np.zeros(max(n, 1), np.int32)
        _abi.check(self._h, self._lib.fot_frenet_state_batch(self._h, n, arr, _as_dp(fr), _as_dp(ref), _as_dp(nps),
                                                             ok.ctypes.data_as(_ip)))
        return fr[:n], ref[:n], nps[:n], ok[:n]

    def safety_metrics(self, egos, ped_positions: Sequence, ped_velocities: Sequence, ego_radius: float,
                       ped_radius: float, use_footprint: bool = True) -> np.ndarray:
        """compute_safety_metrics_static (data_structures.py:301-388) for n egos in one launch.

        egos [n, 4] = x, y, yaw, v; ped_positions / ped_velocities: one [P_i, 2] array per ego.  Returns a structured
        array with fields min_distance, ttc, clearance, clearance_ahead, collision."""
        ego = np.ascontiguousarray(egos, dtype=np.float64).reshape(-1, 4)
        n = ego.shape[0]
        if len(ped_positions) != n or len(ped_velocities) != n:
            raise ValueError("one pedestrian array per ego is required")
        off = np.zeros(n + 1, np.int32)
        pos, vel = [], []
        for i in range(n):
            p = np.asarray(ped_positions[i], dtype=np.float64).reshape(-1, 2)
            v = np.asarray(ped_velocities[i], dtype=np.float64).reshape(-1, 2)
            if p.shape != v.shape:
                raise ValueError(f"ego {i}: positions {p.shape} and velocities {v.shape} differ")
            off[i + 1] = off[i] + p.shape[0]
            pos.append(p); vel.append(v)
        pos = np.ascontiguousarray(np.concatenate(pos, axis=0)) if n else np.empty((0, 2))
        vel = np.ascontiguousarray(np.concatenate(vel, axis=0)) if n else np.empty((0, 2))
        out = (_abi.Safety * max(n, 1))()
        _abi.check(self._h, self._lib.fot_safety_metrics_batch(
            self._h, n, _as_dp(ego), off.ctypes.data_as(_ip), _as_dp(pos) if pos.size else None,
            _as_dp(vel) if vel.size else None, float(ego_radius), float(ped_radius), int(bool(use_footprint)), out))
        return np.ctypeslib.as_array(out)[:n].copy() if n else np.zeros(0, dtype=np.dtype(_abi.Safety))

    @staticmethod
    def _pack_paths(paths: Sequence, fields: Sequence[str]):
        """FrenetPath-like objects -> {field: [n, MAX_NT]} arrays, lengths of x / t, and the per-rule lengths of
        ``fot_check_paths`` [n, CHECK_RULE_LENS]: every array keeps its own length (the reference applies each rule over
        the arrays that rule reads, frenet_planner.py:944-984, :1013-1022, :317-318), zeros behind it."""
        n = len(paths)
        arrs = {f: np.zeros((max(n, 1), _abi.MAX_NT)) for f in fields}
        ln = np.zeros(max(n, 1), np.int32)
        rule_len = np.zeros((max(n, 1), _abi.CHECK_RULE_LENS), np.int32)
        for i, fp in enumerate(paths):
            m = min(len(fp.x), len(fp.t))                        # frenet_planner.py:1146
            own = {}
            for f in fields:
                v = getattr(fp, f, None)
                v = np.zeros(0) if v is None else np.asarray(v, dtype=float)
                if len(v) > _abi.MAX_NT:
                    raise ValueError(f"path {i}: {f} is longer than {_abi.MAX_NT} samples")
                own[f] = len(v)
                arrs[f][i, :len(v)] = v
                if f == "yaw" and 0 < len(v) < m:                # :1158-1161 hold the last value
                    arrs[f][i, len(v):m] = v[-1]
            ln[i] = m
            geo = min(own.get(f, 0) for f in ("x", "y", "yaw", "s", "d"))
            rule_len[i] = [geo] + [own.get(f, 0) for f in ("d", "v", "a", "c", "s")]
        return arrs, ln, rule_len

    def _obstacle_args(self, static, dyn, dist):
        req = PlanRequest(0, 0, 0, 0, 0, static=static, dyn=dyn, dist=dist)
        pb = PackedBatch([req], np.float64)
        mode, S, P, T = (int(v) for v in pb.dyn_dims[0])
        st = pb.static_xy
        return pb, (int(st.shape[0]), _as_dp(st) if st.size else None, mode, S, P, T,
                    _as_dp(pb.dyn_xy) if pb.dyn_xy.size else None)

    def paths_collision_free(self, paths: Sequence, static=None, dyn=None, dist=None) -> np.ndarray:
        """_path_is_collision_free (frenet_planner.py:1035-1047) for FrenetPath-like objects."""
        n = len(paths)
        arrs, ln, _ = self._pack_paths(paths, ("x", "y", "yaw", "t"))
        keep, oargs = self._obstacle_args(static, dyn, dist)
        free = np.zeros(max(n, 1), np.int32)
        _abi.check(self._h, self._lib.fot_check_collision_paths(
            self._h, n, ln.ctypes.data_as(_ip), _as_dp(arrs["x"]), _as_dp(arrs["y"]), _as_dp(arrs["yaw"]),
            _as_dp(arrs["t"]), *oargs, free.ctypes.data_as(_ip)))
        return free[:n].astype(bool)

    def check_paths(self, paths: Sequence, static=None, dyn=None, overrides=None, dist=None,
                    max_stop_distance=None) -> np.ndarray:
        """_check_paths (+ stop-distance filter) categories of FrenetPath-like objects: FOT_ST_* per path."""
        n = len(paths)
        fields = ("x", "y", "yaw", "v", "a", "c", "d", "s", "t")
        arrs, ln, rule_len = self._pack_paths(paths, fields)
        for i, fp in enumerate(paths):                           # :933-940 silently skipped
            if len(fp.x) == 0 or len(fp.x) != len(fp.t):
                ln[i] = 0
        keep, oargs = self._obstacle_args(static, dyn, dist)
        ov = _abi.Overrides()
        o = overrides or {}
        nan = float("nan")
        ov.max_speed, ov.max_accel = float(o.get("max_speed", nan)), float(o.get("max_accel", nan))
        ov.max_curvature, ov.max_lat_accel = float(o.get("max_curvature", nan)), float(o.get("max_lat_accel", nan))
        status = np.zeros(max(n, 1), np.int32)
        _abi.check(self._h, self._lib.fot_check_paths(
            self._h, n, ln.ctypes.data_as(_ip), rule_len.ctypes.data_as(_ip), *[_as_dp(arrs[f]) for f in fields],
            C.byref(ov), nan if max_stop_distance is None else float(max_stop_distance), *oargs,
            status.ctypes.data_as(_ip)))
        status = status[:n]
        status[ln[:n] == 0] = _abi.ST_DROPPED
        return status


class _NearestPointState:
    """Stands in for ``planner.converter`` of the reference: carries the cached arc length
    (CoordinateConverter._prev_s, coordinate_converter.py:221, 283); absent until the first search."""

    def __init__(self, path):
        self.reference_path = path


class FrenetPlanner:
    """Drop-in for the reference's FrenetPlanner (frenet_planner.py:125-304) backed by libfot."""

    def __init__(self, reference_path, max_speed: float = MAX_SPEED, max_accel: float = MAX_ACCEL,
                 max_curvature: float = MAX_CURVATURE, dt: float = DT, d_road_w: float = D_ROAD_W,
                 max_road_width: float = MAX_ROAD_WIDTH, robot_radius: float = ROBOT_RADIUS,
                 obstacle_radius: float = 0.3, min_t: float = MIN_T, max_t: float = MAX_T, d_t_s: float = D_T_S,
                 n_s_sample: int = N_S_SAMPLE, **kwargs):
        self.csp = reference_path
        self.max_speed = max_speed
        self.max_accel = max_accel
        self.max_curvature = max_curvature
        self.max_lat_accel = float(kwargs.get("max_lat_accel", 3.0))
        self.dt = dt
        self.d_road_w = d_road_w
        self.max_road_width = max_road_width
        self.robot_radius = robot_radius
        self.obstacle_radius = obstacle_radius
        self.min_t = min_t
        self.max_t = max_t
        self.d_t_s = d_t_s
        self.n_s_sample = n_s_sample
        self.k_j = kwargs.get("k_j", 0.1)
        self.k_t = kwargs.get("k_t", 0.1)
        self.k_d = kwargs.get("k_d", 1.0)
        self.k_s_dot = kwargs.get("k_s_dot", 1.0)
        self.k_lat = kwargs.get("k_lat", 1.0)
        self.k_lon = kwargs.get("k_lon", 1.0)
        self.chance_epsilon = float(kwargs.get("chance_epsilon", 0.0))
        self.collision_margin_inflation = float(kwargs.get("collision_margin_inflation", 1.0))
        self.footprint = kwargs.get("footprint", None)
        self.converter = _NearestPointState(reference_path)
        self._last_kappa = 0.0
        self.last_check_stats = None
        # The reference plans any lattice and its plan() never raises (frenet_planner.py:266-268: a failure is `None`).
        # The library has capacities (include/fot.h FOT_MAX_*: 256 samples per candidate, 64 horizons, 32 terminal speeds,
        # 32 brake horizons, 8 footprint circles, 64 prediction samples -- up to 254 with sample_capacity=); a configuration
        # or a call beyond them keeps the reference's contract: a warning once, plan() returns None with last_check_stats
        # None, and `last_error` says why.
        self.last_error: Optional[str] = None
        self._warned = False
        self.sample_capacity = kwargs.get("sample_capacity", None)     # of every engine this planner builds
        try:
            self._engine = BatchPlanner(
                reference_path=reference_path, device=int(kwargs.get("device", -1)), sample_capacity=self.sample_capacity,
                max_speed=max_speed, max_accel=max_accel, max_curvature=max_curvature, dt=dt, d_road_w=d_road_w,
                max_road_width=max_road_width, robot_radius=robot_radius, obstacle_radius=obstacle_radius, min_t=min_t,
                max_t=max_t, d_t_s=d_t_s, max_lat_accel=self.max_lat_accel, k_j=self.k_j, k_t=self.k_t, k_d=self.k_d,
                k_s_dot=self.k_s_dot, k_lat=self.k_lat, k_lon=self.k_lon, chance_epsilon=self.chance_epsilon,
                collision_margin_inflation=self.collision_margin_inflation, footprint=self.footprint)
        except _abi.FotError as e:
            if e.code != _abi.ERR_UNSUPPORTED:
                raise
            self._engine = None
            self._unsupported(str(e))

    def _unsupported(self, msg: str) -> None:
        self.last_error = msg
        if not self._warned:
            import warnings
            warnings.warn(f"FrenetPlanner: beyond the library's capacities, plan() returns None ({msg})", RuntimeWarning,
                          stacklevel=3)
            self._warned = True

    @property
    def engine(self) -> BatchPlanner:
        return self._engine

    def _request(self, ego_state, static_obstacles, dynamic_obstacles, target_speed, constraint_overrides,
                 dynamic_obstacles_distribution, max_stop_distance) -> PlanRequest:
        return PlanRequest(
            x=float(ego_state.x), y=float(ego_state.y), yaw=float(ego_state.yaw), v=float(ego_state.v),
            a=float(ego_state.a), target_speed=float(target_speed), last_kappa=float(self._last_kappa),
            prev_s=getattr(self.converter, "_prev_s", None), overrides=constraint_overrides or None,
            max_stop_distance=max_stop_distance, static=static_obstacles, dyn=dynamic_obstacles,
            dist=dynamic_obstacles_distribution)

    def plan(self, ego_state: EgoVehicleState, static_obstacles: np.ndarray,
             dynamic_obstacles: Optional[np.ndarray] = None, target_speed: float = TARGET_SPEED,
             constraint_overrides: Optional[Dict[str, float]] = None,
             dynamic_obstacles_distribution: Optional[np.ndarray] = None,
             max_stop_distance: Optional[float] = None) -> Optional[FrenetPath]:
        """Same contract as the reference (frenet_planner.py:227-304): best path or None; never
        raises on "no path"; updates last_check_stats, _last_kappa and the nearest-point cache."""
        self.last_check_stats = None
        if self._engine is None:                                   # (a configuration beyond the library's capacities)
            return None
        req = self._request(ego_state, static_obstacles, dynamic_obstacles, target_speed, constraint_overrides,
                            dynamic_obstacles_distribution, max_stop_distance)
        try:
            res = self._engine.plan_batch([req])
        except _abi.FotError as e:                                 # (a call beyond them: more prediction samples than 64, ...)
            if e.code != _abi.ERR_UNSUPPORTED:
                raise
            self._unsupported(str(e))
            return None
        self.last_error = None
        rec = res.records[0]
        if not np.isnan(rec.new_prev_s):
            self.converter._prev_s = float(rec.new_prev_s)
        self.last_check_stats = res.stats(0)
        path = res.path(0)
        if path is not None:
            self._last_kappa = float(rec.new_last_kappa)
        return path

    def reset_ego_curvature(self):
        self._last_kappa = 0.0

    # -- stages the reference's tests reach into ---------------------------
    def _cartesian_to_frenet_state(self, ego_state) -> Optional[FrenetState]:
        req = PlanRequest(ego_state.x, ego_state.y, ego_state.yaw, ego_state.v, ego_state.a,
                          last_kappa=self._last_kappa, prev_s=getattr(self.converter, "_prev_s", None))
        fr, _ref, nps, ok = self._engine.frenet_states([req])
        if not np.isnan(nps[0]):
            self.converter._prev_s = float(nps[0])
        if not ok[0]:
            return None
        return FrenetState(*[float(v) for v in fr[0]])

    def _path_is_collision_free(self, fp, static_obstacles, dynamic_obstacles, dynamic_distribution) -> bool:
        return bool(self._engine.paths_collision_free([fp], static_obstacles, dynamic_obstacles,
                                                      dynamic_distribution)[0])

    def _check_collision(self, fp, static_obstacles, dynamic_obstacles=None) -> bool:
        return self._path_is_collision_free(fp, static_obstacles, dynamic_obstacles, None)

    def _engine_for_epsilon(self, epsilon: float) -> BatchPlanner:
        """chance_epsilon is a handle constant; other values get their own (cached) handle."""
        if float(epsilon) == self.chance_epsilon:
            return self._engine
        cache = self.__dict__.setdefault("_eps_engines", {})
        if float(epsilon) not in cache:
            p = self._engine.params
            kw = {name: getattr(p, name) for name, _ in p._fields_
                  if name not in ("_pad", "n_circles", "footprint_radius", "footprint_offsets", "chance_epsilon")}
            cache[float(epsilon)] = BatchPlanner(reference_path=self.csp, chance_epsilon=float(epsilon),
                                                 footprint=self.footprint, sample_capacity=self.sample_capacity, **kw)
        return cache[float(epsilon)]

    def _check_collision_distribution(self, fp, static_obstacles, dynamic_distribution, epsilon=None) -> bool:
        eng = self._engine_for_epsilon(self.chance_epsilon if epsilon is None else epsilon)
        if dynamic_distribution is None or np.size(dynamic_distribution) == 0:
            return bool(eng.paths_collision_free([fp], static_obstacles, None, None)[0])
        return bool(eng.paths_collision_free([fp], static_obstacles, None, dynamic_distribution)[0])

    def _check_paths(self, fp_list, static_obstacles, dynamic_obstacles=None, constraint_overrides=None,
                     dynamic_obstacles_distribution=None) -> dict:
        """Same categorisation as the reference's _check_paths (frenet_planner.py:891-993), on the device."""
        status = self._engine.check_paths(fp_list, static_obstacles, dynamic_obstacles, constraint_overrides,
                                          dynamic_obstacles_distribution)
        out = {k: [] for k in _abi.STATUS_NAMES[:7]}
        for fp, st in zip(fp_list, status):
            if st < 7:
                out[_abi.STATUS_NAMES[st]].append(fp)
        return out

    # The generation / conversion stages as separate calls (frenet_planner.py:376-503, 736-889).  libfot generates,
    # converts and checks a candidate in one pass over registers; these views re-run the lattice from the GIVEN Frenet
    # state (FOT_EGO_IS_FRENET) and read the candidates back through the debug entries -- what the reference's tests
    # look at, not a path plan() takes.
    _FRENET_FIELDS = ("t", "s", "s_d", "s_dd", "s_ddd", "d", "d_d", "d_dd", "d_ddd")
    _CART_FIELDS = ("x", "y", "yaw", "v", "a", "c")

    # --- the reference's polynomial builders, as views (its test-suite calls them; plan() never does: the lattice is
    # generated on the device).  The boundary-value inverses are the library's own closed forms.
    def _build_time_cache(self, time: float) -> "TimeCache":
        """frenet_planner.py:586-617: inclusive sample grid of the horizon, its powers, the two inverses."""
        n_t, qa, qi = self._engine.time_info(time)
        t = np.arange(n_t) * self.dt
        t2 = t * t
        return TimeCache(t=t, t2=t2, t3=t2 * t, t4=t2 * t2, t5=t2 * t2 * t, quartic_A_inv=qa, quintic_A_inv=qi)

    def _build_longitudinal_profiles(self, frenet_state, target_velocities, time: float, time_cache) -> list:
        """frenet_planner.py:619-658: one quartic per terminal speed (s(0), s'(0), s''(0) from the state; s'(T) = tv,
        s''(T) = 0), sampled on the cache's grid."""
        tc = time_cache
        a0, a1, a2 = frenet_state.s, frenet_state.s_d, frenet_state.s_dd / 2.0
        out = []
        for tv in np.asarray(target_velocities, dtype=float):
            a3, a4 = tc.quartic_A_inv @ np.array([tv - a1 - 2.0 * a2 * time, -2.0 * a2])
            out.append(LongitudinalProfile(
                t=tc.t, s=a0 + a1 * tc.t + a2 * tc.t2 + a3 * tc.t3 + a4 * tc.t4,
                s_d=a1 + 2.0 * a2 * tc.t + 3.0 * a3 * tc.t2 + 4.0 * a4 * tc.t3,
                s_dd=2.0 * a2 + 6.0 * a3 * tc.t + 12.0 * a4 * tc.t2, s_ddd=6.0 * a3 + 24.0 * a4 * tc.t))
        return out

    def _build_lateral_profiles(self, frenet_state, lateral_offsets, time: float, time_cache) -> list:
        """frenet_planner.py:660-701: one quintic per lateral target (d, d', d'' from the state; d(T) = di,
        d'(T) = d''(T) = 0)."""
        tc = time_cache
        a0, a1, a2 = frenet_state.d, frenet_state.d_d, frenet_state.d_dd / 2.0
        out = []
        for di in np.asarray(lateral_offsets, dtype=float):
            a3, a4, a5 = tc.quintic_A_inv @ np.array([di - a0 - a1 * time - a2 * time * time, -a1 - 2.0 * a2 * time,
                                                      -2.0 * a2])
            out.append(LateralProfile(
                d=a0 + a1 * tc.t + a2 * tc.t2 + a3 * tc.t3 + a4 * tc.t4 + a5 * tc.t5,
                d_d=a1 + 2.0 * a2 * tc.t + 3.0 * a3 * tc.t2 + 4.0 * a4 * tc.t3 + 5.0 * a5 * tc.t4,
                d_dd=2.0 * a2 + 6.0 * a3 * tc.t + 12.0 * a4 * tc.t2 + 20.0 * a5 * tc.t3,
                d_ddd=6.0 * a3 + 24.0 * a4 * tc.t + 60.0 * a5 * tc.t2))
        return out

    def _lattice_from(self, frenet_state, target_speed):
        fs = frenet_state
        req = PlanRequest(float(fs.s), float(fs.s_d), float(fs.s_dd), float(fs.d), float(fs.d_d),
                          target_speed=float(target_speed), last_kappa=float(fs.d_dd), is_frenet=True)
        self._engine.plan_batch([req])
        cost, _status, keep, _nt = self._engine.candidates(0)
        return cost, keep

    def _generate_frenet_paths(self, frenet_state, target_speed: float) -> List[FrenetPath]:
        """Every candidate of the lattice (grid, then the brake ladder) with its Frenet arrays and cost
        (frenet_planner.py:376-451); the Cartesian arrays are filled in by ``_calc_global_paths``."""
        cost, keep = self._lattice_from(frenet_state, target_speed)
        paths = []
        for i in range(len(cost)):
            full = self._engine.candidate_path(i)
            fp = FrenetPath(**{f: getattr(full, f) for f in self._FRENET_FIELDS})
            fp.cost = float(cost[i])
            fp.__dict__["_fot_global"] = ({f: getattr(full, f) for f in self._CART_FIELDS}, int(keep[i]))
            paths.append(fp)
        return paths

    def _generate_brake_candidates(self, frenet_state, target_speed: float) -> List[FrenetPath]:
        """The brake-ladder candidates alone (frenet_planner.py:453-503): the tail of the generation order; none
        below BRAKE_MIN_SPEED."""
        standing = FrenetState(frenet_state.s, 0.0, frenet_state.s_dd, frenet_state.d, frenet_state.d_d,
                               frenet_state.d_dd)
        n_grid = len(self._lattice_from(standing, target_speed)[0])          # (no ladder from a standing start)
        return self._generate_frenet_paths(frenet_state, target_speed)[n_grid:]

    def _calc_global_paths(self, fp_list: List[FrenetPath]) -> List[FrenetPath]:
        """Cartesian arrays of candidates made by ``_generate_frenet_paths``, cut to the valid prefix in lockstep
        with the Frenet arrays (frenet_planner.py:736-889: out-of-domain tail dropped, fewer than two samples or a
        singular point empty the path)."""
        for fp in fp_list:
            cart, keep = fp.__dict__["_fot_global"]
            for f in self._CART_FIELDS:
                setattr(fp, f, list(cart[f][:keep]))
            for f in self._FRENET_FIELDS:
                setattr(fp, f, list(getattr(fp, f)[:keep]))
        return fp_list

    def _path_collision_geometry(self, fp, dynamic_margin_inflation: float = 1.0):
        """(path_points, path_t, path_min, path_max, sq_rubicon, sq_rubicon_dyn) as the reference's tests read them
        (frenet_planner.py:1126-1179): one point per footprint circle and sample, the squared radii, the box.  A view
        for tests -- the kernels derive these points in registers."""
        n = min(len(fp.x), len(fp.t))
        if len(fp.x) == 0:
            return None
        pts = np.stack([np.asarray(fp.x[:n], float), np.asarray(fp.y[:n], float)], axis=1)
        t = np.asarray(fp.t[:n], float)
        radius = self.robot_radius
        if self.footprint is not None:
            radius = self.footprint.radius
            yaw = np.asarray(fp.yaw[:n], float)
            if len(yaw) < n:
                yaw = np.concatenate([yaw, np.full(n - len(yaw), yaw[-1] if len(yaw) else 0.0)])
            heading = np.stack([np.cos(yaw), np.sin(yaw)], axis=1)
            off = np.asarray(self.footprint.offsets, float)
            pts = (pts[None] + off[:, None, None] * heading[None]).reshape(-1, 2)
            t = np.tile(t, len(off))
        r_static = max(radius + self.obstacle_radius, 1e-6)
        r_dyn = r_static * dynamic_margin_inflation
        grow = max(r_static, r_dyn)
        return pts, t, pts.min(axis=0) - grow, pts.max(axis=0) + grow, r_static ** 2, r_dyn ** 2

    @staticmethod
    def _apply_stop_distance_filter(fp_dict: dict, max_stop_distance: float) -> None:
        """frenet_planner.py:307-324 on a categorised dict: 'ok' paths that do not come to rest within the travel
        move to 'stop_distance_error'."""
        ok, late = [], []
        for fp in fp_dict["ok"]:
            at_rest = len(fp.v) > 0 and abs(fp.v[-1]) <= 0.15                # STOP_SPEED_EPS
            travel = float(fp.s[-1] - fp.s[0]) if len(fp.s) > 0 else 0.0
            (ok if at_rest and travel <= max_stop_distance + 1e-6 else late).append(fp)
        fp_dict["ok"], fp_dict["stop_distance_error"] = ok, late

    @staticmethod
    def _select_best_path(path_dict: dict) -> Optional[FrenetPath]:
        """First minimum-cost entry of 'ok' (frenet_planner.py:1235-1259)."""
        best, best_cost = None, float("inf")
        for fp in path_dict["ok"]:
            if fp.cost < best_cost:
                best, best_cost = fp, fp.cost
        return best

    def candidate_table(self):
        """(cost, status, keep, n_t) per candidate of the last plan() call (diagnostic)."""
        return self._engine.candidates(0)
