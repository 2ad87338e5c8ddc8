"""Cases of the step-bookkeeping tests (test_step_bookkeeping_cpu.py, test_gpu_step_bookkeeping.py).

The evaluation walk (csrc/fot_math.hpp evaluate_segment / check_sample) keeps three pieces of bookkeeping per time step
that the lean grouped and lean split kernels form differently from the other four (SREG): the lateral state of a
brake-ladder lane that holds (a scalar branch on the tile's ne_min, the smallest n_eval of its candidates), the first
NaN sample (keyed on its index; CK_SEEN_NAN set behind the loop) and the largest step (one v_max_f64 in every kernel).
Every case here is built so that the ORACLE's own arrays prove it reaches the branch it is about -- the counts are
asserted, not assumed -- and the expectation is the oracle's table and record under the same inputs.

  hold    ladder     a moving ego: the brake ladder is there, a tile mixes polynomial and holding lanes (ne_min < n_loop)
          all_hold   a lattice of 8 horizons x 8 speeds: the grouped cut ends on a tile of ladder candidates only, every
                     lane of which holds from some step on (as the last tile of `ladder` under either cut)
          partial    a tile of fewer than 64 candidates (lanes that walk the empty path)
          standing   a standing ego: no ladder, no lane ever holds
  nan     the ego 0.5 / 2 / 8 / 20 / 26 m before the end of the reference path: the first NaN sample of its candidates falls at
          k = 1, 2, in the middle and on the last step (keep = first_nan >= 2 ? first_nan : 0); an ego at x = NaN: k = 0; a
          tight arc that ends: a singular sample before the NaN.  (A singular sample BEHIND the first NaN does not exist
          through plan(): the NaN is the end of the reference path, and every later sample lies behind it too.)
  step    the `step` scene of tests/limit_boundaries_common.py: step_limit at (1 -+ 1e-9) of the largest step of candidates
          whose largest step is the first one (k = 1) and the last one.
A step of NaN length (CK_NANSTEP) with a valid sample needs x = +-inf twice in a row; no ego and path reach that, on the
CPU or the GPU.  tests/emu/fot_step_emu.cpp drives check_sample over such points on the host (the CPU test); on the
device the rule rests on v_max_f64 returning its other operand for a quiet NaN.
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

import limit_boundaries_common as lb
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PlanRequest
from integrated_path_planning_amd.params import make_params
from oracle import oracle as orc
from oracle.check import oracle_plan_for_request

WAVE = 64


class StepEmu(lb.Emu):
    """tests/emu/fot_step_emu.cpp: the host emulation that walks every candidate in both forms of the bookkeeping."""
    SRC = os.path.join(lb.ROOT, "tests", "emu", "fot_step_emu.cpp")
    SO = os.path.join(lb.ROOT, "tests", "emu", "_build", "libfot_step_emu.so")
    FIELDS = ("walked", "differences", "steps_direct", "steps_held", "seen_nan", "singular", "nan_step")

    def __init__(self):
        csrc = os.path.join(lb.ROOT, "integrated_path_planning_amd", "csrc")
        srcs = [self.SRC, lb.Emu.SRC, os.path.join(lb.ROOT, "include", "fot.h")] + \
               [os.path.join(csrc, f) for f in ("fot_math.hpp", "fot_setup.hpp", "fot_types.h")]
        if not os.path.exists(self.SO) or os.path.getmtime(self.SO) < max(os.path.getmtime(s) for s in srcs):
            os.makedirs(os.path.dirname(self.SO), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", self.SO, self.SRC],
                           check=True)
        super().__init__(so=self.SO)
        ip = C.POINTER(C.c_int32)
        self.L.step_tally_get.argtypes = [C.POINTER(C.c_int64), C.c_char_p]
        self.L.step_tiles.argtypes = [C.POINTER(_abi.Params), C.c_int, C.c_int, C.c_int, ip, ip]
        self.L.step_nan_step.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_double)]

    def reset(self):
        self.L.step_tally_reset()

    def tally(self):
        out, first = (C.c_int64 * 7)(), C.create_string_buffer(160)
        self.L.step_tally_get(out, first)
        return dict(zip(self.FIELDS, (int(v) for v in out)), first=first.value.decode())

    def tiles(self, kw, n_tv, grouped):
        """[(first candidate, size)] of the tiles of a lattice shape under the per-wave / grouped cut."""
        cap = 4096
        c0, n = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        ip = C.POINTER(C.c_int32)
        m = self.L.step_tiles(C.byref(make_params(**kw)), n_tv, int(grouped), cap, c0.ctypes.data_as(ip), n.ctypes.data_as(ip))
        assert 0 < m < cap, m
        return [(int(a), int(b)) for a, b in zip(c0[:m], n[:m])]

    def nan_step(self):
        fl, mx = C.c_uint32(0), (C.c_double * 5)()
        self.L.step_nan_step(C.byref(fl), mx)
        return int(fl.value), [float(v) for v in mx]


ARC_KW = dict(lb.LENIENT, **lb.ARC_KW)                      # 21 samples per candidate: the lean form is eligible
SQUARE_KW = dict(lb.LENIENT, dt=0.2, min_t=2.6, max_t=4.0, max_speed=25.0)     # 8 horizons
END_KW = dict(lb.LENIENT, dt=0.2, min_t=3.0, max_t=4.0, max_speed=25.0)
PATH_LEN = 60.0


@dataclass
class Case:
    name: str
    group: str                   # "hold", "nan", "step"
    waypoints: tuple
    kw: dict
    req: PlanRequest
    want: object = None          # the oracle's PlanOutput with tables
    info: dict = None            # per candidate, from the oracle's arrays (cand_info)

    @property
    def n_total(self):
        return int(round(self.kw["max_t"] / self.kw["dt"])) + 1


def on_path(wp, s0, off, dyaw, v, a, **kw):
    sp = orc.Spline(*wp)
    x, y, yaw = (c[0] for c in sp.eval([s0])[:3])
    return PlanRequest(float(x - np.sin(yaw) * off), float(y + np.cos(yaw) * off), float(yaw + dyaw), float(v), float(a), **kw)


def n_tv_of(kw, target_speed):
    n_down = int(target_speed / kw["d_t_s"] + 1e-9)
    return n_down + 1 + (target_speed - n_down * kw["d_t_s"] > 1e-9)


def n_grid_of(kw, target_speed):
    n_ti = int((kw["max_t"] - kw["min_t"]) / kw["dt"] + 1e-9) + 1
    n_di = 2 * int(kw["max_road_width"] / kw["d_road_w"] + 1e-9) + 1
    return n_ti * n_tv_of(kw, target_speed) * n_di


def cand_info(case):
    """Per candidate, from the oracle's arrays alone: n_t, n_eval (samples before a ladder entry holds), the first NaN
    sample (-1: none), whether a singular sample lies before it, and the step k of the largest step (-1: none)."""
    params, sp, w = orc.make_params(**case.kw), orc.Spline(*case.waypoints), case.want
    n_grid = min(n_grid_of(case.kw, case.req.target_speed), w.n_cand)
    nt_all, ne_all, fn_all, sing_all, kmax_all = [], [], [], [], []
    for c in range(w.n_cand):
        _, arr, _ = orc.candidate_path(params, sp, w.frenet0, case.req.target_speed, c)
        nt = int(w.cand_nt[c])
        ne = nt
        if c >= n_grid:
            held = np.flatnonzero((arr[lb.SD_, :nt] == 0.0) & (arr[lb.SDDD_, :nt] == 0.0) & (np.arange(nt) > 0))
            ne = int(held[0]) if len(held) else nt
        x = arr[lb.X_, :nt]
        nn = np.flatnonzero(np.isnan(x))
        fn = int(nn[0]) if len(nn) else -1
        end = fn if fn >= 0 else nt
        with np.errstate(invalid="ignore"):
            omkd = 1.0 - sp.eval(arr[lb.S_, :nt])[3] * arr[lb.D_, :nt]
            sing = bool((np.isfinite(omkd[:end]) & (omkd[:end] <= 0.05)).any())
            step = np.hypot(np.diff(x[:end]), np.diff(arr[lb.Y_, :end]))
        kmax = int(np.argmax(step)) + 1 if len(step) and not np.isnan(step).any() else -1
        nt_all.append(nt); ne_all.append(ne); fn_all.append(fn); sing_all.append(sing); kmax_all.append(kmax)
    return dict(n_grid=n_grid, n_t=np.array(nt_all), n_eval=np.array(ne_all), first_nan=np.array(fn_all),
                singular_before=np.array(sing_all), k_max_step=np.array(kmax_all))


def finish(case):
    case.want = oracle_plan_for_request(orc, orc.make_params(**case.kw), orc.Spline(*case.waypoints), case.req, table=True)
    case.info = cand_info(case)
    return case


def hold_cases():
    arc = lb.arc()
    out = [Case("ladder", "hold", arc, ARC_KW, on_path(arc, 5.0, -0.2, -0.03, 6.0, 0.8, target_speed=7.0)),
           Case("all_hold", "hold", arc, SQUARE_KW, on_path(arc, 5.0, -0.2, -0.03, 6.0, 0.8, target_speed=14.0)),
           Case("partial", "hold", arc, ARC_KW, on_path(arc, 5.0, 0.3, 0.02, 3.0, 0.2, target_speed=3.0)),
           Case("standing", "hold", arc, ARC_KW, on_path(arc, 5.0, -0.2, 0.0, 0.0, 0.0, target_speed=7.0))]
    return [finish(c) for c in out]


def tile_facts(emu, case, grouped):
    """Per tile of the instance's lattice under a cut: (lanes with a candidate, ne_min, n_loop, holding lanes)."""
    info, n_cand = case.info, case.want.n_cand
    out = []
    for c0, n in emu.tiles(case.kw, n_tv_of(case.kw, case.req.target_speed), grouped):
        c1 = min(c0 + n, n_cand)
        if c1 <= c0:
            continue
        ne, nt = info["n_eval"][c0:c1], info["n_t"][c0:c1]
        out.append((c1 - c0, int(ne.min()), int(nt.max()), int((ne < nt).sum())))
    return out


def nan_cases():
    line = lb.straight(0.4, PATH_LEN)
    out = []
    for gap in (0.5, 2.0, 8.0, 20.0, 26.0):
        out.append(Case(f"end_{gap:g}", "nan", line, END_KW, on_path(line, PATH_LEN - gap, 0.1, 0.02, 6.0, 0.3, target_speed=7.0)))
    out.append(Case("nan_ego", "nan", line, END_KW, PlanRequest(float("nan"), 1.0, 0.4, 6.0, 0.3, target_speed=7.0)))
    tight = lb.arc(radius=2.6, span=2.4)
    out.append(Case("tight_end", "nan", tight, dict(END_KW, max_road_width=3.0),
                    on_path(tight, 2.6 * 2.4 - 3.0, 2.55, 0.0, 2.0, 0.2, target_speed=3.0)))
    return [finish(c) for c in out]


NAN_REQUIRED = ("none", "k0", "k1", "k2", "middle", "last", "singular_before")


def nan_positions(cases):
    """position -> number of candidates over the cases whose first NaN sample falls there."""
    h = {"none": 0, "k0": 0, "k1": 0, "k2": 0, "middle": 0, "last": 0, "singular_before": 0, "singular_no_nan": 0}
    for case in cases:
        fn, nt = case.info["first_nan"], case.info["n_t"]
        h["none"] += int((fn < 0).sum())
        for k in (0, 1, 2):
            h[f"k{k}"] += int((fn == k).sum())
        h["last"] += int(((fn == nt - 1) & (fn > 2)).sum())
        h["middle"] += int(((fn > 2) & (fn < nt - 1)).sum())
        h["singular_before"] += int((case.info["singular_before"] & (fn >= 0)).sum())
        h["singular_no_nan"] += int((case.info["singular_before"] & (fn < 0)).sum())
    return h


def step_cases(emu):
    """Instances of the `step` scene whose step_limit sits 1e-9 below / above the largest step of a target candidate,
    the largest step being the first (k = 1) or the last one: [(Case, target, delta)]."""
    sc = lb.Scene("step", emu)
    _, paths = emu.paths(sc.kw, sc.waypoints, sc.request())
    insts, picked, _ = lb.build(sc, lambda c: paths[c], extras=False)
    out = []
    for inst in insts:
        (t, d), = inst.targets
        if abs(d) == 1e-9 and ({"k1", "last"} & set(t.cases)):
            kw = dict(sc.kw, **inst.kw)
            case = Case(f"step_c{t.c}_{'above' if d > 0 else 'below'}", "step", sc.waypoints, kw, inst.req, want=inst.want)
            case.info = cand_info(case)
            out.append((case, t, d))
    return out
