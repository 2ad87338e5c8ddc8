"""Cases and premises of the selection tests (test_selection_ties_cpu.py, test_gpu_selection_ties.py).

plan() ends in the reference's `if cost < min_cost` over the 'ok' candidates in generation order: the FIRST minimum
wins, and a candidate whose cost is not below +inf is never picked.  On the device that rule is a parallel arg-min in
four places (csrc/fot_kernels.hip tile_results, tile_done, select_instance_wave and the evaluation kernels' tile
order); with generic costs no two candidates ever share the minimum and none of it is exercised.  Here the weights are
chosen so that many candidates hold the minimal cost BIT FOR BIT, by construction and not by luck:

  zero      k_j = k_t = k_d = k_s_dot = 0: every cost is a sum of products with zero -- every 'ok' candidate ties
  k_t       only k_t: the cost is (k_lat + k_lon) k_t T, one value per horizon -- the 'ok' candidates of the first
            horizon that has one tie
  k_t_neg   a negative k_t: the same with the LAST horizon, i.e. the last tiles and the first-launched group
  k_s_dot   k_s_dot, and a k_t a hundred times smaller: (target - s_d(T))^2 is shared by the candidates of one
            longitudinal profile (all lateral offsets) -- the 'ok' offsets of the first horizon's profile that ends
            at the target speed tie.  (With k_s_dot ALONE the oracle's cost is exactly 0 on that profile of several
            horizons at once, s_d(T) happening to round to the target; that is luck, not construction, and the device,
            which contracts the quartic into fused multiply-adds, measured 1.0e-30 on one of them: the class was
            replaced by this one, whose k_t term separates the horizons by 2 k_t dt >> 1e-30.)
  k_d       only k_d (and k_j), k_lon = 0, the ego on the path's first waypoint with yaw 0 so that the oracle's
            frenet0[3:6] is exactly 0 (asserted): the centre candidates' lateral quintic is identically zero, their cost
            exactly 0 on every horizon, and +d / -d mirror each other
  inf       k_t = 1e308, k_lat = 10: every cost overflows to +inf -- nothing may be selected
  nan       k_t = 1e308, k_lat = 0: 0 * inf, every cost NaN -- nothing may be selected
  mixed     k_t = 1e308, k_lat = k_lon = 0.5 on horizons 1.5 .. 2.1 s: k_t T is finite below 1.797 s, +inf above

Which candidates are 'ok' -- and with it WHERE the first minimum sits -- is moved by per-instance overrides (max_accel
against an ego faster than every terminal speed rejects the short horizons; max_curvature rejects the outer lateral
offsets), static walls along one side of the road, max_stop_distance (only candidates that end standing within the
distance remain: the brake ladder alone, where it is short) and standing or slow egos (no ladder).  Where the winner
sits -- tile, lane, group under either cut of the lattice -- is read from the tile tables of the shared host builder
(tests/emu/fot_select_emu.cpp emu_tile_tables), never guessed; premises() computes it from the ORACLE's tables alone and
both test files assert it, so a case that no longer reaches its place fails on the CPU.

Nothing here is taken from the code under test except the tile tables (host code, itself checked by
test_emu_logic.test_tile_tables_*).
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np

from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PlanRequest
from integrated_path_planning_amd.params import make_params
from oracle import oracle as orc
from oracle.check import oracle_plan_for_request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
SELECT_SRC = os.path.join(EMU_DIR, "fot_select_emu.cpp")
SELECT_DEPS = [SELECT_SRC, os.path.join(ROOT, "include", "fot.h")] + [os.path.join(CSRC, f) for f in
                                                                      ("fot_math.hpp", "fot_setup.hpp", "fot_types.h")]
WAVE = 64

# -- lattices ---------------------------------------------------------------------------------------------------------
# limits wide enough that a rejection is the instance's own doing (overrides, walls, stop distance)
WIDE = dict(max_speed=30.0, max_accel=40.0, max_curvature=20.0, max_lat_accel=200.0, robot_radius=0.3,
            obstacle_radius=0.1)
LATTICES = {
    # 11 horizons x n_tv x 9 offsets + 3 ladder entries
    "small": dict(WIDE, dt=0.1, min_t=2.0, max_t=3.0, d_t_s=0.5, max_road_width=2.0, d_road_w=0.5),
    # 2 horizons x 2 x 9 + 1 ladder entry: the whole lattice in one tile under either cut
    "tile": dict(WIDE, dt=0.25, min_t=1.0, max_t=1.25, d_t_s=1.0, max_road_width=2.0, d_road_w=0.5),
    # 41 horizons x 8 x 15 + 1: 4921 candidates at 7 m/s -- more than 64 tiles in the selecting wave's strided loop
    "big": dict(WIDE, dt=0.1, min_t=1.0, max_t=5.0, d_t_s=1.0, max_road_width=3.5, d_road_w=0.5),
    # the same with 29 offsets: more than 128 tiles, so that tiles t and t + 64 can both lie at or behind a winner in
    # the second round of the strided loop (tile >= 64)
    "huge": dict(WIDE, dt=0.1, min_t=1.0, max_t=5.0, d_t_s=1.0, max_road_width=3.5, d_road_w=0.25),
    # 65 samples per candidate: the general form, and two rounds of the selected path's sample loop
    "n65": dict(WIDE, dt=0.05, min_t=3.0, max_t=3.2, d_t_s=1.0, max_road_width=1.5, d_road_w=0.5),
    # horizons 1.5 .. 2.1 s around the overflow of 1e308 * T at 1.797 s
    "around179": dict(WIDE, dt=0.1, min_t=1.5, max_t=2.1, d_t_s=1.0, max_road_width=1.0, d_road_w=0.5),
}
ZERO = dict(k_j=0.0, k_t=0.0, k_d=0.0, k_s_dot=0.0, k_lat=1.0, k_lon=1.0)
WEIGHTS = {
    "zero": ZERO,
    "k_t": dict(ZERO, k_t=0.7),
    "k_t_neg": dict(ZERO, k_t=-0.7),
    "k_s_dot": dict(ZERO, k_s_dot=1.3, k_t=0.013),
    "k_d": dict(ZERO, k_d=1.0, k_j=0.1, k_lon=0.0),
    "inf": dict(ZERO, k_t=1e308, k_lat=10.0),
    "nan": dict(ZERO, k_t=1e308, k_lat=0.0),
    "mixed": dict(ZERO, k_t=1e308, k_lat=0.5, k_lon=0.5),
    "default": dict(k_j=0.1, k_t=0.1, k_d=1.0, k_s_dot=1.0, k_lat=1.0, k_lon=1.0),
}
NONFINITE = ("inf", "nan", "mixed")

STRAIGHT = (np.linspace(0.0, 120.0, 25), np.zeros(25))


def wall(d, s0=0.0, s1=60.0, step=0.25):
    """Static points along the straight path at lateral offset d."""
    s = np.arange(s0, s1, step)
    return np.stack([s, np.full_like(s, d)], axis=1)


# -- the select emulation ----------------------------------------------------------------------------------------------
def build_select(tag, flags, main=False):
    """tests/emu/fot_select_emu.cpp as a shared object, or (main) as the program of its own."""
    out = os.path.join(EMU_DIR, "_build", ("fot_select_emu_" + tag) if main else ("libfot_select_emu_" + tag + ".so"))
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in SELECT_DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        how = ["-DFOT_SELECT_EMU_MAIN"] if main else ["-fPIC", "-shared"]
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, *how, "-o", out, SELECT_SRC], check=True)
    return out


class SelectEmu:
    def __init__(self):
        L = self.L = C.CDLL(build_select("o2", ["-O2"]))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L.emu_tile_tables.argtypes = [C.POINTER(_abi.Params), C.c_int, C.c_int, C.c_int, ip, ip]
        L.emu_select_entries.argtypes = [C.c_int, ip, dp, ip, dp, ip]
        L.emu_merge_butterfly.argtypes = [dp, ip, dp, ip]
        L.emu_merge_strided.argtypes = [C.c_int, dp, ip, ip, dp, ip, ip]
        L.emu_merge_serial.argtypes = [C.c_int, dp, ip, ip, dp, ip]
        self.group_tiles = int(L.emu_group_tiles())
        self._tables = {}

    def tile_tables(self, kw, n_tv, grouped):
        """(cand0 [n_tiles], n [n_tiles]) of the lattice of planner kwargs kw at n_tv terminal speeds, either cut."""
        key = (tuple(sorted((k, v) for k, v in kw.items() if not k.startswith("k_"))), n_tv, bool(grouped))
        if key not in self._tables:
            cap = 4096
            c0, n = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            ip = C.POINTER(C.c_int32)
            params = make_params(**kw)
            nt = self.L.emu_tile_tables(C.byref(params), n_tv, int(grouped), cap, c0.ctypes.data_as(ip), n.ctypes.data_as(ip))
            assert nt > 0, nt
            self._tables[key] = (c0[:nt].copy(), n[:nt].copy())
        return self._tables[key]

    @staticmethod
    def _d(a):
        return a.ctypes.data_as(C.POINTER(C.c_double))

    @staticmethod
    def _i(a):
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    def entries(self, status, cost, index):
        status, index = (np.ascontiguousarray(a, np.int32) for a in (status, index))
        cost = np.ascontiguousarray(cost, np.float64)
        ec, ei = np.zeros(len(cost)), np.zeros(len(cost), np.int32)
        self.L.emu_select_entries(len(cost), self._i(status), self._d(cost), self._i(index), self._d(ec), self._i(ei))
        return ec, ei

    def butterfly(self, cost, idx):
        """(cost [64], idx [64]) the result in every slot."""
        cost, idx = np.ascontiguousarray(cost, np.float64), np.ascontiguousarray(idx, np.int32)
        assert len(cost) == len(idx) == WAVE
        oc, oi = np.zeros(WAVE), np.zeros(WAVE, np.int32)
        self.L.emu_merge_butterfly(self._d(cost), self._i(idx), self._d(oc), self._i(oi))
        return oc, oi

    def strided(self, cost, idx, keep):
        cost = np.ascontiguousarray(cost, np.float64)
        idx, keep = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(keep, np.int32)
        oc, oi, ok = C.c_double(0.0), C.c_int32(0), C.c_int32(0)
        differ = self.L.emu_merge_strided(len(cost), self._d(cost), self._i(idx), self._i(keep), C.byref(oc), C.byref(oi),
                                          C.byref(ok))
        return differ, oc.value, oi.value, ok.value

    def serial(self, cost, idx, perm):
        cost = np.ascontiguousarray(cost, np.float64)
        idx, perm = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(perm, np.int32)
        oc, oi = C.c_double(0.0), C.c_int32(0)
        self.L.emu_merge_serial(len(cost), self._d(cost), self._i(idx), self._i(perm), C.byref(oc), C.byref(oi))
        return oc.value, oi.value


# -- cases -------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    lattice: str
    weights: str
    reqs: list                                   # [PlanRequest]
    tied_min: int = 8                            # every instance with a path: at least this many tied 'ok' candidates
    waypoints: tuple = STRAIGHT
    wants: list = field(default_factory=list)    # the oracle's PlanOutput with tables, per instance

    @property
    def kw(self):
        return dict(LATTICES[self.lattice], **WEIGHTS[self.weights])

    @property
    def n_total(self):
        return int(round(self.kw["max_t"] / self.kw["dt"])) + 1

    @property
    def nonfinite(self):
        return self.weights in NONFINITE

    def label(self, i=None):
        return f"{self.name} [{self.lattice}, {self.weights}]" + ("" if i is None else f" inst {i}")


def n_tv_of(kw, target_speed):
    n_down = int(target_speed / kw["d_t_s"] + 1e-9)
    return n_down + 1 + (target_speed - n_down * kw["d_t_s"] > 1e-9)


def ego(v, target, **kw):
    """An ego on the straight path's first waypoint, yaw 0: the oracle's frenet0[3:6] is exactly 0."""
    return PlanRequest(0.0, 0.0, 0.0, v, 0.0, target_speed=target, **kw)


def off_ego(v, target, **kw):
    """A generic ego: off the path, turned, accelerating."""
    return PlanRequest(3.1, 0.23, 0.04, v, 0.3, target_speed=target, **kw)


def left_ego(v, target, **kw):
    """An ego 2 m left of the path with a wall at 1.5 m: only the candidates that stay on the outermost offset (the
    LAST of each profile's nine) clear it."""
    return PlanRequest(3.1, 2.0, 0.0, v, 0.0, target_speed=target, static=wall(1.5), **kw)


def _accel(limits, make=off_ego, v=9.0, target=6.0, **kw):
    # an ego faster than every terminal speed: the peak deceleration to the nearest one falls with the horizon, so a
    # max_accel override rejects every horizon below one of its choosing (and every terminal speed but the first)
    return [make(v, target, overrides=dict(max_accel=a), **kw) for a in limits]


def make_cases():
    cases = [
        Case("plain egos", "small", "zero", [off_ego(5.0, 6.0), off_ego(2.0, 6.0), ego(6.0, 6.0)]),
        Case("short horizons rejected by max_accel", "small", "zero", _accel((2.4, 2.1, 1.9, 1.75, 1.65))),
        Case("walls on the right, outer offsets rejected by max_curvature", "small", "zero",
             [off_ego(9.0, 6.0, overrides=dict(max_accel=a), static=wall(d)) for a, d in
              ((2.1, -1.6), (1.9, -1.1), (1.75, -0.6))]
             + [off_ego(5.0, 6.0, overrides=dict(max_curvature=c)) for c in (0.05, 0.1)]),
        Case("wall on the left: the last offset of a profile", "small", "zero", _accel((40.0, 2.2, 2.1, 2.04), left_ego)),
        Case("ladder only", "small", "zero",
             [ego(4.0, 6.0, max_stop_distance=3.5, overrides=dict(max_accel=a)) for a in (5.0, 7.0, 12.0)], tied_min=1),
        Case("stop filter keeps the standing ends", "small", "zero",
             [off_ego(4.0, 6.0, max_stop_distance=m) for m in (6.0, 8.0)], tied_min=5),
        Case("first horizon ties", "small", "k_t", [off_ego(5.0, 6.0), off_ego(2.0, 4.0), ego(6.0, 6.0, static=wall(-1.1))]),
        Case("last horizon ties", "small", "k_t_neg", [off_ego(5.0, 6.0), off_ego(2.0, 4.0), ego(0.0, 3.0)], tied_min=7),
        Case("one profile ties", "small", "k_s_dot",
             [off_ego(5.0, 6.0), off_ego(2.0, 4.0), ego(6.0, 6.0), off_ego(5.0, 6.0, static=wall(-1.1))]
             + _accel((1.9,)), tied_min=6),
        Case("centre candidates tie on every horizon", "small", "k_d", [ego(5.0, 6.0), ego(2.0, 4.0), ego(0.0, 3.0)]),
        Case("one tile", "tile", "zero", [off_ego(1.5, 1.0), ego(0.0, 1.0), off_ego(1.5, 1.0, static=wall(-0.7))]),
        Case("one tile, last horizon", "tile", "k_t_neg", [off_ego(1.5, 1.0), ego(0.0, 1.0)]),
        Case("65 samples", "n65", "zero", [off_ego(5.0, 3.0), ego(0.0, 3.0), off_ego(6.0, 3.0, overrides=dict(max_accel=2.0))]),
        Case("65 samples, last horizon", "n65", "k_t_neg", [off_ego(5.0, 3.0), ego(0.0, 3.0)], tied_min=6),
        Case("4921 candidates", "big", "zero",
             [off_ego(5.0, 7.0), off_ego(10.0, 7.0, overrides=dict(max_accel=1.2)), ego(0.0, 7.0)]),
        Case("4921 candidates, last horizon", "big", "k_t_neg", [off_ego(5.0, 7.0), off_ego(2.0, 7.0)]),
        Case("9513 candidates, winner behind tile 64", "huge", "zero", _accel((2.25,), v=11.0, target=7.0)),
        Case("every cost +inf", "small", "inf", [off_ego(5.0, 6.0), ego(0.0, 3.0)]),
        Case("every cost NaN", "small", "nan", [off_ego(5.0, 6.0), ego(0.0, 3.0)]),
        Case("finite below 1.797 s, +inf above", "around179", "mixed",
             [off_ego(3.0, 3.0), ego(0.0, 2.0), off_ego(6.0, 3.0, overrides=dict(max_accel=2.5))], tied_min=3),
        Case("4921 candidates, every cost +inf", "big", "inf", [off_ego(5.0, 7.0)]),
    ]
    for c in cases:
        params, sp = orc.make_params(**c.kw), orc.Spline(*c.waypoints)
        c.wants = [oracle_plan_for_request(orc, params, sp, r, table=True) for r in c.reqs]
    return cases


_CASES = None


def cases():
    """The cases with the oracle's outputs, computed once and shared (left unchanged by the tests)."""
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
    return _CASES


# -- premises ----------------------------------------------------------------------------------------------------------
def reference_select(status, cost):
    """The reference's loop (frenet_planner.py:1254-1257) over a candidate table: the first strict minimum below +inf
    among the 'ok' candidates in ascending index order; -1 without one."""
    best, best_cost = -1, np.inf
    for i in np.flatnonzero(np.asarray(status) == _abi.ST_OK):
        if cost[i] < best_cost:
            best, best_cost = int(i), cost[i]
    return best, best_cost


def place(tables, index):
    """(tile, lane, n of the tile) of a candidate index under a cut's tile table."""
    c0, n = tables
    t = int(np.flatnonzero((c0 <= index) & (index < c0 + n))[0])
    return t, int(index - c0[t]), int(n[t])


def tile_parts(tables, status, cost, keep):
    """Per tile what tile_results leaves, from a candidate table: (cost, idx, keep) of its first minimum; idx -1: none."""
    c0, n = tables
    out = []
    for t in range(len(c0)):
        hi = min(int(c0[t] + n[t]), len(status))
        lo = min(int(c0[t]), hi)
        b, bc = reference_select(status[lo:hi], cost[lo:hi])
        out.append((bc, lo + b, int(keep[lo + b])) if b >= 0 else (np.inf, -1, 0))
    return out


def premises(case, emu):
    """Per instance, from the ORACLE's tables and the tile tables alone: a dict of
    winner, tied (indices of the 'ok' candidates that hold the winner's cost bit for bit), n_tied, and per cut
    ("wave", "group"): tile, lane, last_lane (the winner on the tile's last occupied lane), n_tiles, tiles of the tied
    set; group / n_groups (grouped cut); ladder (the winner is a brake-ladder entry and no lattice candidate is 'ok');
    lowest_not_ok (the lowest index holding the winner's cost is not 'ok'); keep_differs (a candidate of a lower index
    with the winner's cost has another keep); lane0_keep_differs (what lane 0 of the selecting wave holds for keep is
    not the winner's); spans64 (tiles t and t + 64 both hold tied candidates)."""
    out = []
    for req, w in zip(case.reqs, case.wants):
        kw = case.kw
        n_tv = n_tv_of(kw, req.target_speed)
        n_di = 2 * int(kw["max_road_width"] / kw["d_road_w"] + 1e-9) + 1
        n_ti = int((kw["max_t"] - kw["min_t"]) / kw["dt"] + 1e-9) + 1
        n_grid = n_ti * n_tv * n_di
        status, cost, keep = w.cand_status, w.cand_cost, w.cand_keep
        ok = status == _abi.ST_OK
        best, best_cost = reference_select(status, cost)
        p = dict(winner=best, n_cand=int(w.n_cand), n_ok=int(ok.sum()), n_grid=n_grid, n_tv=n_tv,
                 finite_ok=int((ok & (cost < np.inf)).sum()))
        assert best == w.best_index, (case.label(), best, w.best_index)
        if best < 0:
            p.update(tied=np.zeros(0, int), n_tied=0)
            out.append(p)
            continue
        same = np.array([np.float64(c).tobytes() == np.float64(best_cost).tobytes() for c in cost])
        tied = np.flatnonzero(ok & same)
        holders = np.flatnonzero(same)
        p.update(tied=tied, n_tied=len(tied), keep=int(keep[best]),
                 ladder=bool(best >= n_grid and not ok[:n_grid].any()),
                 lowest_not_ok=bool(holders[0] < best),
                 keep_differs=bool(np.any(keep[holders[holders < best]] != keep[best])),
                 keeps_in_tied=len(set(keep[tied].tolist())))
        for cut, grouped in (("wave", False), ("group", True)):
            tab = emu.tile_tables(kw, n_tv, grouped)
            t, lane, n = place(tab, best)
            last_occupied = min(n, w.n_cand - int(tab[0][t])) - 1
            tiles = sorted({place(tab, int(i))[0] for i in tied})
            real = [i for i in range(len(tab[0])) if tab[1][i] > 0 and tab[0][i] < w.n_cand]
            parts = tile_parts(tab, status, cost, keep)
            lane0 = (np.inf, -1, 0)
            for tt in range(0, len(parts), WAVE):                       # what lane 0 of the selecting wave folds
                if parts[tt][1] >= 0 and (lane0[1] < 0 or parts[tt][0] < lane0[0]):
                    lane0 = parts[tt]
            p[cut] = dict(tile=t, lane=lane, last_lane=lane == last_occupied and lane > 0, n_tiles=len(tab[0]),
                          first_tile=t == real[0], last_tile=t == real[-1], tied_tiles=tiles,
                          spans64=any(a + WAVE in tiles for a in tiles),
                          lane0_keep_differs=lane0[2] != int(keep[best]))
            if grouped:
                p[cut].update(group=t // emu.group_tiles, n_groups=len(tab[0]) // emu.group_tiles,
                              last_group=t // emu.group_tiles == real[-1] // emu.group_tiles)
        out.append(p)
    return out


def describe(case, prem):
    rows = []
    for i, p in enumerate(prem):
        if p["winner"] < 0:
            rows.append(f"{case.label(i)}: no path, {p['n_ok']} ok of {p['n_cand']}, {p['finite_ok']} with a cost below +inf")
            continue
        w, g = p["wave"], p["group"]
        rows.append(f"{case.label(i)}: winner {p['winner']} of {p['n_cand']}, {p['n_tied']} tied ({p['tied'][0]} .. {p['tied'][-1]}), "
                    f"keep {p['keep']} ({p['keeps_in_tied']} distinct in the tied set); wave cut tile {w['tile']}/{w['n_tiles']} "
                    f"lane {w['lane']}{' (last)' if w['last_lane'] else ''}; grouped cut tile {g['tile']}/{g['n_tiles']} lane "
                    f"{g['lane']}{' (last)' if g['last_lane'] else ''} group {g['group']}/{g['n_groups']}"
                    f"{' ladder' if p['ladder'] else ''}{' lowest-not-ok' if p['lowest_not_ok'] else ''}"
                    f"{' keep-differs' if p['keep_differs'] else ''}{' spans64' if w['spans64'] else ''}")
    return rows


def assert_case(case, prem):
    """What every case must show by the oracle alone."""
    for i, (p, w, r) in enumerate(zip(prem, case.wants, case.reqs)):
        lab = case.label(i)
        if case.weights == "k_d":
            assert np.all(w.frenet0[3:6] == 0.0), f"{lab}: the oracle's frenet0[3:6] is {w.frenet0[3:6]!r}, not exactly 0"
        if case.weights in ("inf", "nan"):
            cost = w.cand_cost[w.cand_status == _abi.ST_OK]
            assert len(cost) >= 8 and w.status == _abi.PLAN_NO_PATH and w.best_index == -1, lab
            assert np.all(np.isnan(cost)) if case.weights == "nan" else np.all(cost == np.inf), lab
            continue
        if p["winner"] < 0:
            continue
        assert p["n_tied"] >= case.tied_min, f"{lab}: {p['n_tied']} tied 'ok' candidates"
        assert p["tied"][0] == p["winner"], lab
    if case.weights == "mixed":
        ok = [w.cand_cost[w.cand_status == _abi.ST_OK] for w in case.wants]
        assert any(np.any(c < np.inf) and np.any(c == np.inf) for c in ok), f"{case.label()}: no instance mixes finite and +inf"
        assert any(len(c) >= 8 and np.all(c == np.inf) and w.status == _abi.PLAN_NO_PATH for c, w in zip(ok, case.wants)), \
            f"{case.label()}: no instance whose 'ok' candidates all cost +inf"


def assert_shown(rows):
    """rows: [(case, premises(case))] of ALL cases -- together they show every place the selection can go wrong at."""
    flat = [(c, i, p) for c, prem in rows for i, p in enumerate(prem) if p["winner"] >= 0]
    big = [x for x in flat if x[2]["n_tied"] >= 8]
    assert len(big) >= 20, len(big)
    for cut in ("wave", "group"):
        at = lambda f, pool=big: [f"{c.label(i)}" for c, i, p in pool if f(p, p[cut])]
        assert at(lambda p, q: q["lane"] == 0 and q["tile"] > 0), f"{cut}: no winner on lane 0 of a tile behind the first"
        assert at(lambda p, q: q["last_lane"], flat), f"{cut}: no winner on the last occupied lane of a tile"
        assert at(lambda p, q: q["first_tile"]) and at(lambda p, q: q["last_tile"], flat), f"{cut}: first / last tile"
        tiles = {(c.lattice, p[cut]["tile"]) for c, i, p in big}
        assert len({t for _, t in tiles}) >= 5, f"{cut}: winners in the tiles {sorted(tiles)} only"
        assert at(lambda p, q: q["spans64"] and q["tile"] < WAVE), f"{cut}: no tied set in tiles t and t + 64"
        assert at(lambda p, q: q["spans64"] and q["tile"] >= WAVE), f"{cut}: no tied set in tiles t, t + 64 behind a winner in tile >= 64"
        assert at(lambda p, q: q["lane0_keep_differs"] and q["tile"] % WAVE != 0), f"{cut}: lane 0 of the selecting wave never holds another keep"
    groups = {(c.lattice, p["group"]["group"]) for c, i, p in big}
    assert len({g for _, g in groups}) >= 3, groups
    assert any(p["group"]["last_group"] for c, i, p in flat), "no winner in the last group"
    assert any(p["group"]["last_group"] for c, i, p in big if c.weights == "k_t_neg") or \
        any(p["group"]["group"] >= p["group"]["n_groups"] - 2 for c, i, p in big if c.weights == "k_t_neg"), "k_t_neg: not at the end"
    assert any(p["ladder"] for c, i, p in flat), "no brake-ladder winner with every lattice candidate rejected"
    assert any(p["lowest_not_ok"] for c, i, p in big), "the lowest tied index is 'ok' everywhere"
    assert any(p["keep_differs"] for c, i, p in big), "no tied candidate of a lower index with another keep"
    assert any(p["keeps_in_tied"] > 1 for c, i, p in big)
    assert {c.weights for c, _ in rows} >= set(WEIGHTS) - {"default"}, "a weight class without a case"
    assert {c.lattice for c, _ in rows} == set(LATTICES)
    assert any(c.n_total > WAVE for c, _ in rows)
