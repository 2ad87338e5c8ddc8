"""Scenes, targets and instances of the chance-budget tests (test_chance_budget_cpu.py, test_gpu_chance_budget.py).

With a prediction distribution of S samples a candidate collides when more than max_viol = floor(eps S) DISTINCT samples
hit it anywhere along its path (frenet_planner.py:1113-1124); static obstacles stay hard constraints and the margin
inflation does not apply.  In plan() that one count passes through device-only code: k_cull's sample id j / P through a
host-built reciprocal, the 64-bit hit mask and the counter of FusedSink<false>, the per-segment masks of
k_evaluate_split that wave 0 folds by popcount(OR), the reload of the per-step values past step 64, the circle loop of
a footprint, the lean / general choice of a launch.  The instances here count on purpose: every hit is an obstacle row
0.5 R from a (candidate, step, circle) point of the ORACLE's lattice -- deep inside the radius, the test is about the
count and not about the radius -- in exactly as many distinct samples as the budget allows (pattern A), one more (B), or
the allowed number repeated over steps, pedestrians and circles (C); every other row of every track sits 5 km away.

All obstacle coordinates are float32 values held in float64 arrays, so one oracle run serves both tensor dtypes.  A
placement keeps every (candidate, step, circle) point of the whole lattice at |d^2 / R^2 - 1| >= CLEARANCE from every row
that step reads (a hit that does not is turned by ROTATE about its point until it does): no decision near the radius,
so the library's table must EQUAL the oracle's.  Nothing is taken from the code under test; importing this module loads
no GPU library.
"""
import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from check_paths_common import eps_pairs
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PlanRequest
from integrated_path_planning_amd.footprint import EgoFootprint
from oracle import oracle as orc
from oracle.check import oracle_plan_for_request
from test_gpu_collision_boundary import FAR, LENIENT, SCENES
from test_gpu_cull_stream import _f32

SCENE_NAMES = ("straight", "long", "arc30")
FOOTPRINTS = {"arc30": EgoFootprint.multi_circle(4.6, 1.9, 3)}
CLEARANCE = 1e-6                  # the floor test_gpu_collision_boundary.py asserts between library and oracle points
ROTATE = 0.7                      # [rad] a placement that misses CLEARANCE is turned by this about its point, up to 8 times
DEPTH = 0.5                       # a hit sits DEPTH R from its point
P = 2                             # pedestrians per sample
PREFERRED_IDS = (0, 32, 31, 33, 63)
EXTRA_PAIR = (0.1, 33)            # the pair of patterns D, E, F
GROUPS = ("A", "B", "C", "extra")


def pairs():
    """(eps, S); max_viol = floor(eps S) in float64, as the reference computes it."""
    below, above = eps_pairs()[:2]
    return [(0.0, 1), (1.0, 1), (0.5, 2), (0.1, 20), (0.1, 31), (0.1, 32), (0.1, 33), (0.05, 63), (0.05, 64), (0.5, 64),
            (63.0 / 64.0, 64), (1.0, 64), below, above, (0.58, 50), (0.02, 50)]


def max_viol(eps, S):
    return int(np.floor(eps * S))


def pair_facts():
    """What the hand-picked pairs are there for (asserted by the CPU test)."""
    below, above = eps_pairs()[:2]
    assert below[0] * below[1] < round(below[0] * below[1]) and above[0] * above[1] > round(above[0] * above[1])
    assert max_viol(*below) == round(below[0] * below[1]) - 1 and max_viol(*above) == round(above[0] * above[1])
    assert max_viol(0.58, 50) == 28 and Fraction("0.58") * 50 == 29               # float64 product below the exact one
    assert max_viol(0.02, 50) == 1 and max_viol(float(np.float32(0.02)), 50) == 0   # an eps rounded to float32 loses one
    assert max_viol(63.0 / 64.0, 64) == 63 and max_viol(1.0, 64) == 64 and max_viol(0.1, 32) == max_viol(0.1, 33) == 3


def sample_ids(S):
    """The order in which hits take their samples: S - 1, 0, 32, 31, 33, 63, then the rest ascending (ids >= S dropped):
    the ends of the mask, both sides of bit 32, and every id exactly once."""
    first = list(dict.fromkeys(s for s in (S - 1,) + PREFERRED_IDS if 0 <= s < S))
    ids = first + [s for s in range(S) if s not in first]
    assert len(ids) == S and len(set(ids)) == S, (S, ids)
    return ids


@dataclass
class Instance:
    scene: str
    group: str                    # of GROUPS
    pattern: str                  # "A", "B", "C", "D", "D+static", "E", "E-twin", "F", "F-single"
    eps: float
    S: int
    inflation: float
    cand: int                     # the target candidate
    collides: bool                # what the pattern says of the target candidate
    req: PlanRequest
    hit_ids: list = field(default_factory=list)   # the samples that hit the target, in placement order
    want: object = None           # the oracle's PlanOutput with tables

    @property
    def key(self):
        """The planner configuration the instance needs beside the scene's (one scenario of a handle per key)."""
        return (self.eps, self.inflation)

    def label(self):
        return f"{self.scene} {self.pattern} eps {self.eps!r} S {self.S} max_viol {max_viol(self.eps, self.S)} cand {self.cand}"


class Scene:
    """One reference path and ego of test_gpu_collision_boundary.SCENES on the oracle alone: the obstacle-free lattice,
    every candidate's collision points, the two target candidates and their steps."""

    def __init__(self, name):
        (wx, wy), skw, (s0, off, dyaw, v, a), self.target_speed = SCENES[name]
        self.name, self.waypoints = name, (np.asarray(wx, float), np.asarray(wy, float))
        self.footprint = FOOTPRINTS.get(name)
        self.base_kw = dict(LENIENT, **skw)
        if self.footprint is None:
            self.offsets = np.zeros(1)
            self.r = self.base_kw["robot_radius"] + self.base_kw["obstacle_radius"]
        else:
            self.offsets = np.asarray(self.footprint.offsets, float)
            self.r = self.footprint.radius + self.base_kw["obstacle_radius"]
        self.sp = orc.Spline(wx, wy)
        x, y, yaw = (c[0] for c in self.sp.eval([s0])[:3])
        self.ego = (float(x - np.sin(yaw) * off), float(y + np.cos(yaw) * off), float(yaw + dyaw), float(v), float(a))
        self.n_total = int(round(self.base_kw["max_t"] / self.base_kw["dt"])) + 1
        self.free = self.oracle(self.request(), 0.0, 1.0)
        self.frenet0 = self.free.frenet0
        n = self.free.n_cand
        # [n_cand, n_total, n_circles, 2] collision points (NaN past a candidate's n_t), yaw and lateral offset per step
        self.points = np.full((n, self.n_total, len(self.offsets), 2), np.nan)
        self.yaw = np.full((n, self.n_total), np.nan)
        self.lat = np.full((n, self.n_total), np.nan)
        params = self.oracle_params(0.0, 1.0)
        for c in range(n):
            _, arr, _ = orc.candidate_path(params, self.sp, self.frenet0, self.target_speed, c)
            nt = int(self.free.cand_nt[c])
            cx, cy, cyaw = arr[9, :nt], arr[10, :nt], arr[11, :nt]
            self.points[c, :nt, :, 0] = cx[:, None] + self.offsets[None] * np.cos(cyaw)[:, None]
            self.points[c, :nt, :, 1] = cy[:, None] + self.offsets[None] * np.sin(cyaw)[:, None]
            self.yaw[c, :nt], self.lat[c, :nt] = cyaw, arr[5, :nt]
        self.cands = self.target_candidates()
        self.far = np.array([self.ego[0] + FAR, self.ego[1] - FAR])

    # ---- planner configurations -------------------------------------------------------------------------------------
    def planner_kw(self, eps, inflation):
        """Keyword arguments of a BatchPlanner / add_scenario for one (eps, inflation) of this scene."""
        kw = dict(self.base_kw, chance_epsilon=eps, collision_margin_inflation=inflation)
        if self.footprint is not None:
            kw["footprint"] = self.footprint
        return kw

    def params_kw(self, eps, inflation):
        """The same as make_params' keyword arguments (oracle.make_params, params.make_params)."""
        kw = self.planner_kw(eps, inflation)
        fp = kw.pop("footprint", None)
        if fp is not None:
            kw["footprint_offsets"], kw["footprint_radius"] = [float(o) for o in fp.offsets], float(fp.radius)
        return kw

    def oracle_params(self, eps, inflation):
        return orc.make_params(**self.params_kw(eps, inflation))

    def oracle(self, req, eps, inflation):
        return oracle_plan_for_request(orc, self.oracle_params(eps, inflation), self.sp, req, table=True)

    def request(self, **obs):
        x, y, yaw, v, a = self.ego
        return PlanRequest(x, y, yaw, v, a, target_speed=self.target_speed, **obs)

    # ---- targets ----------------------------------------------------------------------------------------------------
    def target_candidates(self):
        """The longest-horizon candidate of the grid and one brake-ladder entry (the candidates behind the grid: its
        profile ends before its tile's longest one and is held from there, so some segments of the split walk hold
        nothing but held samples of it), among those the obstacle-free lattice keeps to the collision check."""
        kw, nt = self.base_kw, self.free.cand_nt
        n_ti = int((kw["max_t"] - kw["min_t"]) / kw["dt"] + 1e-9) + 1
        n_di = 2 * int(kw["max_road_width"] / kw["d_road_w"] + 1e-9) + 1
        n_down = int(self.target_speed / kw["d_t_s"] + 1e-9)
        n_tv = n_down + 1 + (self.target_speed - n_down * kw["d_t_s"] > 1e-9)
        self.n_grid = n_ti * n_tv * n_di
        assert 0 < self.n_grid < self.free.n_cand, (self.name, self.n_grid, self.free.n_cand)
        ok = np.flatnonzero(self.free.cand_status == _abi.ST_OK)
        grid, brake = ok[ok < self.n_grid], ok[ok >= self.n_grid]
        assert len(grid), self.name
        longest = grid[nt[grid] == nt[grid].max()]
        out = [int(longest[len(longest) // 2])]
        if len(brake):
            out.append(int(brake[len(brake) // 2]))
        return out

    def steps(self, c):
        """Target steps of candidate c: 1, about n_t / 3, about 2 n_t / 3, n_t - 1; past 64 steps also 63 and 64."""
        nt = int(self.free.cand_nt[c])
        ks = [1, nt // 3, (2 * nt) // 3, nt - 1] + [k for k in (63, 64) if k < nt - 1]
        assert len(set(ks)) == len(ks) and min(ks) >= 1, (self.name, c, ks)
        return ks

    # ---- placement --------------------------------------------------------------------------------------------------
    def clearance_at(self, pos, k=None, radii=None):
        """Smallest |d^2 / R^2 - 1| between obstacle position pos and every collision point of the lattice at step k
        (None: at every step, what a static obstacle meets), over the radii given (the scene's)."""
        pts = self.points if k is None else self.points[:, k]
        d2 = ((pts - np.asarray(pos, float)) ** 2).sum(-1)
        d2 = d2[np.isfinite(d2)]
        return min(float(np.abs(d2 / (r * r) - 1.0).min()) for r in (radii or (self.r,)))

    @functools.lru_cache(maxsize=None)
    def place(self, c, k, circle, depth=DEPTH, static=False, radii=None):
        """The float32-exact position `depth` R from circle `circle` of candidate c at step k along the path normal (on
        the side the candidate is offset to), turned by ROTATE until the whole lattice keeps CLEARANCE from it."""
        p, yaw = self.points[c, k, circle], self.yaw[c, k]
        side = 1.0 if self.lat[c, k] >= 0.0 else -1.0
        for turn in range(8):
            th = yaw + side * (0.5 * np.pi + turn * ROTATE)
            pos = _f32(p + depth * self.r * np.array([np.cos(th), np.sin(th)]))
            if self.clearance_at(pos, None if static else k, radii) >= CLEARANCE:
                return pos
        raise AssertionError(f"{self.name}: no clear placement at cand {c} step {k} circle {circle}")

    def far_tensor(self, S, n_ped=P):
        """[S, n_ped, n_total, 2] with every row about 5 km from the ego, no two rows alike."""
        t = np.zeros((S, n_ped, self.n_total, 2)) + self.far
        t += np.arange(self.n_total)[None, None, :, None] * 0.01
        t[..., 0] += np.arange(n_ped)[None, :, None] * 7.0
        t[..., 1] += np.arange(S)[:, None, None] * 3.0
        return _f32(t)


# ---- patterns -------------------------------------------------------------------------------------------------------

def _hits(sc, c, S, n_hit, spread):
    """The distribution in which the first n_hit samples of sample_ids(S) hit candidate c: hit j at target step j mod
    n_steps, pedestrian j mod P, circle j mod n_circles.  spread: every hitting sample also hits at all other target
    steps, through both pedestrians and going round the circles."""
    steps, n_c = sc.steps(c), len(sc.offsets)
    ids = sample_ids(S)[:n_hit]
    d = sc.far_tensor(S)
    for j, s in enumerate(ids):
        d[s, j % P, steps[j % len(steps)]] = sc.place(c, steps[j % len(steps)], j % n_c)
        if spread:
            for q, k in enumerate(steps):
                for ped in range(P):
                    d[s, ped, k] = sc.place(c, k, (j + q + ped) % n_c)
    return d, ids


def _instance(sc, group, pattern, eps, S, c, collides, inflation=1.0, hit_ids=(), **obs):
    return Instance(sc.name, group, pattern, eps, S, inflation, c, collides, sc.request(**obs), list(hit_ids))


def pattern_instances(sc):
    """A, B and C for every (eps, S) pair and target candidate (B skipped where max_viol + 1 > S)."""
    out = []
    for eps, S in pairs():
        m = max_viol(eps, S)
        for c in sc.cands:
            d, ids = _hits(sc, c, S, m, False)
            out.append(_instance(sc, "A", "A", eps, S, c, False, hit_ids=ids, dist=d))
            if m + 1 <= S:
                d, ids = _hits(sc, c, S, m + 1, False)
                out.append(_instance(sc, "B", "B", eps, S, c, True, hit_ids=ids, dist=d))
            d, ids = _hits(sc, c, S, m, True)
            out.append(_instance(sc, "C", "C", eps, S, c, False, hit_ids=ids, dist=d))
    return out


def extra_instances(sc):
    """D, E, F once per scene, at EXTRA_PAIR on the scene's first target candidate."""
    eps, S = EXTRA_PAIR
    m, c = max_viol(eps, S), sc.cands[0]
    steps = sc.steps(c)
    out = []
    # D: with eps = 1 every sample may hit; a static point is never forgiven
    d, ids = _hits(sc, c, S, S, False)
    out.append(_instance(sc, "extra", "D", 1.0, S, c, False, hit_ids=ids, dist=d))
    st = sc.place(c, steps[1], 0, static=True)[None].copy()
    out.append(_instance(sc, "extra", "D+static", 1.0, S, c, True, hit_ids=ids, dist=d, static=st))
    # E: a NaN forgives the track it is in (frenet_planner.py:1211-1219) and no other
    d, ids = _hits(sc, c, S, m + 1, False)
    nan_row = next(k for k in range(2, sc.n_total) if k not in steps)
    j = 1                                            # the second hit: sample ids[1] = 0 through pedestrian 1
    e = d.copy()
    e[ids[j], j % P, nan_row, 1] = np.nan
    out.append(_instance(sc, "extra", "E", eps, S, c, False, hit_ids=ids, dist=e))
    e = d.copy()
    e[ids[j], (j + 1) % P, nan_row, 0] = np.nan
    out.append(_instance(sc, "extra", "E-twin", eps, S, c, True, hit_ids=ids, dist=e))
    # F: the margin inflation applies to a single sample only
    infl = 1.2
    k = steps[2]
    pos = sc.place(c, k, 0, depth=1.1, radii=(sc.r, sc.r * infl))
    d = sc.far_tensor(S)
    d[:, 0, k] = pos
    out.append(_instance(sc, "extra", "F", 0.0, S, c, False, inflation=infl, hit_ids=list(range(S)), dist=d))
    out.append(_instance(sc, "extra", "F-single", 0.0, 1, c, True, inflation=infl, hit_ids=[0], dyn=d[0].copy()))
    return out


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(name)


@functools.lru_cache(maxsize=None)
def instances(name):
    """Every instance of a scene with the oracle's plan (computed once; shared by every test and left unchanged)."""
    sc = scene(name)
    out = pattern_instances(sc) + extra_instances(sc)
    for inst in out:
        inst.want = sc.oracle(inst.req, inst.eps, inst.inflation)
        for a in (inst.req.static, inst.req.dyn, inst.req.dist):
            if a is not None:
                a.setflags(write=False)
    return tuple(out)


def configurations(insts):
    """The distinct (eps, inflation) of a scene's instances, in order of first use: the scenarios of its handle."""
    return list(dict.fromkeys(i.key for i in insts))


# ---- the clearance of an instance, independent of place() -------------------------------------------------------------

def instance_clearance(sc, inst):
    """Smallest |d^2 / R^2 - 1| over every candidate of the lattice, every step and circle and every obstacle row that
    step reads (step k reads row min(k, T - 1) of every track; a static point is read by every step), at every radius
    the instance's mode applies.  Rows beyond 1 km from the ego are only held to that distance (asserted)."""
    radii = (sc.r, sc.r * inst.inflation) if inst.req.dyn is not None else (sc.r,)
    ego = np.array(sc.ego[:2])
    reach = np.nanmax(np.abs(sc.points - ego))
    assert reach < 500.0, (sc.name, reach)
    worst = np.inf
    if inst.req.static is not None:
        for pos in np.asarray(inst.req.static).reshape(-1, 2):
            worst = min(worst, sc.clearance_at(pos, None, radii))
    tracks = inst.req.dist if inst.req.dist is not None else (None if inst.req.dyn is None else inst.req.dyn[None])
    if tracks is not None:
        tracks = np.asarray(tracks)
        T = tracks.shape[2]
        for k in range(sc.n_total):
            rows = tracks[:, :, min(k, T - 1)].reshape(-1, 2)
            rows = rows[np.isfinite(rows).all(1)]
            near = rows[np.abs(rows - ego).max(1) < 1000.0]
            for pos in np.unique(near, axis=0):
                worst = min(worst, sc.clearance_at(pos, k, radii))
    return worst
