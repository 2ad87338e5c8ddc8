"""Planning against prediction distributions of 65 .. 254 samples, on the GPU.

A handle plans up to 64 samples unless its sample capacity is raised (BatchPlanner(sample_capacity=...),
fot_set_sample_capacity, at most 254).  A launch with an instance of more than 64 samples is WIDE: it runs
k_evaluate*_wide (the general form, the DISTINCT hitting samples in four mask words) or k_evaluate*_lean_wide (the lean
form, whose exact re-check never looks at a sample id), never a flat kernel; every other launch runs what it ran
before, raised capacity or not.  tests/wide_samples_common.py builds the budget instances (exactly max_viol distinct
samples hit the target: A; one more: B; max_viol samples over and over: C; sample ids on both sides of every word
edge) and tests/test_wide_samples_cpu.py proves their premises on the oracle alone, so every table here must EQUAL the
oracle's.

  1  the budget under every wide kernel: every launch shape and 2, 3, 4 time segments, "lean-wide" exactly for the
     eps S < 1 instances of the straight scene, records byte-identical across the shapes
  2  float32 tensors and the time-major layout: records byte-identical to 1's
  3  a wide instance beside instances of up to 64 samples, in one launch and in one mixed-scenario launch: every record
     byte-identical to its record alone (the narrow ones: alone on a DEFAULT handle)
  4  64 samples on a raised handle: today's kernels ("lean" / "general"), today's records
  5  the capacity itself: argument checks, a handle raised to 128, the drop-in FrenetPlanner, the external-path checkers
  6  the reference fixtures of tests/golden/wide_samples/ under every launch shape
  7  FrenetPlanner._check_collision_distribution with an epsilon of its own on a raised planner
"""
import ctypes as C
import warnings

import numpy as np
import pytest

import chance_budget_common as cb
import check_paths_common as cp
import wide_samples_common as ws
from conftest import Golden
from helpers import (EVAL_PATHS_NEVER_FLAT, TIGHT, assert_no_flat_launch, assert_record_matches_oracle, request_from_golden,
                     set_eval_path, wrap_angle)
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu

PATHS = EVAL_PATHS_NEVER_FLAT + ("wave-2", "wave-3")     # as tests/test_gpu_chance_budget.py: "split-wave" is 4 segments
CASES = [(s, p) for s in ws.SCENE_NAMES for p in ws.PATTERNS]
FIXTURES = ("dist_s100_eps0", "dist_s100_eps005", "footprint3_s130_eps01")


def set_path(bp, path):
    if path.startswith("wave-"):
        bp.set_tile_cut(1)
        bp.set_eval_segments(int(path[5:]))
        bp.set_flat(1)
    else:
        set_eval_path(bp, path)


def rec_bytes(rec):
    return bytes(memoryview(rec).cast("B"))


def check_instance(bp, res, slot, inst, how):
    """the library's candidate tables and record of instance `slot` of the last call EQUAL the oracle's"""
    lab = f"{inst.label()} [{how}]"
    want = inst.want
    cost, status, keep, nt = bp.candidates(slot)
    assert len(status) == want.n_cand, lab
    np.testing.assert_array_equal(nt, want.cand_nt, err_msg=lab)
    np.testing.assert_array_equal(keep, want.cand_keep, err_msg=lab)
    np.testing.assert_array_equal(status, want.cand_status, err_msg=lab)
    np.testing.assert_allclose(cost, want.cand_cost, rtol=TIGHT, atol=TIGHT, err_msg=lab)
    assert_record_matches_oracle(res.records[slot], want, label=lab)       # status, best_index, n_keep, stats, path
    assert int(status[inst.cand]) == (_abi.ST_COLLISION if inst.collides else _abi.ST_OK), lab


class Handle:
    """One handle per scene, capacity 254 (or as given): a scenario per distinct eps of the instances it is built for."""

    def __init__(self, name, insts, sample_capacity=_abi.MAX_PLAN_SAMPLES):
        self.sc, self.insts = ws.scene(name), list(insts)
        self.keys = cb.configurations(self.insts)
        self.bp = BatchPlanner(waypoints=self.sc.waypoints, sample_capacity=sample_capacity, **self.sc.planner_kw(*self.keys[0]))
        for k, key in enumerate(self.keys[1:], start=1):
            assert self.bp.add_scenario(waypoints=self.sc.waypoints, **self.sc.planner_kw(*key)) == k
        self.reqs = [self.req(i) for i in self.insts]

    def req(self, inst):
        return PlanRequest(**{**inst.req.__dict__, "scenario": self.keys.index(inst.key)})

    def launches(self, pattern):
        """the instances of a pattern as the launches they go out in: the lean-eligible ones, and the others"""
        idx = [i for i, inst in enumerate(self.insts) if inst.pattern == pattern]
        lean = [i for i in idx if ws.lean_eligible(self.sc, self.insts[i])]
        return [(form, part) for form, part in (("lean-wide", lean), ("general-wide", [i for i in idx if i not in lean])) if part]

    def restore(self):
        set_eval_path(self.bp, "auto")
        self.bp.set_eval_form("auto")


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Handle(name, ws.instances(name))
        return made[name]
    yield get
    for h in made.values():
        h.restore()
        h.bp.close()


@pytest.fixture(scope="module")
def plain_records():
    """(scene, pattern) -> {instance index: record bytes} of test 1's launches under PATHS[0], for test 2"""
    return {}


# ---- 1 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,pattern", CASES, ids=[f"{s}-{p}" for s, p in CASES])
def test_the_budget_under_every_wide_kernel(handles, plain_records, name, pattern):
    h = handles(name)
    assert h.bp.sample_capacity == _abi.MAX_PLAN_SAMPLES
    launches = h.launches(pattern)
    assert [f for f, _ in launches] == (["lean-wide", "general-wide"] if name == "straight" else ["general-wide"])
    first = {}
    try:
        for path in PATHS:
            set_path(h.bp, path)
            for form, idx in launches:
                if form == "lean-wide":              # exactly the eps S < 1 instances
                    assert all(h.insts[i].eps * h.insts[i].S < 1 for i in idx) and len(idx) == 4
                else:
                    assert all(h.insts[i].eps * h.insts[i].S >= 1 or name != "straight" for i in idx)
                res = h.bp.plan_batch([h.reqs[i] for i in idx])
                assert h.bp.last_eval_form() == form, f"{name} {pattern} [{path}]: {h.bp.last_eval_form()}"
                assert_no_flat_launch(h.bp, f"{name} {pattern} [{path}]")
                for slot, i in enumerate(idx):
                    check_instance(h.bp, res, slot, h.insts[i], path)
                    b = rec_bytes(res.records[slot])
                    assert first.setdefault(i, b) == b, f"{h.insts[i].label()}: record under [{path}] differs from [{PATHS[0]}]"
        plain_records[(name, pattern)] = first
    finally:
        h.restore()


# ---- 2 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,pattern", CASES, ids=[f"{s}-{p}" for s, p in CASES])
def test_float32_and_time_major_tensors(handles, plain_records, name, pattern):
    h = handles(name)
    try:
        if (name, pattern) not in plain_records:     # (run alone: the float64 launch of test 1 under its first path)
            set_path(h.bp, PATHS[0])
            plain_records[(name, pattern)] = {}
            for _form, idx in h.launches(pattern):
                res = h.bp.plan_batch([h.reqs[i] for i in idx])
                plain_records[(name, pattern)].update({i: rec_bytes(res.records[s]) for s, i in enumerate(idx)})
        plain = plain_records[(name, pattern)]
        for path in ("group", "split-wave"):
            set_eval_path(h.bp, path)
            for dtype, tsp in ((np.float64, True), (np.float32, False), (np.float32, True)):
                how = f"{path}, {np.dtype(dtype).name}{', time-major' if tsp else ''}"
                for form, idx in h.launches(pattern):
                    res = h.bp.plan_packed(PackedBatch([h.reqs[i] for i in idx], dtype, dyn_layout_tsp=tsp))
                    assert h.bp.last_eval_form() == form, how
                    assert_no_flat_launch(h.bp, f"{name} [{how}]")
                    for slot, i in enumerate(idx):
                        check_instance(h.bp, res, slot, h.insts[i], how)
                        assert rec_bytes(res.records[slot]) == plain[i], f"{h.insts[i].label()} [{how}]: record differs"
    finally:
        h.restore()


# ---- 3, 4 -------------------------------------------------------------------------------------------------------------

def _pick(insts, pattern, eps, S, cand):
    return next(i for i in insts if (i.pattern, i.eps, i.S, i.cand) == (pattern, eps, S, cand))


@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_a_wide_instance_in_company(name):
    """eps = 0.5 is a pair of both modules: (0.5, 2) and (0.5, 64) there, (0.5, 128) here; eps = 0.1 at 33 samples is a
    second scenario.  One launch on one scenario, one launch over both."""
    sc = ws.scene(name)
    c = sc.cands[0]
    narrow = [_pick(cb.instances(name), p, 0.5, S, c) for p, S in (("A", 64), ("B", 64), ("C", 2))]
    other = [_pick(cb.instances(name), p, 0.1, 33, c) for p in ("A", "B")]
    wide = [_pick(ws.instances(name), "B", 0.5, 128, c), _pick(ws.instances(name), "A", 0.5, 128, sc.cands[1])]
    everything = narrow + other + wide
    raised, default = Handle(name, everything), Handle(name, everything, sample_capacity=None)
    try:
        assert default.bp.sample_capacity == _abi.MAX_SAMPLES and raised.keys == default.keys == [(0.5, 1.0), (0.1, 1.0)]
        alone = {}
        for inst in narrow + other:                  # alone on the DEFAULT handle: today's kernels
            res = default.bp.plan_batch([default.req(inst)])
            assert default.bp.last_eval_form() == "general"
            check_instance(default.bp, res, 0, inst, "alone, default handle")
            alone[id(inst)] = rec_bytes(res.records[0])
        for inst in wide:
            res = raised.bp.plan_batch([raised.req(inst)])
            assert raised.bp.last_eval_form() == "general-wide"
            check_instance(raised.bp, res, 0, inst, "alone")
            alone[id(inst)] = rec_bytes(res.records[0])
        for how, group in (("one scenario", narrow + wide[:1]), ("one scenario, wide first", wide + narrow),
                           ("mixed scenarios", [other[0], narrow[0], wide[0], other[1], narrow[1], wide[1], narrow[2]])):
            for path in ("auto", "group", "wave"):
                set_eval_path(raised.bp, path)
                res = raised.bp.plan_batch([raised.req(i) for i in group])
                assert raised.bp.last_eval_form() == "general-wide", how
                assert_no_flat_launch(raised.bp, how)
                for slot, inst in enumerate(group):
                    check_instance(raised.bp, res, slot, inst, f"{how} [{path}]")
                    assert rec_bytes(res.records[slot]) == alone[id(inst)], f"{inst.label()} [{how}, {path}]: differs from alone"
    finally:
        raised.bp.close()
        default.bp.close()


@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_64_samples_on_a_raised_handle_run_todays_kernels(name):
    sc = ws.scene(name)
    c = sc.cands[0]
    budget = [_pick(cb.instances(name), p, 0.5, 64, c) for p in ("A", "B", "C")]
    d, ids = ws.hits(sc, c, 64, 1, False)            # eps = 0, one hit of sample 63: lean-eligible on the straight scene
    hard = cb._instance(sc, "B", "B", 0.0, 64, c, True, hit_ids=ids, dist=d)
    hard.want = sc.oracle(hard.req, 0.0, 1.0)
    everything = budget + [hard]
    raised, default = Handle(name, everything), Handle(name, everything, sample_capacity=None)
    try:
        for group, form in ((budget, "general"), ([hard], "lean" if ws.lean_eligible(sc, hard) else "general")):
            for path in EVAL_PATHS_NEVER_FLAT:
                recs = []
                for h in (default, raised):
                    set_eval_path(h.bp, path)
                    res = h.bp.plan_batch([h.req(i) for i in group])
                    assert h.bp.last_eval_form() == form, f"{name} [{path}] capacity {h.bp.sample_capacity}"
                    for slot, inst in enumerate(group):
                        check_instance(h.bp, res, slot, inst, f"{path}, capacity {h.bp.sample_capacity}")
                    recs.append([rec_bytes(res.records[s]) for s in range(len(group))])
                assert recs[0] == recs[1], f"{name} [{path}]: a raised capacity changed a launch of 64 samples"
    finally:
        raised.bp.close()
        default.bp.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------

def test_capacity_argument_checks():
    sc = ws.scene("straight")
    bp = BatchPlanner(waypoints=sc.waypoints, **sc.planner_kw(0.0, 1.0))
    lib = _abi.lib()
    try:
        got = C.c_int32(-7)
        assert lib.fot_get_sample_capacity(bp._h, C.byref(got)) == _abi.OK and got.value == 64 == bp.sample_capacity
        assert lib.fot_get_sample_capacity(bp._h, None) == _abi.ERR_INVALID
        assert lib.fot_get_sample_capacity(None, C.byref(got)) == _abi.ERR_INVALID
        assert lib.fot_set_sample_capacity(None, 100) == _abi.ERR_INVALID
        for start in (64, 200):
            assert lib.fot_set_sample_capacity(bp._h, start) == _abi.OK and bp.sample_capacity == start
            for bad in (63, 255, 0, -1):
                assert lib.fot_set_sample_capacity(bp._h, bad) == _abi.ERR_INVALID, bad
                assert bp.sample_capacity == start, bad
                with pytest.raises(_abi.FotError) as e:
                    bp.set_sample_capacity(bad)
                assert e.value.code == _abi.ERR_INVALID and bp.sample_capacity == start
        for good in (64, 254, 128):
            assert lib.fot_set_sample_capacity(bp._h, good) == _abi.OK and bp.sample_capacity == good
    finally:
        bp.close()


@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_a_handle_raised_to_128(name):
    sc = ws.scene(name)
    c = sc.cands[0]
    fits = [_pick(ws.instances(name), p, 0.5, 128, c) for p in ws.PATTERNS]
    beyond = _pick(ws.instances(name), "B", 0.5, 129, c)
    h = Handle(name, fits + [beyond], sample_capacity=128)
    try:
        assert h.bp.sample_capacity == 128
        for round_ in range(2):                      # ... and again after the refusal: the handle is usable
            res = h.bp.plan_batch([h.req(i) for i in fits])
            assert h.bp.last_eval_form() == "general-wide"
            for slot, inst in enumerate(fits):
                check_instance(h.bp, res, slot, inst, f"capacity 128, round {round_}")
            for reqs in ([h.req(beyond)], [h.req(fits[0]), h.req(beyond)]):
                with pytest.raises(_abi.FotError) as e:
                    h.bp.plan_batch(reqs)
                assert e.value.code == _abi.ERR_UNSUPPORTED
                msg = _abi.lib().fot_last_error(h.bp._h).decode()
                assert "sample" in msg and "128" in msg and "129" in msg and "fot_set_sample_capacity" in msg, msg
        h.bp.set_sample_capacity(129)
        res = h.bp.plan_batch([h.req(beyond)])
        check_instance(h.bp, res, 0, beyond, "capacity 129")
    finally:
        h.bp.close()


def test_drop_in_planner_with_a_raised_capacity():
    from integrated_path_planning_amd import synthetic as syn
    from integrated_path_planning_amd.cubic_spline import CubicSpline2D
    from integrated_path_planning_amd.data_structures import EgoVehicleState
    from integrated_path_planning_amd.planner import FrenetPlanner
    csp = CubicSpline2D(list(syn.STRAIGHT_WX), list(syn.STRAIGHT_WY))
    ego = EgoVehicleState(5.0, 0.0, 0.0, 5.0, 0.0)
    pl = FrenetPlanner(csp, dt=0.2, sample_capacity=128)
    assert pl.engine.sample_capacity == 128
    far = np.full((129, 2, 26, 2), 400.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")               # no warning within the capacity
        path = pl.plan(ego, np.empty((0, 2)), dynamic_obstacles_distribution=far[:128])
    assert path is not None and pl.last_error is None and pl.engine.last_eval_form() == "lean-wide"
    assert pl.last_check_stats is not None and pl.last_check_stats["collision_error"] == 0
    with pytest.warns(RuntimeWarning, match="capacities") as rec:
        assert pl.plan(ego, np.empty((0, 2)), dynamic_obstacles_distribution=far) is None
        assert pl.plan(ego, np.empty((0, 2)), dynamic_obstacles_distribution=far) is None       # warned once
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert pl.last_check_stats is None and "sample" in pl.last_error and "128" in pl.last_error
    assert pl.plan(ego, np.empty((0, 2)), dynamic_obstacles_distribution=far[:128]) is not None and pl.last_error is None
    # every engine the planner builds has the capacity
    assert pl._engine_for_epsilon(0.25).sample_capacity == 128 and pl._engine_for_epsilon(0.25) is not pl.engine


def _cfg_of(sc, eps):
    kw = sc.base_kw
    fp = None if sc.footprint is None else ([float(o) for o in sc.footprint.offsets], float(sc.footprint.radius))
    return cp.cfg(max_speed=kw["max_speed"], max_accel=kw["max_accel"], max_curvature=kw["max_curvature"],
                  max_lat_accel=kw["max_lat_accel"], dt=kw["dt"], max_road_width=kw["max_road_width"],
                  robot_radius=kw["robot_radius"], obstacle_radius=kw["obstacle_radius"], chance_epsilon=eps, footprint=fp)


@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_the_external_path_checkers_on_a_raised_engine(name):
    """paths_collision_free / check_paths (k_check_ext_wide: collide_candidate_wide) against check_paths_common's NumPy
    restatement of the reference, on the target candidates' own paths and a budget instance of each pattern."""
    sc = ws.scene(name)
    picks = [_pick(ws.instances(name), p, eps, S, c) for (eps, S) in ((0.07, 100), (0.999, 254)) for p in ws.PATTERNS
             for c in sc.cands]
    h = Handle(name, picks)
    default = BatchPlanner(waypoints=sc.waypoints, **sc.planner_kw(0.07, 1.0))
    engines = {}
    try:
        h.bp.plan_batch([PlanRequest(**{**sc.request().__dict__})])          # the obstacle-free lattice: the candidates' paths
        fps = {c: h.bp.candidate_path(c) for c in sc.cands}
        n_cases = 0
        for inst in picks:
            if inst.eps not in engines:              # (the checkers read scenario 0 of their handle: an engine per eps)
                engines[inst.eps] = BatchPlanner(waypoints=sc.waypoints, sample_capacity=254, **sc.planner_kw(inst.eps, 1.0))
            eng = engines[inst.eps]
            dist = np.asarray(inst.req.dist)
            assert dist.shape[0] >= 100
            paths = [fps[c] for c in sc.cands]
            free = eng.paths_collision_free(paths, None, None, dist)
            cats = eng.check_paths(paths, None, None, None, dist)
            cfg_ = _cfg_of(sc, inst.eps)
            for k, c in enumerate(sc.cands):
                p = {f: list(getattr(fps[c], f)) for f in cp.FIELDS}
                want_free, margin = cp.collision_free(cfg_, p, dist=dist)
                want_cat, _ = cp.categorise(cfg_, p, dist=dist)
                assert margin > 1e-7, inst.label()                          # (no collision decision near the radius)
                assert bool(free[k]) == want_free and int(cats[k]) == want_cat, f"{inst.label()} path of cand {c}"
                if c == inst.cand:
                    assert want_free == (not inst.collides), inst.label()
                    assert want_cat == (cp.COLLISION if inst.collides else cp.OK), inst.label()
                    n_cases += 1
        assert n_cases == len(picks)
        # the capacity holds for the checkers as well: 255 samples are refused on a handle raised as far as it goes,
        # 100 on a default one
        far = sc.far_tensor(255)
        for eng, S in ((h.bp, 255), (default, 100)):
            for call in (lambda: eng.paths_collision_free([fps[sc.cands[0]]], None, None, far[:S]),
                         lambda: eng.check_paths([fps[sc.cands[0]]], None, None, None, far[:S])):
                with pytest.raises(_abi.FotError) as e:
                    call()
                assert e.value.code == _abi.ERR_UNSUPPORTED and "sample" in str(e.value)
        assert h.bp.paths_collision_free([fps[sc.cands[0]]], None, None, far[:254])[0]
        assert default.paths_collision_free([fps[sc.cands[0]]], None, None, far[:64])[0]
    finally:
        h.bp.close()
        default.close()
        for eng in engines.values():
            eng.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture(name, path):
    """tests/test_gpu_golden.py's comparison on the three reference cases of more than 64 samples"""
    g = Golden("wide_samples/" + name)
    bp = BatchPlanner(waypoints=(g["wx"], g["wy"]), sample_capacity=254, **g.planner_kwargs())
    try:
        set_path(bp, path)
        res = bp.plan_batch([request_from_golden(g)])
        assert bp.last_eval_form() == ("lean-wide" if name == "dist_s100_eps0" else "general-wide")
        assert_no_flat_launch(bp, f"{name} [{path}]")          # (an exactly straight path: the wide launches have no flat form)
        r = res.records[0]
        np.testing.assert_allclose(np.array(r.frenet0[:]), g["frenet0"], rtol=TIGHT, atol=TIGHT)
        np.testing.assert_allclose(np.array(r.ref0[:]), g["ref0"], rtol=TIGHT, atol=TIGHT)
        cost, status, keep, nt = bp.candidates(0)
        assert len(cost) == len(g["cand_cost"]) == r.n_cand
        np.testing.assert_array_equal(nt, g["cand_nt"])
        np.testing.assert_array_equal(keep, g["cand_keep"])
        np.testing.assert_allclose(cost, g["cand_cost"], rtol=TIGHT, atol=TIGHT)
        np.testing.assert_array_equal(status, g["cand_status"].astype(np.int32))
        stats = g["stats"]
        assert res.stats(0) == {_abi.STATUS_NAMES[i]: int(stats[i]) for i in range(8) if stats[i] >= 0}
        bi = int(g["best_index"])
        assert r.best_index == bi and bi >= 0
        p = res.path(0)
        np.testing.assert_allclose(p.cost, float(g["best_cost"]), rtol=TIGHT)
        for f in _abi.PATH_FIELDS:
            got, exp = np.array(getattr(p, f)), g["best_" + f]
            assert len(got) == len(exp), f
            if f == "yaw":
                np.testing.assert_allclose(wrap_angle(got - exp), 0.0, atol=TIGHT)
            else:
                np.testing.assert_allclose(got, exp, rtol=TIGHT, atol=TIGHT, err_msg=f)
        np.testing.assert_allclose(r.new_last_kappa, float(g["last_kappa_after"]), rtol=TIGHT, atol=TIGHT)
    finally:
        bp.close()


def test_a_default_handle_refuses_the_fixtures():
    g = Golden("wide_samples/dist_s100_eps005")
    bp = BatchPlanner(waypoints=(g["wx"], g["wy"]), **g.planner_kwargs())
    try:
        with pytest.raises(_abi.FotError) as e:
            bp.plan_batch([request_from_golden(g)])
        assert e.value.code == _abi.ERR_UNSUPPORTED and "sample" in str(e.value) and "64" in str(e.value)
    finally:
        bp.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_check_collision_distribution_counts_in_the_engine_of_its_epsilon(name):
    from integrated_path_planning_amd.cubic_spline import CubicSpline2D
    from integrated_path_planning_amd.planner import FrenetPlanner
    sc = ws.scene(name)
    kw = dict(sc.planner_kw(0.0, 1.0))
    kw.pop("chance_epsilon")
    wx, wy = sc.waypoints
    pl = FrenetPlanner(CubicSpline2D(list(wx), list(wy)), sample_capacity=254, **kw)
    pl.engine.plan_batch([PlanRequest(**{**sc.request().__dict__})])
    c = sc.cands[0]
    fp = pl.engine.candidate_path(c)
    for eps in (0.07, 0.29):
        a, b = (_pick(ws.instances(name), p, eps, 100, c) for p in ("A", "B"))
        assert pl._check_collision_distribution(fp, np.empty((0, 2)), np.asarray(a.req.dist), eps) is True, a.label()
        assert pl._check_collision_distribution(fp, np.empty((0, 2)), np.asarray(b.req.dist), eps) is False, b.label()
        assert pl._engine_for_epsilon(eps).sample_capacity == 254
        # the planner's own epsilon (0) forgives nothing: pattern A collides there as soon as one sample hits
        assert pl._check_collision_distribution(fp, np.empty((0, 2)), np.asarray(a.req.dist)) is False
    far = sc.far_tensor(100)
    assert pl._check_collision_distribution(fp, np.empty((0, 2)), far) is True
