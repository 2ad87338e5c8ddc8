"""The lean form of the evaluation kernels (k_evaluate_lean / _split_lean / _group_lean, and the flat forms
k_evaluate_split_lean_flat / _group_lean_flat of the latter two) on the GPU.

A plan call takes the lean form when every scenario of the handle has at most 64 samples per candidate and the single
centre circle, and every instance of the launch has no chance budget (max_viol == 0); anything else runs the general
form.  `BatchPlanner.set_eval_form("general")` forces the general form on an eligible call and `last_eval_form()` tells
which one the most recent call ran.  On an exactly straight path a lean launch of the split or the grouped shape takes
the flat form unless `set_flat(0)` holds it back; `set_flat(-1)` tells whether the most recent call did.  Most paths of
this module are straight, so every comparison names the kernel it wants and asserts that it ran:

  * three ways where the path is straight -- flat, lean (`set_flat(0)`: the kernels every bent road runs) and forced
    general -- and lean against forced-general elsewhere: byte-identical records, equal candidate tables; this also
    keeps the general form covered on eps = 0 inputs now that "auto" takes the lean one there.  Under the names
    "group-noflat" / "split-noflat" of helpers.EVAL_PATHS the first leg is itself held back: lean twice, then general;
  * the eligibility edges, each held against per-instance calls and the oracle, with the flat form and without;
  * band lanes: obstacles one float32 ulp inside / outside the collision radius and at the two float32 thresholds of the
    sink, on tiles of 1, 63 and 64 candidates, decided by the exact re-check that keeps its state in locals -- on their
    straight scenes under the flat kernels and under the lean ones.
"""
import numpy as np
import pytest

import eps_band
from conftest import Golden
from helpers import (EVAL_PATH_KNOBS, EVAL_PATHS, NOFLAT_PATHS, TIGHT, assert_flat_as_named, assert_record_matches_oracle,
                     oracle_plan_for_request, request_from_golden, request_from_instance, set_eval_path, took_flat,
                     waypoints_are_flat)
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.footprint import EgoFootprint
from integrated_path_planning_amd.planner import BatchPlanner
from oracle import oracle as orc
from test_gpu_collision_boundary import SCENES, Scene, expected_status, lib_points, straight
from test_gpu_scenarios import _check_table, _mixed_handle, _rec_bytes

pytestmark = pytest.mark.gpu

WP = (syn.STRAIGHT_WX, syn.STRAIGHT_WY)
# the eps = 0, single-circle goldens that reach the rare branches of the walk; one time grid (dt 0.1 s, 5 s), so one handle
GOLDENS = ["arc_singular", "trunc_end", "trunc_end60", "nan_ped_dist", "nan_ped_single", "creep", "standstill",
           "emergency_stop", "crawl_17857_3", "crawl_19368_3"]


def tables(bp, n):
    return [bp.candidates(i) for i in range(n)]


def assert_same_tables(a, b, label):
    for i, (ta, tb) in enumerate(zip(a, b)):
        for name, x, y in zip(("cost", "status", "keep", "n_t"), ta, tb):
            np.testing.assert_array_equal(x, y, err_msg=f"{label} inst {i}: {name} (lean against general)")


def both_forms(bp, reqs, label, eval_path, flat_path, **kw):
    """plan `reqs` under `eval_path` as the call runs by itself -- the flat form where every path is exactly straight
    (`flat_path`), the name allows it and its shape has a flat kernel, else the lean form --, where that was a flat
    launch again with the flat form held back (set_flat(0): the lean kernel), and with the general form forced.  Each
    launch is asserted to have run the kernel it stands for; records byte-identical, tables equal."""
    set_eval_path(bp, eval_path)
    bp.set_eval_form("auto")
    first = bp.plan_batch(reqs, **kw)
    assert bp.last_eval_form() == "lean", f"{label}: an eligible call ran the {bp.last_eval_form()} form"
    assert_flat_as_named(bp, eval_path, flat_path, label)
    was_flat = took_flat(bp)
    legs = [("flat" if was_flat else "lean", first, tables(bp, len(reqs)))]
    if was_flat:
        bp.set_flat(0)
        lean = bp.plan_batch(reqs, **kw)
        assert bp.last_eval_form() == "lean" and not took_flat(bp), f"{label}: set_flat(0) ran {bp.last_eval_form()}, flat {took_flat(bp)}"
        legs.append(("lean", lean, tables(bp, len(reqs))))
    bp.set_eval_form("general")
    gen = bp.plan_batch(reqs, **kw)
    assert bp.last_eval_form() == "general" and not took_flat(bp), label
    legs.append(("general", gen, tables(bp, len(reqs))))
    bp.set_eval_form("auto")
    set_eval_path(bp, eval_path)
    for name, res, tabs in legs[1:]:
        for i in range(len(reqs)):
            assert _rec_bytes(first.records[i]) == _rec_bytes(res.records[i]), f"{label} inst {i}: {legs[0][0]} and {name} records differ"
        assert_same_tables(legs[0][2], tabs, f"{label} ({legs[0][0]} against {name})")
    return first


@pytest.mark.parametrize("eval_path", EVAL_PATHS)
def test_lean_equals_forced_general_on_config3(eval_path):
    """Eight config-3 instances (20 samples x 30 pedestrians), float32 tensors; seed 1 finds no path."""
    bp = BatchPlanner(waypoints=WP, **syn.CONFIG3_PLANNER)
    set_eval_path(bp, eval_path)
    reqs = [request_from_instance(syn.config3_instance(s, S=20, P=30)) for s in range(8)]
    res = both_forms(bp, reqs, f"config 3 [{eval_path}]", eval_path, True, obstacle_dtype=np.float32)
    assert res.status(1) == _abi.PLAN_NO_PATH and res.status(0) == _abi.PLAN_OK
    bp.close()


@pytest.mark.parametrize("eval_path", EVAL_PATHS)
def test_lean_equals_forced_general_on_the_goldens_in_one_call(eval_path):
    gs = [Golden(n) for n in GOLDENS]
    bp = _mixed_handle(gs)
    set_eval_path(bp, eval_path)
    reqs = []
    for k, g in enumerate(gs):
        r = request_from_golden(g)
        r.scenario = k
        reqs.append(r)
    all_flat = all(waypoints_are_flat(g["wx"], g["wy"]) for g in gs)
    assert not all_flat and sum(waypoints_are_flat(g["wx"], g["wy"]) for g in gs) == 7     # (arc_singular and the crawls bend)
    both_forms(bp, reqs, f"goldens [{eval_path}]", eval_path, all_flat)
    bp.plan_batch(reqs)                                      # (lean again: its tables against the reference's)
    assert bp.last_eval_form() == "lean" and not took_flat(bp)
    for i, g in enumerate(gs):
        _check_table(bp, i, g, f"{g.name} lean [{eval_path}]")
    bp.close()


@pytest.mark.parametrize("eval_path", EVAL_PATHS)
def test_flat_lean_and_general_on_the_straight_goldens_in_one_call(eval_path):
    """The goldens of the list whose path is exactly straight, alone in a call: such a launch takes the flat form, so the
    rare branches they reach (truncation at the path's end, NaN pedestrians, creep, standstill, emergency stop) are
    walked by the flat kernel, by the lean kernel with the flat form held back, and by the general one; the lean
    kernel's tables are then held to the reference's."""
    gs = [g for g in (Golden(n) for n in GOLDENS) if waypoints_are_flat(g["wx"], g["wy"])]
    assert [g.name for g in gs] == ["trunc_end", "trunc_end60", "nan_ped_dist", "nan_ped_single", "creep", "standstill",
                                    "emergency_stop"]
    bp = _mixed_handle(gs)
    reqs = []
    for k, g in enumerate(gs):
        r = request_from_golden(g)
        r.scenario = k
        reqs.append(r)
    both_forms(bp, reqs, f"straight goldens [{eval_path}]", eval_path, True)
    for flat in (1, 0):
        bp.set_flat(flat and EVAL_PATH_KNOBS[eval_path][2])
        bp.plan_batch(reqs)
        assert bp.last_eval_form() == "lean"
        if not flat:
            assert not took_flat(bp)
        for i, g in enumerate(gs):
            _check_table(bp, i, g, f"{g.name} {'as named' if flat else 'lean, flat form off'} [{eval_path}]")
    bp.close()


# ---- eligibility edges ------------------------------------------------------------------------------------------------

def oracle_of(kw, wp=WP):
    okw = dict(kw)
    fp = okw.pop("footprint", None)
    if fp is not None:
        okw["footprint_offsets"], okw["footprint_radius"] = list(fp.offsets), fp.radius
    return orc.make_params(**okw), orc.Spline(*wp)


def oracle_plans(reqs, kws):
    out = []
    for rq in reqs:
        params, sp = oracle_of(kws[rq.scenario])
        out.append(oracle_plan_for_request(orc, params, sp, rq, table=True))
    return out


def check_against_oracle(bp, res, wants, label):
    for i, want in enumerate(wants):
        lab = f"{label} inst {i}"
        assert_record_matches_oracle(res.records[i], want, label=lab)
        cost, status, keep, nt = bp.candidates(i)
        np.testing.assert_array_equal(keep, want.cand_keep, err_msg=lab)
        np.testing.assert_allclose(cost, want.cand_cost, rtol=TIGHT, atol=TIGHT, err_msg=lab)
        eps_band.check_status_table(bp, i, status, want.cand_status, lab)


def c3_request(seed, scenario=0):
    r = request_from_instance(syn.config3_instance(seed, S=20, P=30))
    for f in ("static", "dyn", "dist"):                      # float64 inputs: the oracle sees the values the device sees
        v = getattr(r, f)
        if v is not None:
            setattr(r, f, np.asarray(v, np.float64))
    r.scenario = scenario
    return r


def plan_and_check(kws, reqs, expect, label):
    """One handle with scenario k on planner kws[k]: the batch must run the `expect` form, equal the oracle, and equal
    the per-instance calls byte for byte.  Returns the form each per-instance call ran."""
    bp = BatchPlanner(waypoints=WP, **kws[0])
    for k, kw in enumerate(kws[1:], start=1):
        assert bp.add_scenario(waypoints=WP, **kw) == k
    wants = oracle_plans(reqs, kws)
    for path in ("auto", "group", "group-noflat", "split-noflat"):       # (WP is straight: flat kernels, then lean ones)
        set_eval_path(bp, path)
        res = bp.plan_batch(reqs)
        assert bp.last_eval_form() == expect, f"{label} [{path}]: ran the {bp.last_eval_form()} form"
        if expect == "lean":
            assert_flat_as_named(bp, path, True, label)
        else:
            assert not took_flat(bp), f"{label} [{path}]: a general launch took a flat kernel"
        check_against_oracle(bp, res, wants, f"{label} [{path}]")
        singles = []
        for i, rq in enumerate(reqs):
            one = bp.plan_batch([rq])
            singles.append(bp.last_eval_form())
            assert took_flat(bp) == (singles[-1] == "lean" and path in ("auto", "group")), f"{label} [{path}] inst {i} alone"
            assert _rec_bytes(one.records[0]) == _rec_bytes(res.records[i]), f"{label} [{path}] inst {i}: batch against single call"
    bp.close()
    return singles


def test_a_batch_with_one_chance_budget_runs_general():
    """eps = 0 and eps = 0.1 (max_viol 2 of 20 samples) in one launch; alone, the eps = 0 instance runs lean."""
    kws = [dict(syn.CONFIG3_PLANNER, chance_epsilon=0.0), dict(syn.CONFIG3_PLANNER, chance_epsilon=0.1)]
    singles = plan_and_check(kws, [c3_request(0, 0), c3_request(2, 1)], "general", "eps 0 + eps 0.1")
    assert singles == ["lean", "general"]
    # the same handle, only its eps = 0 scenario in the batch: eligible
    assert plan_and_check(kws, [c3_request(0, 0), c3_request(3, 0)], "lean", "eps 0 twice") == ["lean", "lean"]


@pytest.mark.parametrize("max_t,n_total,expect", [(6.3, 64, "lean"), (6.4, 65, "general")])
def test_sixty_four_samples_run_lean_sixty_five_general(max_t, n_total, expect):
    """The same scene with 6.3 s and 6.4 s of horizon at dt 0.1: 64 and 65 samples per candidate (the per-step values
    of a tile sit in the 64 lanes of its wave; the lean form never reloads them)."""
    kw = dict(syn.CONFIG3_PLANNER, dt=0.1, min_t=max_t - 0.4, max_t=max_t)
    assert int(round(kw["max_t"] / kw["dt"])) + 1 == n_total
    singles = plan_and_check([kw], [c3_request(0), c3_request(4), c3_request(5)], expect, f"{n_total} samples")
    assert set(singles) == {expect}


@pytest.mark.parametrize("n_circles,expect", [(0, "lean"), (3, "general")])
def test_the_centre_circle_runs_lean_three_footprint_circles_general(n_circles, expect):
    kw = dict(syn.CONFIG3_PLANNER)
    if n_circles:
        kw["footprint"] = EgoFootprint.multi_circle(4.5, 1.8, n_circles)
    plan_and_check([kw], [c3_request(0), c3_request(6)], expect, f"{n_circles} footprint circles")


def test_one_ineligible_scenario_makes_the_handle_general():
    """Eligibility is the handle's: a scenario with footprint circles, even one no instance of the batch uses, keeps
    every launch on the general form (the kernels resolve the scenario per instance)."""
    fp = EgoFootprint.multi_circle(4.5, 1.8, 3)
    kws = [dict(syn.CONFIG3_PLANNER), dict(syn.CONFIG3_PLANNER, footprint=fp)]
    plan_and_check(kws, [c3_request(0, 0), c3_request(7, 1)], "general", "mixed scenarios")
    plan_and_check(kws, [c3_request(0, 0), c3_request(7, 0)], "general", "only the eligible scenario in the batch")


# ---- band lanes -------------------------------------------------------------------------------------------------------

# Lattices whose per-wave cut (tile_extent, csrc/fot_math.hpp) makes tiles of 64 and 63, and of 3 and 1 candidates:
#  * 63 lateral offsets x 2 terminal speeds x 1 horizon + 1 brake-ladder entry = 127 candidates: 64 | 62 + 1;
#  * 1 lateral offset x 4 terminal speeds x 1 horizon of 0.5 s (no brake ladder below 0.5 s): three profiles of 11 rows
#    fit the 41 rows a wave stages, the fourth does not: 3 | 1.
SCENES.setdefault("lean_64_63", (straight(0.7, 250.0), dict(dt=0.1, min_t=1.0, max_t=1.0, max_speed=25.0, d_road_w=0.05,
                                                              max_road_width=1.55, d_t_s=20.0),
                                 (10.0, 0.3, 0.02, 8.0, 0.0), 10.0))
SCENES.setdefault("lean_3_1", (straight(0.7, 250.0), dict(dt=0.05, min_t=0.5, max_t=0.5, max_speed=25.0, d_road_w=1.0,
                                                            max_road_width=0.5, d_t_s=0.3),
                               (10.0, 0.0, 0.0, 1.0, 0.0), 0.9))


def wave_cut(kw, target):
    """tile_extent / profile_rows of csrc/fot_math.hpp for the per-wave cut: the tile sizes of the lattice"""
    dt = kw["dt"]
    n_total = int(round(kw["max_t"] / dt)) + 1
    n_ti = int((kw["max_t"] - kw["min_t"]) / dt + 1e-9) + 1
    n_di = 2 * int(kw["max_road_width"] / kw["d_road_w"] + 1e-9) + 1
    n_down = int(target / kw["d_t_s"] + 1e-9)
    n_tv = n_down + 1 + (1 if target - n_down * kw["d_t_s"] > 1e-9 else 0)
    rows = [int(round((kw["min_t"] + i * dt) / dt)) + 1 for i in range(n_ti) for _ in range(n_tv)]
    n_grid = len(rows) * n_di
    for j in range(max(int(np.ceil((kw["min_t"] - 1e-9 - 0.5) / 0.5)), 0)):
        ne = int(round((0.5 + 0.5 * j) / dt)) + 1
        if ne <= n_total:
            rows.append(ne + 1 if ne < n_total else ne)
    n_cand = n_grid + len(rows) - n_grid // n_di
    budget = min(3 * n_total + 8, 176) if 3 * n_total + 8 < 176 else max(176, n_total)
    tiles, c = [], 0
    while c < n_cand:
        n = used = profs = 0
        while n < 64 and c < n_cand and profs < 8:
            slot, left = (c // n_di, (c // n_di + 1) * n_di - c) if c < n_grid else (n_grid // n_di + c - n_grid, 1)
            if profs > 0 and used + rows[slot] > budget:
                break
            used += rows[slot]; profs += 1
            take = min(left, 64 - n)
            n += take; c += take
        tiles.append(n)
    return tiles


def thresholds32(sq, bound):
    """filter_threshold / filter_threshold_sure (csrc/fot_math.hpp) at |x| + |y| = bound, in float32"""
    f = np.float32
    sq32 = f(sq)
    r = f(np.sqrt(sq32)) + f(1.0)
    e = (f(bound) + f(2.0) * r + f(12.0)) * f(4.7683716e-7)
    thr = (sq32 + f(4.0) * r * e) * f(1.000002)
    sure = (sq32 * f(0.9999999) - f(4.0) * r * e) * f(0.999998)
    return float(thr), float(sure)


# The same two lattices on a path along +x (y exactly constant): there "auto" and "group" launch the flat kernels, whose
# band lanes take the same re-check, and "group-noflat" / "split-noflat" the lean ones.  (The scenes above head 0.7 rad:
# never flat, asserted.)
for _name in ("lean_64_63", "lean_3_1"):
    SCENES.setdefault(_name + "_x", (straight(0.0, 250.0),) + SCENES[_name][1:])


@pytest.mark.parametrize("scene,want_tiles,cands", [("lean_64_63", [64, 63], (0, 62, 100, 126)), ("lean_3_1", [3, 1], (2, 3)),
                                                    ("lean_64_63_x", [64, 63], (0, 62, 100, 126)), ("lean_3_1_x", [3, 1], (2, 3))])
def test_band_lanes_on_tiles_of_1_63_and_64_candidates(scene, want_tiles, cands):
    """Static obstacles whose float32 distance to a candidate's point falls between the sink's two thresholds, so that
    the lane leaves the min-only walk for the per-chunk walk and the float64 re-check: one float32 ulp of the radius
    inside and outside, and at the thresholds themselves for the point's own |x| + |y| and for tile boxes up to 6 m
    wider.  Each candidate's status must be what the float64 predicate says on the library's own points."""
    sc = Scene(scene, {})
    assert wave_cut(sc.kw, sc.target) == want_tiles, f"{scene}: per-wave tiles {wave_cut(sc.kw, sc.target)}"
    assert len(sc.lib_status) == sum(want_tiles)
    _, _, keep, _ = sc.bp.candidates(0)
    X, Y = lib_points(sc)
    r32 = np.float32(sc.r)
    sq = sc.r * sc.r
    reqs, labels, target = [], [], []
    for c in cands:
        assert sc.lib_status[c] == _abi.ST_OK, f"{scene}: candidate {c} does not reach the collision check"
        for k in (1, int(keep[c]) - 1):
            p = np.array([X[c, k], Y[c, k]])
            yaw = sc.lib_path(c)[2][k]
            u = np.array([-np.sin(yaw), np.cos(yaw)])
            bound = abs(np.float32(p[0] - sc.ego.x)) + abs(np.float32(p[1] - sc.ego.y))
            dists = [(float(r32) - float(np.spacing(r32)), "radius - 1 ulp32"), (float(r32) + float(np.spacing(r32)), "radius + 1 ulp32")]
            for grow in (0.0, 1.0, 3.0, 6.0):
                thr, sure = thresholds32(sq, bound + grow)
                dists += [(np.sqrt(thr), f"thr (+{grow} m)"), (np.sqrt(sure), f"thr_sure (+{grow} m)")]
            for d, what in dists:
                reqs.append(sc.request(static=(p + d * u)[None].copy()))
                labels.append(f"cand {c} step {k} {what} ({d / sc.r - 1.0:+.2e} of the radius)")
                target.append(c)
    want = [expected_status(sc, X, Y, keep, rq.static) for rq in reqs]
    # (half of the placements lie inside the radius of their own candidate's point, half outside; neighbours may be hit)
    n_hit = sum(int(w[c] == _abi.ST_COLLISION) for w, c in zip(want, target))
    assert len(reqs) // 4 <= n_hit <= 3 * len(reqs) // 4, f"{scene}: {n_hit} of {len(reqs)} placements hit their candidate"
    flat_path = waypoints_are_flat(*SCENES[scene][0])
    assert flat_path == scene.endswith("_x")
    assert len(reqs) * len(want_tiles) <= 2304                   # ("auto": a split launch)
    for path in ("wave", "auto", "group") + (NOFLAT_PATHS if flat_path else ()):
        set_eval_path(sc.bp, path)
        sc.bp.plan_batch(reqs)
        assert sc.bp.last_eval_form() == "lean", f"{scene} [{path}]"
        assert_flat_as_named(sc.bp, path, flat_path, scene)
        for i, w in enumerate(want):
            _, status, _, _ = sc.bp.candidates(i)
            bad = np.flatnonzero(status != w)
            assert not len(bad), f"{scene} inst {i} [{path}] {labels[i]}: {len(bad)} candidate(s) differ from the float64 " \
                                 f"predicate, e.g. cand {bad[0]}: got {status[bad[0]]} want {w[bad[0]]}"
    set_eval_path(sc.bp, "auto")
    sc.bp.close()
