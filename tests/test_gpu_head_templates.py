"""The header templates on the GPU: k_frenet_state composes every group header (GroupHead) from the handle's templates
(HeadTemplate: what the lattice alone decides, built on the host with the tile table) and the instance's own fields.

One small batch holds the states in which a header is composed differently: a moving ego (the variant with the brake
ladder), an ego at the 0.1 m/s brake gate and a standing one (the variant without), an ego whose conversion fails (EMPTY
headers only), a chain of two (the head's workgroup writes both members' headers) and an ego given as a Frenet state.
It runs on a lattice whose one-speed shape is a single tile and on the default lattice; the records must be
byte-identical between the grouped kernels (which read the headers) and the per-wave kernels (which have none), and
match the oracle -- under "group", which on this module's exactly straight path launches k_evaluate_group_lean_flat, and
under "group-noflat", which launches k_evaluate_group_lean as any bent road does; both are asserted to.  Then, on the same handle, whatever rebuilds the tile table must rebuild the templates: a further
scenario with another group count, the tile cut changed and changed back, and one batch over the three scenario planners.
"""
import copy

import numpy as np
import pytest

from helpers import assert_record_matches_oracle, oracle_plan_for_request, set_eval_path, took_flat
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.batch import PlanRequest
from integrated_path_planning_amd.planner import BatchPlanner
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

WP = (syn.STRAIGHT_WX, syn.STRAIGHT_WY)
# one horizon (min_t == max_t): with one terminal speed (target 0) the whole lattice, brake ladder included, is one tile
SINGLE_TILE = dict(dt=0.1, min_t=3.0, max_t=3.0, d_t_s=0.5, max_road_width=2.0, d_road_w=0.5, max_speed=20.0,
                   robot_radius=0.8, obstacle_radius=0.2)
DEFAULT = dict(syn.CONFIG2_PLANNER)                              # dt 0.1 s, the module defaults otherwise
# on DEFAULT's time grid, three times its horizons at half its lateral offsets: another number of groups per shape
OTHER_GROUPS = dict(DEFAULT, min_t=3.0, d_road_w=1.0, max_road_width=4.0, robot_radius=1.0, obstacle_radius=0.2)


def rec_bytes(rec):
    return bytes(memoryview(rec).cast("B"))


def obstacles(seed, n_total):
    rng = np.random.default_rng(seed)
    dyn = np.array([25.0, 0.3]) + rng.normal(0, 5.0, (6, 1, 2)) + np.cumsum(rng.normal(0, 0.1, (6, n_total, 2)), axis=1)
    static = np.column_stack([rng.uniform(5, 60, 12), rng.uniform(-5, 5, 12)])
    return dyn, static


def the_batch(bp, scenario=0, seed=1):
    """moving | at the gate | standing | no Frenet state | chain head | chain member | given as a Frenet state"""
    dyn, static = obstacles(seed, bp.n_total_samples)
    kw = dict(dyn=dyn, static=static, scenario=scenario)
    moving = PlanRequest(20.0, 0.6, 0.05, 5.0, 0.2, target_speed=6.0, **kw)
    set_eval_path(bp, "group")
    fr = bp.plan_batch([moving]).records[0].frenet0
    return [
        moving,
        PlanRequest(15.0, 0.0, 0.0, 0.1, 0.0, target_speed=2.2, **kw),
        PlanRequest(15.0, -0.2, 0.0, 0.0, 0.0, target_speed=0.0, **kw),
        PlanRequest(500.0, 1.0, 0.0, 0.0, 0.0, is_frenet=True, scenario=scenario),
        PlanRequest(12.0, 0.3, 0.02, 6.0, 0.2, target_speed=0.0, **kw),
        PlanRequest(12.0, 0.3, 0.02, 6.0, 0.2, target_speed=4.5, chain_prev_s=True, overrides={"max_accel": 1.5}, **kw),
        PlanRequest(*[float(v) for v in fr[:5]], last_kappa=float(fr[5]), is_frenet=True, target_speed=6.0, **kw),
    ]


FAILED, CHAIN_HEAD, CHAIN_MEMBER, GIVEN = 3, 4, 5, 6


GROUPED = ("group", "group-noflat")


def group_and_wave(bp, reqs, label, flat=True):
    """the batch under both cuts (each change of the cut rebuilds the tile table): byte-identical records.  flat: every
    path the launch uses is exactly straight, so "group" takes the flat kernel; "group-noflat" never does.  Returns the
    grouped results by name."""
    results = {}
    for path in GROUPED:
        set_eval_path(bp, path)
        results[path] = bp.plan_batch(reqs)
        want = flat and path == "group"
        assert bp.last_eval_form() == "lean", f"{label} [{path}]"
        assert took_flat(bp) == want, f"{label} [{path}]: flat launch {took_flat(bp)}, expected {want}"
    set_eval_path(bp, "wave")
    wave = bp.plan_batch(reqs)
    assert not took_flat(bp), f"{label} [wave]"
    for path, grouped in results.items():
        for i in range(len(reqs)):
            assert rec_bytes(grouped.records[i]) == rec_bytes(wave.records[i]), \
                f"{label} inst {i}: the grouped record [{path}] differs from the per-wave one"
    set_eval_path(bp, "group")
    return results


def against_oracle(results, reqs, kws, wps, label):
    """every record of every result (by path name) against the oracle; a chain member as the call behind its head, a
    given state without new_prev_s"""
    assert set(results) == set(GROUPED)
    prev_s = None
    for i, rq in enumerate(reqs):
        if rq.is_frenet and rq.x > 400.0:                       # beyond the path: no Frenet state
            for res in results.values():
                assert res.records[i].status == _abi.PLAN_C2F_FAILED and res.records[i].n_cand == 0, (label, i)
            continue
        one = copy.copy(rq)
        if rq.chain_prev_s:
            one.chain_prev_s, one.prev_s = False, prev_s
        given = None
        if rq.is_frenet:                                         # the oracle plans the Cartesian ego it came from
            given, one = one, copy.copy(reqs[0])
        want = oracle_plan_for_request(orc, orc.make_params(**kws[rq.scenario]), orc.Spline(*wps[rq.scenario]), one)
        prev_s = float(want.new_prev_s)
        if given is not None:
            want = copy.copy(want)
            want.new_prev_s = float("nan")
        for path, res in results.items():
            assert_record_matches_oracle(res.records[i], want, label=f"{label} [{path}] inst {i}")


def check_batch(bp, kws, wps, scenario, label, seed=1):
    reqs = the_batch(bp, scenario, seed)
    results = group_and_wave(bp, reqs, label)
    against_oracle(results, reqs, kws, wps, label)
    res = results["group"]
    n = [res.records[i].n_cand for i in range(len(reqs))]
    assert n == [results["group-noflat"].records[i].n_cand for i in range(len(reqs))]
    assert n[1] > 0 and n[2] > 0 and n[FAILED] == 0 and n[CHAIN_HEAD] != n[CHAIN_MEMBER], (label, n)
    return res, n


def test_single_tile_lattice():
    bp = BatchPlanner(waypoints=WP, **SINGLE_TILE)
    res, n = check_batch(bp, [SINGLE_TILE], [WP], 0, "single tile")
    n_di, ladder = 9, 5
    assert n[2] == n_di and n[CHAIN_HEAD] == n_di + ladder, n   # one speed: with the ladder, 14 candidates in one tile
    assert n[0] % n_di == ladder and n[1] % n_di == 0, n        # ladder of the moving ego, none at the gate
    bp.close()


def test_default_lattice_then_every_rebuild_of_the_tile_table():
    bp = BatchPlanner(waypoints=WP, **DEFAULT)
    kws, wps = [DEFAULT], [WP]
    _, n0 = check_batch(bp, kws, wps, 0, "default")
    # a further scenario whose shapes have another number of groups: the table and the templates are rebuilt
    assert bp.add_scenario(waypoints=WP, **OTHER_GROUPS) == 1
    kws.append(OTHER_GROUPS); wps.append(WP)
    _, n1 = check_batch(bp, kws, wps, 1, "other group count", seed=2)
    assert n1[0] != n0[0], (n0, n1)
    # (check_batch went to the per-wave cut and back: the first scenario's templates again)
    _, again = check_batch(bp, kws, wps, 0, "default again", seed=3)
    assert again == n0
    # the three scenario planners next to the two: one batch over all of them
    for w, kw in syn.SCENARIO_PLANNERS:
        kws.append(kw); wps.append(w)
        assert bp.add_scenario(waypoints=w, **kw) == len(kws) - 1
    reqs = []
    for s in range(9):
        r = syn.config3_instance(s, S=4, P=8)
        reqs.append(PlanRequest(*[float(v) for v in r.ego], target_speed=float(r.target_speed),
                                static=np.asarray(r.static, np.float64), scenario=2 + s % 3))
    reqs[4].v = 0.05                                             # (a standing ego among them)
    results = group_and_wave(bp, reqs, "scenarios", flat=False)  # (the third scenario planner's path is curved)
    against_oracle(results, reqs, kws, wps, "scenarios")
    bp.close()
