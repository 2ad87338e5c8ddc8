"""The group headers on the GPU: k_frenet_state builds one GroupHead per instance and group position, the grouped
evaluation kernels (k_evaluate_group / k_evaluate_group_lean / k_evaluate_group_lean_flat) read it instead of deriving its
content per workgroup.

Every case plans the same batch under the grouped cut -- "group", which on this module's exactly straight path means
the flat kernel for a lean launch, and "group-noflat", the lean kernel every bent road runs; both are asserted to have
launched what they name -- and under the per-wave cut ("wave": k_evaluate / k_evaluate_lean, which have no header), asks
for byte-identical records, then holds the records of both grouped launches to the oracle.
The cases are the states in which a header differs in kind: group positions a lattice does not have, groups past the
candidates of a standing ego, no Frenet state at all, chains and Frenet-given egos (whose headers k_frenet_state writes in
its chain loop), scenarios mixed in one call, both forms of the kernel, a horizon of more than 64 samples, and a handle
whose header table still holds an earlier, larger batch.
"""
import copy

import numpy as np
import pytest

import eps_band
from helpers import TIGHT, assert_record_matches_oracle, oracle_plan_for_request, request_from_instance, set_eval_path, took_flat
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.batch import PlanRequest
from integrated_path_planning_amd.planner import BatchPlanner
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

WP = (syn.STRAIGHT_WX, syn.STRAIGHT_WY)
# a lattice with a brake ladder (min_t 2 s: entries at 0.5, 1.0, 1.5 s) and up to 32 terminal speeds (d_t_s 0.5)
LATTICE = dict(dt=0.1, min_t=2.0, max_t=3.0, d_t_s=0.5, max_road_width=2.0, d_road_w=0.5, max_speed=20.0,
               robot_radius=0.8, obstacle_radius=0.2)


def rec_bytes(rec):
    return bytes(memoryview(rec).cast("B"))


def c3(seed, scenario=0):
    r = request_from_instance(syn.config3_instance(seed, S=4, P=8))
    r.scenario = scenario
    return r


def obstacles(seed):
    rng = np.random.default_rng(seed)
    dyn = np.array([25.0, 0.3]) + rng.normal(0, 5.0, (10, 1, 2)) + np.cumsum(rng.normal(0, 0.1, (10, 31, 2)), axis=1)
    static = np.column_stack([rng.uniform(5, 60, 20), rng.uniform(-5, 5, 20)])
    return dyn, static


GROUPED = ("group", "group-noflat")


def group_and_wave(bp, reqs, label, flat=True, **kw):
    """the batch under both cuts: byte-identical records.  flat: the launch under "group" is lean and every path it uses
    exactly straight, so it takes k_evaluate_group_lean_flat; "group-noflat" never does.  Returns the grouped results by
    name and the record bytes."""
    results = {}
    for path in GROUPED:
        set_eval_path(bp, path)
        results[path] = bp.plan_batch(reqs, **kw)
        want = flat and path == "group"
        assert took_flat(bp) == want, f"{label} [{path}]: flat launch {took_flat(bp)}, expected {want}"
        if flat:
            assert bp.last_eval_form() == "lean", f"{label} [{path}]"
    blobs = [rec_bytes(results["group"].records[i]) for i in range(len(reqs))]
    for i in range(len(reqs)):
        assert blobs[i] == rec_bytes(results["group-noflat"].records[i]), \
            f"{label} inst {i}: the flat grouped record differs from the lean grouped one"
    set_eval_path(bp, "wave")
    wave = bp.plan_batch(reqs, **kw)
    assert not took_flat(bp), f"{label} [wave]"
    for i in range(len(reqs)):
        assert blobs[i] == rec_bytes(wave.records[i]), f"{label} inst {i}: the grouped record differs from the per-wave one"
    set_eval_path(bp, "group")
    return results, blobs


def against_oracle(results, reqs, kws, wps, label, skip=()):
    """every result of `results` (by path name) against the oracle's plans, computed once"""
    wants = {i: oracle_plan_for_request(orc, orc.make_params(**kws[rq.scenario]), orc.Spline(*wps[rq.scenario]), rq)
             for i, rq in enumerate(reqs) if i not in skip}
    assert set(results) == set(GROUPED)
    for path, res in results.items():
        for i, want in wants.items():
            assert_record_matches_oracle(res.records[i], want, label=f"{label} [{path}] inst {i}")


def check(kw, reqs, label, wp=WP, form=None, flat=True, **plan_kw):
    bp = BatchPlanner(waypoints=wp, **kw)
    if form:
        bp.set_eval_form(form)
    results, _ = group_and_wave(bp, reqs, label, flat=flat, **plan_kw)
    if form:
        assert bp.last_eval_form() == form, label
    against_oracle(results, reqs, [kw], [wp], label)
    bp.close()
    return results["group"]


def test_one_instance():
    check(syn.CONFIG3_PLANNER, [c3(0)], "one instance", obstacle_dtype=np.float32)


def test_nine_instances_two_on_one_queue():
    check(syn.CONFIG3_PLANNER, [c3(s) for s in range(9)], "nine instances", obstacle_dtype=np.float32)


def test_ragged_terminal_speed_grids():
    """1, 2, 4, 17 and 32 terminal speeds in one call: the short lattices have no group at most positions."""
    dyn, static = obstacles(3)
    targets = [0.0, 0.3, 1.5, 8.0, 15.5, 0.0]
    reqs = [PlanRequest(3.0 + 2 * i, 0.2 - 0.1 * i, 0.01, 5.0, 0.1, target_speed=t, dyn=dyn if i % 2 else None,
                        static=static) for i, t in enumerate(targets)]
    res = check(LATTICE, reqs, "ragged")
    n_cand = [res.records[i].n_cand for i in range(len(reqs))]
    n_di, n_ti, ladder = 9, 11, 3
    assert n_cand == [n_ti * n_tv * n_di + ladder for n_tv in (1, 2, 4, 17, 32, 1)], n_cand


def test_standing_ego_without_brake_ladder():
    """v = 0.05 m/s: below the brake gate, n_cand ends at the grid -- the tile that holds the ladder is cut short or empty."""
    dyn, static = obstacles(4)
    reqs = [PlanRequest(15.0, 0.0, 0.0, 0.05, 0.0, target_speed=t, static=static, dyn=dyn) for t in (4.1, 1.0, 0.0)]
    res = check(LATTICE, reqs, "standing")
    assert [res.records[i].n_cand for i in range(3)] == [11 * n_tv * 9 for n_tv in (10, 3, 1)]


def test_ego_just_over_the_brake_gate():
    dyn, static = obstacles(5)
    reqs = [PlanRequest(15.0, 0.0, 0.0, v, 0.0, target_speed=2.2, static=static, dyn=dyn) for v in (0.11, 0.1, 0.09)]
    res = check(LATTICE, reqs, "0.11 m/s")
    assert [res.records[i].n_cand - 11 * 6 * 9 for i in range(3)] == [3, 0, 0]


def test_no_frenet_state_between_two_healthy_instances():
    """The middle instance is given as a Frenet state beyond the end of the path: no state, every header says skip."""
    reqs = [c3(0), PlanRequest(500.0, 1.0, 0.0, 0.0, 0.0, is_frenet=True), c3(2)]
    bp = BatchPlanner(waypoints=WP, **syn.CONFIG3_PLANNER)
    results, _ = group_and_wave(bp, reqs, "failed c2f", obstacle_dtype=np.float32)
    for res in results.values():
        assert res.records[1].status == _abi.PLAN_C2F_FAILED and res.records[1].n_cand == 0
    against_oracle(results, reqs, [syn.CONFIG3_PLANNER], [WP], "failed c2f", skip=(1,))
    bp.close()


def test_chain_of_three():
    """chain_prev_s: the head's workgroup of k_frenet_state walks the chain and writes every member's headers."""
    dyn, static = obstacles(6)
    reqs = []
    for j in range(3):
        reqs.append(PlanRequest(12.0, 0.3, 0.02, 6.0, 0.2, target_speed=7.0 - 2.5 * j, dyn=dyn, static=static,
                                chain_prev_s=j > 0, overrides={"max_accel": 1.0 + 0.5 * j} if j else None))
    bp = BatchPlanner(waypoints=WP, **LATTICE)
    results, _ = group_and_wave(bp, [c3(1)] + reqs + [c3(2)], "chain")
    prev_s = None
    for j, rq in enumerate(reqs):                                # the oracle, call by call, as the chain stands for
        one = copy.copy(rq)
        one.chain_prev_s, one.prev_s = False, prev_s
        want = oracle_plan_for_request(orc, orc.make_params(**LATTICE), orc.Spline(*WP), one)
        for path, res in results.items():
            assert_record_matches_oracle(res.records[1 + j], want, label=f"chain member {j} [{path}]")
        prev_s = float(want.new_prev_s)
    for res in results.values():
        assert len({res.records[1 + j].n_cand for j in range(3)}) == 3
    bp.close()


def test_ego_given_as_frenet_state():
    dyn, static = obstacles(7)
    ego = PlanRequest(20.0, 0.6, 0.05, 5.0, 0.2, target_speed=6.0, dyn=dyn, static=static)
    bp = BatchPlanner(waypoints=WP, **LATTICE)
    rec0 = bp.plan_batch([ego]).records[0]
    given = PlanRequest(*[float(v) for v in rec0.frenet0[:5]], last_kappa=float(rec0.frenet0[5]), is_frenet=True,
                        target_speed=6.0, dyn=dyn, static=static)
    results, _ = group_and_wave(bp, [given, ego], "frenet given")
    want = oracle_plan_for_request(orc, orc.make_params(**LATTICE), orc.Spline(*WP), ego)
    want_given = copy.copy(want)
    want_given.new_prev_s = float("nan")                        # (no nearest-point search: the record has none)
    for path, res in results.items():
        assert_record_matches_oracle(res.records[1], want, label=f"cartesian ego [{path}]")
        assert_record_matches_oracle(res.records[0], want_given, label=f"the same ego as a Frenet state [{path}]")
    bp.close()


def test_three_scenarios_in_one_call():
    (w0, kw0), *rest = syn.SCENARIO_PLANNERS
    bp = BatchPlanner(waypoints=w0, **kw0)
    for k, (w, kw) in enumerate(rest, start=1):
        assert bp.add_scenario(waypoints=w, **kw) == k
    reqs = [c3(s, scenario=(s * 7 // 5) % 3) for s in range(9)]
    assert {r.scenario for r in reqs} == {0, 1, 2}
    results, _ = group_and_wave(bp, reqs, "scenarios", flat=False, obstacle_dtype=np.float32)   # (the third path is curved)
    assert bp.last_eval_form() == "lean"
    against_oracle(results, reqs, [kw for _, kw in syn.SCENARIO_PLANNERS], [w for w, _ in syn.SCENARIO_PLANNERS], "scenarios")
    bp.close()


def test_general_form_forced():
    check(syn.CONFIG3_PLANNER, [c3(s) for s in range(5)], "general form", form="general", flat=False, obstacle_dtype=np.float32)


def test_sixty_five_sample_horizon():
    """dt 0.1 s, 6.4 s: 65 samples per candidate -- the general form, per-step values in two blocks of 64."""
    kw = dict(syn.CONFIG3_PLANNER, dt=0.1, min_t=6.0, max_t=6.4)
    assert int(round(kw["max_t"] / kw["dt"])) + 1 == 65
    reqs = []
    for s in (0, 4, 5):
        r = c3(s)
        for f in ("static", "dyn", "dist"):                     # (65 steps: the instance's tensors hold 51)
            setattr(r, f, None)
        rng = np.random.default_rng(s)
        r.dyn = (np.array([r.x + 20.0, 0.5]) + rng.normal(0, 4.0, (8, 1, 2))
                 + np.cumsum(rng.normal(0, 0.1, (8, 65, 2)), axis=1))
        reqs.append(r)
    bp = BatchPlanner(waypoints=WP, **kw)
    results, _ = group_and_wave(bp, reqs, "65 samples", flat=False)
    assert bp.last_eval_form() == "general"
    against_oracle(results, reqs, [kw], [WP], "65 samples")
    bp.close()


def test_a_reused_handle_never_reads_an_earlier_batchs_headers():
    """9, then 1, then 9 instances with other seeds and other lattices on one handle: the table only grows, and a call
    must see nothing of the call before it."""
    dyn, static = obstacles(8)

    def batch(n, seed):
        rng = np.random.default_rng(seed)
        return [PlanRequest(float(rng.uniform(2, 30)), float(rng.uniform(-0.5, 0.5)), 0.01, float(rng.choice([0.05, 3.0, 7.0])),
                            0.1, target_speed=float(rng.choice([0.0, 1.2, 6.0, 15.5])), dyn=dyn if k % 2 else None,
                            static=static) for k in range(n)]

    bp = BatchPlanner(waypoints=WP, **LATTICE)
    for n, seed in ((9, 1), (1, 2), (9, 3)):
        reqs = batch(n, seed)
        results, blobs = group_and_wave(bp, reqs, f"reused handle, {n} instances (seed {seed})")
        against_oracle(results, reqs, [LATTICE], [WP], f"reused handle, {n} instances (seed {seed})")
        fresh = BatchPlanner(waypoints=WP, **LATTICE)
        for path in GROUPED:
            set_eval_path(fresh, path)
            want = fresh.plan_batch(reqs)
            assert took_flat(fresh) == (path == "group")
            for i in range(n):
                assert blobs[i] == rec_bytes(want.records[i]), f"seed {seed} inst {i} [{path}]: a fresh handle gives another record"
        fresh.close()
    bp.close()


def test_candidate_tables_under_the_grouped_cut():
    reqs = []
    for s in range(4):
        r = c3(s)
        for f in ("static", "dyn", "dist"):                     # float64 inputs: the oracle sees the values the device sees
            v = getattr(r, f)
            if v is not None:
                setattr(r, f, np.asarray(v, np.float64))
        reqs.append(r)
    bp = BatchPlanner(waypoints=WP, **syn.CONFIG3_PLANNER)
    wants = [oracle_plan_for_request(orc, orc.make_params(**syn.CONFIG3_PLANNER), orc.Spline(*WP), rq, table=True) for rq in reqs]
    for path in GROUPED:
        set_eval_path(bp, path)
        res = bp.plan_batch(reqs)
        assert bp.last_eval_form() == "lean" and took_flat(bp) == (path == "group"), path
        for i, want in enumerate(wants):
            lab = f"inst {i} [{path}]"
            assert_record_matches_oracle(res.records[i], want, label=lab)
            cost, status, keep, nt = bp.candidates(i)
            np.testing.assert_array_equal(keep, want.cand_keep, err_msg=lab)
            np.testing.assert_allclose(cost, want.cand_cost, rtol=TIGHT, atol=TIGHT, err_msg=lab)
            eps_band.check_status_table(bp, i, status, want.cand_status, lab)
    bp.close()
