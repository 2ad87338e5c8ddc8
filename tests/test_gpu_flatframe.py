"""The flat form of the lean evaluation kernels (k_evaluate_group_lean_flat, k_evaluate_split_lean_flat) on the GPU, against
the lean form it replaces.

`BatchPlanner.set_flat(0)` keeps a handle's launches on the kernels every other test runs, `set_flat(1)` (the default)
lets a lean-eligible launch whose every path is exactly straight take the flat form, and the call's return value tells
whether the most recent plan call launched one.  Every case of tests/flatframe_common.py is planned both ways:

  * records byte-identical, per-candidate tables (cost, status, keep, n_t) equal, under both tile cuts and with the
    walk in one piece and cut into 2 and 3 time segments, in batches of 1 to 8 -- the grouped and the split kernel have
    a flat form, the per-wave kernel (per-wave cut, one piece) has none: such a launch reports "no flat launch";
  * flat paths equal the oracle;
  * the rotated and the curved path, and a handle with synthetic.SCENARIO_PLANNERS' three scenarios in one call (its
    third path is curved), report "no flat launch";
  * non-finite egos give the records of set_flat(0).
"""
import ctypes as C

import numpy as np
import pytest

import eps_band
import flatframe_common as ff
from helpers import TIGHT, assert_record_matches_oracle, oracle_plan_for_request
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.batch import PlanRequest
from integrated_path_planning_amd.planner import BatchPlanner
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

PATHS = {p.name: p for p in ff.paths()}
# (tile cut, time segments): k_evaluate_group / k_evaluate with the walk in one piece, k_evaluate_split with 2 and 3
# segments under either cut; "auto" is what a caller gets
FORMS = [(0, 0), (2, 1), (1, 1), (1, 2), (2, 2), (1, 3), (2, 3)]
BATCHES = (1, 2, 3, 4, 8)


def has_flat_kernel(cut, seg):
    """the launch shape of a batch of at most 8 instances: "auto" cuts it into time segments; the per-wave cut walked in
    one piece is k_evaluate_lean, which has no flat form"""
    return not (cut == 1 and seg == 1)


def rec_bytes(rec):
    return bytes(memoryview(rec).cast("B"))


def plan(bp, reqs, on, **kw):
    bp.set_flat(on)
    res = bp.plan_batch(reqs, **kw)
    took = bp.set_flat(-1)
    tabs = [bp.candidates(i) for i in range(len(reqs))]
    bp.set_flat(1)
    return res, tabs, took


def both(bp, reqs, label, expect_flat, **kw):
    flat, t_flat, took = plan(bp, reqs, 1, **kw)
    assert took == expect_flat, f"{label}: flat launch {took}, expected {expect_flat}"
    assert bp.last_eval_form() == "lean", f"{label}: a flat launch reports as lean ({bp.last_eval_form()})"
    lean, t_lean, took0 = plan(bp, reqs, 0, **kw)
    assert not took0, f"{label}: set_flat(0) still launched a flat kernel"
    for i in range(len(reqs)):
        assert rec_bytes(flat.records[i]) == rec_bytes(lean.records[i]), f"{label} inst {i}: records differ"
        for name, x, y in zip(("cost", "status", "keep", "n_t"), t_flat[i], t_lean[i]):
            np.testing.assert_array_equal(x, y, err_msg=f"{label} inst {i}: {name}")
    return flat


def chunks(reqs):
    out, at = [], 0
    for n in BATCHES:
        out.append([reqs[(at + j) % len(reqs)] for j in range(n)])
        at += n
    return out


@pytest.fixture(scope="module")
def oracle_wants():
    """the oracle's plan of every case on a flat path, computed once"""
    cache = {}

    def want(case):
        if case.name not in cache:
            cache[case.name] = oracle_plan_for_request(orc, orc.make_params(**case.kw), orc.Spline(*case.path.waypoints),
                                                       case.req, table=True)
        return cache[case.name]
    return want


@pytest.mark.parametrize("path", sorted(PATHS))
def test_flat_launch_equals_the_lean_launch(path, oracle_wants):
    p = PATHS[path]
    cs = ff.cases(path_names=(path,))
    for kw in (ff.KW, ff.ODD_KW):
        mine = [c for c in cs if c.kw is kw]
        reqs = [c.req for c in mine]
        bp = BatchPlanner(waypoints=p.waypoints, **kw)
        for cut, seg in FORMS:
            bp.set_tile_cut(cut)
            bp.set_eval_segments(seg)
            for batch in chunks(reqs):
                both(bp, batch, f"{path} [cut {cut}, {seg} segments, {len(batch)} instances]", p.flat and has_flat_kernel(cut, seg))
        if kw is ff.ODD_KW:
            assert all(bp.plan_batch([r]).records[0].n_cand % 64 for r in reqs), f"{path}: the odd lattice is a multiple of 64"
        if p.flat:                                           # the flat launch against the oracle (grouped cut, one piece)
            bp.set_tile_cut(2)
            bp.set_eval_segments(1)
            res, tabs, took = plan(bp, reqs, 1)
            assert took
            for i, c in enumerate(mine):
                want = oracle_wants(c)
                assert_record_matches_oracle(res.records[i], want, label=c.name)
                cost, status, keep, nt = tabs[i]
                np.testing.assert_array_equal(keep, want.cand_keep, err_msg=c.name)
                np.testing.assert_allclose(cost, want.cand_cost, rtol=TIGHT, atol=TIGHT, err_msg=c.name)
                eps_band.check_status_table(bp, i, status, want.cand_status, c.name)
        bp.close()


def test_float32_tensors_and_the_smoke_batch():
    """config 3 with float32 tensors on the benchmark's path: four instances, as smoke() plans them"""
    from helpers import request_from_instance
    bp = BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), **syn.CONFIG3_PLANNER)
    reqs = [request_from_instance(syn.config3_instance(s, S=20, P=30)) for s in range(8)]
    for cut, seg in FORMS:
        bp.set_tile_cut(cut)
        bp.set_eval_segments(seg)
        both(bp, reqs, f"config 3 float32 [cut {cut}, {seg} segments]", has_flat_kernel(cut, seg), obstacle_dtype=np.float32)
    bp.close()


def test_three_scenarios_in_one_call_stay_on_the_lean_kernels():
    """synthetic.SCENARIO_PLANNERS: two straight paths and a curved one on one handle.  A call that uses all three is not
    flat; a call on the two straight ones is; eligibility follows the paths a launch uses, not the handle's."""
    (wp0, kw0), *rest = syn.SCENARIO_PLANNERS
    bp = BatchPlanner(waypoints=wp0, **kw0)
    for k, (wp, kw) in enumerate(rest, start=1):
        assert bp.add_scenario(waypoints=wp, **kw) == k
    reqs = []
    for k in range(3):
        for ego in ("on_path", "ladder"):
            _, r = ff.request(PATHS["curved" if k == 2 else "x_even"], ego)
            reqs.append(PlanRequest(**{**r.__dict__, "scenario": k}))
    for cut, seg in ((1, 2), (2, 1), (0, 0)):
        bp.set_tile_cut(cut)
        bp.set_eval_segments(seg)
        both(bp, reqs, f"three scenarios [cut {cut}, {seg} segments]", False)
        both(bp, reqs[:4], f"the two straight scenarios [cut {cut}, {seg} segments]", True)
        both(bp, reqs[4:], f"the curved scenario alone [cut {cut}, {seg} segments]", False)
    bp.close()


def test_the_flag_follows_the_path_through_every_route():
    """waypoints, coefficients, and a path replaced on a live handle"""
    flat, curved = PATHS["offset"], PATHS["curved"]
    _, rq = ff.request(flat, "beside")
    bp = BatchPlanner(waypoints=flat.waypoints, **ff.KW)
    both(bp, [rq], "waypoints", True)
    coef = bp.path_coeffs()
    bp.set_waypoints(*curved.waypoints)
    both(bp, [ff.request(curved, "beside")[1]], "replaced by a curved path", False)
    dp = C.POINTER(C.c_double)
    arrs = [np.ascontiguousarray(a) for a in coef]
    _abi.check(bp._h, bp._lib.fot_set_path_coeffs(bp._h, len(arrs[0]), *[a.ctypes.data_as(dp) for a in arrs]))
    both(bp, [rq], "coefficients", True)
    arrs[7][len(arrs[7]) - 2] = 1e-300                       # one non-zero second-derivative coefficient of y, last segment
    _abi.check(bp._h, bp._lib.fot_set_path_coeffs(bp._h, len(arrs[0]), *[a.ctypes.data_as(dp) for a in arrs]))
    both(bp, [rq], "one non-zero coefficient", False)
    bp.close()


@pytest.mark.parametrize("path", ["x_even", "y_offset", "reversed"])
def test_non_finite_egos_give_the_lean_records(path):
    p = PATHS[path]
    kw, named = ff.nonfinite_requests(p)
    bp = BatchPlanner(waypoints=p.waypoints, **kw)
    reqs = [r for _, r in named]
    for cut, seg in ((2, 1), (0, 0), (1, 3)):
        bp.set_tile_cut(cut)
        bp.set_eval_segments(seg)
        for i in range(0, len(reqs), 8):
            both(bp, reqs[i:i + 8], f"{path} non-finite [{named[i][0]} ...; cut {cut}, {seg} segments]", True)
    bp.close()
