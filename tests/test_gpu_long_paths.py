"""Reference paths longer than what the plan kernels stage in LDS, against the oracle (pinned to the reference on such
paths by the `long_*` goldens): k_frenet_state stages a path of at most 512 knots, k_cull one of at most 64, the evaluation
kernels one of at most 28; a longer one is read from HBM through the same SplineView, and in a mixed-scenario batch every
workgroup decides for itself.  The road is tests/long_paths_common.py's: a path of n knots is its first n waypoints.

Everything is held to oracle/check.py as it stands: TIGHT, the crawl rule, the arc length of the nearest point equal bit
for bit; candidate tables through eps_band.check_status_table."""
import collections
from types import SimpleNamespace

import numpy as np
import pytest

import check_paths_common as pc
import eps_band
import long_paths_common as lp
# (the road is a random walk of headings: never exactly straight, so no launch takes a flat kernel -- asserted after each
# plan call -- and helpers' "-noflat" names would repeat "group" and "split-wave")
from helpers import (EVAL_PATHS_NEVER_FLAT as EVAL_PATHS, TIGHT, assert_no_flat_launch, assert_record_matches_oracle,
                     set_eval_path, wrap_angle)
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest
from integrated_path_planning_amd.planner import BatchPlanner
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SIDES = (27, 28, 29, 63, 64, 65, 511, 512, 513, 1500)          # each side of 28 / 64 / 512, and far beyond all of them
MIXED = (20, 28, 29, 64, 65, 512, 513, 1500)                    # scenario k of the mixed handle: a path of MIXED[k] knots


def _planner(n):
    return BatchPlanner(waypoints=lp.road(n), **lp.PLANNER)


def _rec_bytes(rec):
    return bytes(memoryview(rec).cast("B"))


def _check_table(bp, inst, want, label):
    cost, status, keep, nt = bp.candidates(inst)
    assert len(cost) == want.n_cand, label
    np.testing.assert_array_equal(nt, want.cand_nt, err_msg=label)
    np.testing.assert_array_equal(keep, want.cand_keep, err_msg=label)
    np.testing.assert_allclose(cost, want.cand_cost, rtol=TIGHT, atol=TIGHT, err_msg=label)
    eps_band.check_status_table(bp, inst, status, want.cand_status, label)


# ------------------------------------------------------------------------------------------------ a. each side of each limit

@pytest.mark.parametrize("n_knots", SIDES)
def test_each_side_of_each_staging_limit(n_knots):
    pairs = lp.egos(n_knots)
    reqs = [rq for rq, _ in pairs]
    assert sum(w.status == orc.PLAN_OK for _, w in pairs) >= 4              # (most of them plan a path)
    bp = _planner(n_knots)
    first = None
    for path in EVAL_PATHS:
        set_eval_path(bp, path)
        res = bp.plan_batch(reqs)
        assert_no_flat_launch(bp, f"{n_knots} knots [{path}]")
        for i, (_, want) in enumerate(pairs):
            assert_record_matches_oracle(res.records[i], want, label=f"{n_knots} knots, {lp.EGO_KINDS[i]} [{path}]")
        for i in (lp.MID, lp.NEAR_END):
            _check_table(bp, i, pairs[i][1], f"{n_knots} knots, {lp.EGO_KINDS[i]} [{path}]")
        raw = [_rec_bytes(res.records[i]) for i in range(len(reqs))]
        if first is None:
            first = raw
        for i in range(len(reqs)):
            assert raw[i] == first[i], f"{n_knots} knots, {lp.EGO_KINDS[i]}: [{path}] differs from [{EVAL_PATHS[0]}]"
    bp.close()


# ------------------------------------------------------------------------------------------------ b. staged and unstaged in one launch

def _device_records(planner, reqs, mixed):
    """The device entry: float32 obstacles resident in HBM, one call on a torch stream."""
    import torch
    dev = torch.device("cuda", 0)
    pb = PackedBatch(reqs, np.float32)
    dyn = torch.from_numpy(pb.dyn_xy).to(dev)
    stat = torch.from_numpy(pb.static_xy).to(dev)
    out = torch.zeros(len(reqs) * _abi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()                                 # (the uploads and the fill ran on torch's default stream, not on st)
    planner.plan_packed_device(pb.with_device_obstacles(stat.data_ptr(), dyn.data_ptr()), out.data_ptr(), st.cuda_stream,
                               scenario=pb if mixed else None)
    st.synchronize()
    raw = out.cpu().numpy().tobytes()
    return [raw[j * _abi.RESULT_BYTES:(j + 1) * _abi.RESULT_BYTES] for j in range(len(reqs))]


@pytest.fixture(scope="module")
def singles():
    """What a handle of each path alone gives for its eight egos: [scenario][ego] record bytes, float64 obstacles through
    the host entry and float32 obstacles through the device entry."""
    host, device = [], []
    for n in MIXED:
        bp = _planner(n)
        reqs = [rq for rq, _ in lp.egos(n)]
        res = bp.plan_batch(reqs)
        host.append([_rec_bytes(res.records[i]) for i in range(len(reqs))])
        device.append(_device_records(bp, reqs, False))
        bp.close()
    return host, device


@pytest.fixture(scope="module")
def mixed_handle():
    bp = _planner(MIXED[0])
    for k, n in enumerate(MIXED[1:], start=1):
        assert bp.add_scenario(waypoints=lp.road(n), **lp.PLANNER) == k
    yield bp
    bp.close()


def _mixed_requests(combos):
    """combos: (scenario, ego) pairs -> requests (copies: the scenario id is the request's)."""
    import dataclasses
    return [dataclasses.replace(lp.egos(MIXED[k])[e][0], scenario=k) for k, e in combos]


# k_evaluate's queue x serves the instances x, x + 8, ... (one queue per XCD) and the waves of a workgroup take
# neighbouring entries of ONE queue.  Scenarios cycling 0..7 therefore leave every k_evaluate workgroup on one scenario
# (staged or not as a whole) while k_frenet_state's and k_cull's neighbouring workgroups alternate; sorted by scenario,
# the waves of a k_evaluate workgroup are on different scenarios and nothing is staged; the shuffled batch has both.
_CYCLE = [(i % 8, i // 8) for i in range(64)]
BATCHES = {
    "cycling": _CYCLE,
    "sorted": sorted(_CYCLE),
    "shuffled": [_CYCLE[i] for i in np.random.default_rng(64).permutation(64)],
    "none_fits": [c for c in _CYCLE if c[0] in (6, 7)],         # 513 + 1500 knots: 0 bytes of dynamic LDS for the spline
    "eval_split": [c for c in _CYCLE if c[0] in (1, 2)],        # 28 staged by the evaluation, 29 in HBM
    "cull_split": [c for c in _CYCLE if c[0] in (3, 4)],        # 64 / 65: the same for k_cull
    "frenet_split": [c for c in _CYCLE if c[0] in (5, 6)],      # 512 / 513: the same for k_frenet_state
}


@pytest.mark.parametrize("eval_path", EVAL_PATHS)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_staged_and_unstaged_paths_in_one_launch(mixed_handle, singles, batch, eval_path):
    combos = BATCHES[batch]
    bp = mixed_handle
    set_eval_path(bp, eval_path)
    res = bp.plan_batch(_mixed_requests(combos))
    assert_no_flat_launch(bp, f"{batch} [{eval_path}]")
    for i, (k, e) in enumerate(combos):
        assert _rec_bytes(res.records[i]) == singles[0][k][e], f"{batch} [{eval_path}] instance {i}: {MIXED[k]} knots, {lp.EGO_KINDS[e]}"
    if batch in ("cycling", "sorted"):                                      # one instance per scenario against the oracle's table
        for i, (k, e) in enumerate(combos):
            if e == lp.MID:
                _check_table(bp, i, lp.egos(MIXED[k])[e][1], f"mixed {MIXED[k]} knots [{eval_path}]")


@pytest.mark.parametrize("eval_path", EVAL_PATHS)
def test_mixed_batch_of_400_through_the_device_entry(mixed_handle, singles, eval_path):
    """400 instances over the eight scenarios (`auto` leaves the split kernel), float32 obstacles in HBM, a torch stream."""
    combos = [_CYCLE[(i * 37) % 64] for i in range(400)]
    set_eval_path(mixed_handle, eval_path)
    got = _device_records(mixed_handle, _mixed_requests(combos), True)
    assert_no_flat_launch(mixed_handle, f"400 instances [{eval_path}]")
    n_ok = 0
    for i, (k, e) in enumerate(combos):
        assert got[i] == singles[1][k][e], f"[{eval_path}] instance {i}: {MIXED[k]} knots, {lp.EGO_KINDS[e]}"
        n_ok += _abi.Result.from_buffer_copy(got[i]).status == _abi.PLAN_OK
    assert n_ok > 200


# ------------------------------------------------------------------------------------------------ c. the helpers on 1500 knots

N_LONG = 1500


@pytest.fixture(scope="module")
def long_planner():
    bp = _planner(N_LONG)
    yield bp
    bp.close()


def _frenet_states_match(bp, sp, egos_):
    fr, ref, nps, ok = bp.frenet_states(egos_)
    for i, rq in enumerate(egos_):
        rc, wfr, wref, ws = orc.cartesian_to_frenet_state(sp, orc.make_ego(rq.x, rq.y, rq.yaw, rq.v, rq.a, rq.last_kappa, rq.prev_s))
        label = f"ego {i} (prev_s {rq.prev_s})"
        assert bool(ok[i]) == (rc == 0), label
        assert nps[i] == ws, f"{label}: arc length {nps[i]!r} != oracle's {ws!r}"
        if rc == 0:
            np.testing.assert_allclose(fr[i], wfr, rtol=TIGHT, atol=TIGHT, err_msg=label)
            np.testing.assert_allclose(np.delete(ref[i], 3), np.delete(wref, 3), rtol=TIGHT, atol=TIGHT, err_msg=label)
            assert abs(wrap_angle(ref[i][3] - wref[3])) <= TIGHT, label
    return nps


def test_frenet_state_batch_over_the_whole_path(long_planner):
    """512 egos spread over 3.7 km, up to 3 m beside the path; the cached arc length absent, right, 9.9995 m off (the true
    point just inside the window's far edge) and 10.5 m off (outside it)."""
    sp, s_end = lp.spline(N_LONG)
    rng = np.random.default_rng(512)
    s_true = np.sort(rng.uniform(0.0, s_end, 512))
    egos_ = []
    for i, s in enumerate(s_true):
        x, y, yaw = lp.pose_at(sp, s, float(rng.uniform(-3.0, 3.0)))
        prev = (None, float(s), float(s - 9.9995), float(s + 10.5))[i % 4]
        egos_.append(PlanRequest(x, y, yaw + float(rng.normal(0.0, 0.05)), float(rng.uniform(0.0, 8.0)), float(rng.normal(0.0, 0.5)),
                                 last_kappa=float(rng.normal(0.0, 0.01)), prev_s=prev))
    nps = _frenet_states_match(long_planner, sp, egos_)
    assert np.median(np.abs(nps - s_true)) < 0.5 and nps.max() > 0.99 * s_end and nps.min() < 0.01 * s_end


def test_window_cut_short_by_the_start_of_the_path(long_planner):
    """A cached arc length of -9.5 m leaves a window [0, 0.5 m] whose 100 samples are 5 mm apart: the last but one is
    within a centimetre of the edge and still no edge (the fallback's 1e-3).  An ego on the normal through that sample
    but hundreds of metres away -- nearer to a later part of the road -- keeps the window's answer, as the reference's
    search does; the global scan would have found the other place."""
    sp, s_end = lp.spline(N_LONG)
    s98 = 0.5 * 98.0 / 99.0
    far = []
    for d in (-900.0, -600.0, -400.0, -250.0, 250.0, 400.0, 600.0, 900.0):
        x, y, yaw = lp.pose_at(sp, s98, d)
        far.append(PlanRequest(x, y, yaw, 3.0, 0.0, prev_s=-9.5))
    nps = _frenet_states_match(long_planner, sp, far)
    assert np.all(nps < 1.0)
    free = [PlanRequest(r.x, r.y, r.yaw, r.v, r.a) for r in far]            # the same egos without the cache: elsewhere
    assert np.sum(_frenet_states_match(long_planner, sp, free) > 50.0) >= 2


def _status_probes(want):
    """The selected candidate and the first candidate of every status of the oracle's table."""
    idx = collections.OrderedDict()
    if want.best_index >= 0:
        idx[int(want.best_index)] = "selected"
    for st in sorted(set(want.cand_status.tolist())):
        idx.setdefault(int(np.flatnonzero(want.cand_status == st)[0]), orc.STATUS_NAMES[st] if st < 8 else "dropped")
    return idx


def _assert_path_matches(got, arr, n, label):
    from oracle.check import CRAWL_C_TOL, CRAWL_S_DOT
    for fi, f in enumerate(orc.PATH_FIELDS):
        g, w = np.array(getattr(got, f))[:n], arr[fi, :n]
        if f == "yaw":
            np.testing.assert_allclose(wrap_angle(g - w), 0.0, atol=TIGHT, err_msg=f"{label} {f}")
        elif f == "c":
            loose = np.where(np.abs(arr[orc.PATH_FIELDS.index("s_d"), :n]) < CRAWL_S_DOT, CRAWL_C_TOL, 0.0)
            assert np.all(np.abs(g - w) <= TIGHT + TIGHT * np.abs(w) + loose), f"{label} {f}"
        else:
            np.testing.assert_allclose(g, w, rtol=TIGHT, atol=TIGHT, err_msg=f"{label} {f}")


def test_debug_candidate_path_and_external_checks(long_planner):
    """fot_debug_candidate_path of the selected candidate and of one candidate per status against the oracle's probe
    path, and three oracle candidate paths through fot_check_paths / fot_check_collision_paths against the restatement
    of the reference's checks (as tests/test_gpu_check_paths_fuzz.py calls it)."""
    sp, _ = lp.spline(N_LONG)
    params = orc.make_params(**lp.PLANNER)
    rq, want = lp.egos(N_LONG)[lp.MID]
    long_planner.set_tile_cut(0); long_planner.set_eval_segments(0)
    long_planner.plan_batch([rq])
    probes = _status_probes(want)
    assert len(probes) >= 4, probes
    paths = {}
    for idx, name in probes.items():
        keep, arr, _ = orc.candidate_path(params, sp, want.frenet0, rq.target_speed, idx)
        assert keep == want.cand_keep[idx]
        got = long_planner.candidate_path(idx)
        assert len(got.x) >= keep, name
        _assert_path_matches(got, arr, keep, f"candidate {idx} ({name})")
        paths[idx] = {f: arr[orc.PATH_FIELDS.index(f), :keep].tolist() for f in pc.FIELDS}
    # the selected path, the last colliding candidate and the first one beyond the curvature limit
    hit = int(np.flatnonzero(want.cand_status == pc.COLLISION)[-1])
    keep, arr, _ = orc.candidate_path(params, sp, want.frenet0, rq.target_speed, hit)
    paths[hit] = {f: arr[orc.PATH_FIELDS.index(f), :keep].tolist() for f in pc.FIELDS}
    three = [int(want.best_index), hit, int(np.flatnonzero(want.cand_status == pc.CURV)[0])]
    cfg = pc.cfg(**{k: lp.PLANNER[k] for k in ("max_speed", "max_accel", "max_curvature", "max_lat_accel", "dt",
                                              "max_road_width", "robot_radius", "obstacle_radius")})
    cl = pc.call(cfg, [paths[i] for i in three], static=rq.static, dist=rq.dist, name="oracle paths on 1500 knots")
    want_cat, want_free, margin = pc.evaluate(cl)
    assert margin.min() >= pc.BAND
    objs = [SimpleNamespace(**p) for p in cl["paths"]]
    cat = long_planner.check_paths(objs, cl["static"], None, None, cl["dist"], None)
    free = long_planner.paths_collision_free(objs, cl["static"], None, cl["dist"])
    assert np.asarray(cat, int).tolist() == want_cat.tolist()
    assert np.asarray(free, bool).tolist() == want_free.tolist()
    # ... and the restatement agrees with what the oracle's planner decided about its own candidates
    assert want_cat.tolist() == [int(want.cand_status[i]) for i in three] == [pc.OK, pc.COLLISION, pc.CURV]
    assert want_free.tolist() == [True, False, False]


def test_wire_form_of_records_kilometres_along_the_path(long_planner):
    """pack_records_host -> unpack_records of the records of part a at 1500 knots (s up to ~3.7 km): the header bit for
    bit, the samples at the tolerance of test_wire_records_far_from_the_origin_and_sharded_planner."""
    from integrated_path_planning_amd.distributed import pack_records_host, unpack_records
    reqs = [rq for rq, _ in lp.egos(N_LONG)]
    res = long_planner.plan_batch(reqs)
    nt = long_planner.n_total_samples
    back = unpack_records(pack_records_host(res.records, len(reqs), nt), len(reqs), nt)
    assert max(res.records[i].s[0] for i in range(len(reqs)) if res.records[i].status == _abi.PLAN_OK) > 3000.0
    for i in range(len(reqs)):
        a, b = res.records[i], back[i]
        assert (a.status, a.best_index, a.n_cand, a.n_keep, a.cost) == (b.status, b.best_index, b.n_cand, b.n_keep, b.cost)
        assert list(a.stats) == list(b.stats) and a.new_last_kappa == b.new_last_kappa
        assert a.new_prev_s == b.new_prev_s or (np.isnan(a.new_prev_s) and np.isnan(b.new_prev_s))
        assert list(a.frenet0) == list(b.frenet0) and list(a.ref0) == list(b.ref0)
        for f in _abi.PATH_FIELDS:
            np.testing.assert_allclose(np.array(getattr(b, f)[: a.n_keep]), np.array(getattr(a, f)[: a.n_keep]),
                                       rtol=2.0 ** -23, atol=1e-5 if f in ("s", "x", "y") else 1e-30, err_msg=f"{i} {f}")
