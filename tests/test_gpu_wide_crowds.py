"""Wide-sample launches (65 .. 254 samples, a raised sample capacity) against crowds, statics, NaN tracks and the radius.

tests/test_gpu_wide_samples.py counts: two pedestrians, hits deep inside the radius, no static obstacle, full tracks.
Here the wide kernels -- k_evaluate{,_split,_group}_wide, their _lean_wide forms, k_check_ext_wide -- get the differential
coverage the narrow ones have in test_gpu_fuzz.py, test_gpu_limits.py and test_gpu_collision_boundary.py, against the
oracle and check_paths_common's NumPy restatement (never against the library itself, except where byte-identity of two
launch shapes is the claim).  tests/wide_crowds_common.py builds the instances, tests/test_wide_crowds_cpu.py proves
their premises without a GPU.  Every test builds its handles with sample_capacity=254, runs PATHS, and asserts the
evaluation form and that no flat kernel ran after every plan call; tables must EQUAL the oracle's.

  1  the wide crowd fuzz: 12 selected instances on 4 handles under every launch shape, lean-wide and general-wide
     launches, time-major and float32 tensors, the HBM-resident entry point
  2  permutations of the sample axis: every table and record byte-identical
  3  k_cull's caches above 64 samples: NaN tracks beyond every cache, 5200 points per step with a budget
  4  the collision radius: `dist`, `mixed` and `footprint3` kinds of test_gpu_collision_boundary.py with wide tensors
  5  a dense wide instance in company of narrow ones in one mixed-scenario launch
  6  the external-path checkers on raised engines against check_paths_common
"""
import numpy as np
import pytest

import check_paths_common as cp
import eps_band
import wide_crowds_common as wc
from helpers import EVAL_PATHS_NEVER_FLAT, TIGHT, assert_no_flat_launch, assert_record_matches_oracle, set_eval_path
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest
from integrated_path_planning_amd.footprint import EgoFootprint
from integrated_path_planning_amd.planner import BatchPlanner
from oracle import oracle as orc
from oracle.check import oracle_plan_for_request
from test_gpu_collision_boundary import DELTAS, MG_COLLISION, Replay, Scene, isolated, rounded32
from test_gpu_wide_samples import rec_bytes, set_path

pytestmark = pytest.mark.gpu

PATHS = EVAL_PATHS_NEVER_FLAT + ("wave-2", "wave-3")
CAPACITY = _abi.MAX_PLAN_SAMPLES


def check_tables(bp, res, slot, want, lab):
    """the library's candidate tables and record of instance `slot` of the last call EQUAL the oracle's"""
    cost, status, keep, nt = bp.candidates(slot)
    assert len(status) == want.n_cand, lab
    np.testing.assert_array_equal(nt, want.cand_nt, err_msg=lab)
    np.testing.assert_array_equal(keep, want.cand_keep, err_msg=lab)
    eps_band.check_status_table(bp, slot, status, want.cand_status, lab)
    np.testing.assert_allclose(cost, want.cand_cost, rtol=TIGHT, atol=TIGHT, err_msg=lab)
    assert_record_matches_oracle(res.records[slot], want, label=lab)


def table_bytes(bp, slot):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in bp.candidates(slot))


def plan_resident(bp, pb):
    """the records of plan_packed_device on tensors that lie in HBM already (tests/test_gpu_fuzz.py's call)"""
    import torch
    dev = torch.device("cuda", 0)
    st_t = torch.from_numpy(pb.static_xy).to(dev) if pb.static_xy.size else None
    dy_t = torch.from_numpy(pb.dyn_xy).to(dev) if pb.dyn_xy.size else None
    out_t = torch.zeros(pb.n * _abi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    bp.plan_packed_device(pb.with_device_obstacles(st_t.data_ptr() if st_t is not None else None,
                                                   dy_t.data_ptr() if dy_t is not None else None),
                          out_t.data_ptr(), stream.cuda_stream, scenario=pb if pb.mixed else None)
    stream.synchronize()
    return out_t.cpu().numpy().tobytes()


class Handle:
    """A raised handle of one wide_crowds_common.CrowdHandle: a scenario per distinct eps of the instances given."""

    def __init__(self, h, insts, sample_capacity=CAPACITY, extra_eps=()):
        self.h, self.insts = h, list(insts)
        self.eps = list(dict.fromkeys([i.eps for i in self.insts] + list(extra_eps)))
        self.bp = BatchPlanner(waypoints=h.waypoints, sample_capacity=sample_capacity, **h.planner_kw(self.eps[0]))
        for k, e in enumerate(self.eps[1:], start=1):
            assert self.bp.add_scenario(waypoints=h.waypoints, **h.planner_kw(e)) == k
        self.reqs = [self.req(i.req, i.eps) for i in self.insts]

    def req(self, rq, eps):
        return PlanRequest(**{**rq.__dict__, "scenario": self.eps.index(eps)})

    def launches(self):
        """the instances as the launches they go out in: the lean-eligible ones together, and the others"""
        lean = [k for k, i in enumerate(self.insts) if i.lean_eligible]
        rest = [k for k in range(len(self.insts)) if k not in lean]
        return [(form, idx) for form, idx in (("lean-wide", lean), ("general-wide", rest)) if idx]

    def plan(self, reqs, form, lab, **packed):
        res = self.bp.plan_packed(PackedBatch(reqs, **packed)) if packed else self.bp.plan_batch(reqs)
        assert self.bp.last_eval_form() == form, f"{lab}: {self.bp.last_eval_form()}"
        assert_no_flat_launch(self.bp, lab)
        return res

    def restore(self):
        set_eval_path(self.bp, "auto")


@pytest.fixture(scope="module")
def crowd_handles():
    made = {}

    def get(k):
        if k not in made:
            made[k] = Handle(*wc.handles()[k])
        return made[k]
    yield get
    for h in made.values():
        h.restore()
        h.bp.close()


# ---- 1 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(wc.N_HANDLES))
def test_wide_crowds_match_the_oracle(crowd_handles, k):
    h = crowd_handles(k)
    assert h.bp.sample_capacity == CAPACITY and len(h.insts) == wc.PER_HANDLE
    launches = h.launches()
    if k == 0:
        assert launches[0][0] == "lean-wide" and len(launches[0][1]) >= 2
    plain = {}
    try:
        for path in PATHS:
            set_path(h.bp, path)
            for form, idx in launches:
                res = h.plan([h.reqs[i] for i in idx], form, f"{h.h.name} [{path}]")
                for slot, i in enumerate(idx):
                    lab = f"{h.insts[i].label()} [{path}]"
                    check_tables(h.bp, res, slot, h.insts[i].want, lab)
                    b = rec_bytes(res.records[slot])
                    assert plain.setdefault(i, b) == b, f"{lab}: record differs from [{PATHS[0]}]"
        for path in ("group", "split-wave"):
            set_eval_path(h.bp, path)
            for form, idx in launches:
                reqs = [h.reqs[i] for i in idx]
                lab = f"{h.h.name} [{path}"
                tsp = h.plan(reqs, form, lab + ", float64 time-major]", obstacle_dtype=np.float64, dyn_layout_tsp=True)
                for slot, i in enumerate(idx):
                    assert rec_bytes(tsp.records[slot]) == plain[i], f"{h.insts[i].label()} [{path}]: time-major record differs"
                f32t = bytes(h.plan(reqs, form, lab + ", float32 time-major]", obstacle_dtype=np.float32, dyn_layout_tsp=True).records)
                f32 = h.plan(reqs, form, lab + ", float32]", obstacle_dtype=np.float32)
                assert bytes(f32.records) == f32t, f"{lab}]: time-major float32 layout changes the records"
                for slot, i in enumerate(idx):      # float32 tensors: the oracle on the rounded inputs
                    check_tables(h.bp, f32, slot, h.insts[i].want32, f"{h.insts[i].label()} [{path}, float32]")
                got = plan_resident(h.bp, PackedBatch(reqs, np.float64))
                assert h.bp.last_eval_form() == form
                assert got == b"".join(plain[i] for i in idx), f"{lab}]: the resident entry point differs"
    finally:
        h.restore()


# ---- 2 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(wc.N_HANDLES))
def test_the_sample_order_does_not_matter(crowd_handles, k):
    """The reference counts DISTINCT samples: the distribution rolled by 1, 63 and 64 along the sample axis, reversed and
    under a fixed random permutation gives byte-identical tables and records.  Every hit moves across the word edges."""
    h = crowd_handles(k)
    try:
        for path in ("group", "split-wave"):
            set_eval_path(h.bp, path)
            for inst, rq in zip(h.insts, h.reqs):
                perms = wc.permutations(inst.S)
                reqs = [rq] + [h.req(wc.permuted(inst, p), inst.eps) for p in perms.values()]
                form = "lean-wide" if inst.lean_eligible else "general-wide"
                res = h.plan(reqs, form, f"{inst.label()} [{path}]")
                check_tables(h.bp, res, 0, inst.want, f"{inst.label()} [{path}]")
                first = (table_bytes(h.bp, 0), rec_bytes(res.records[0]))
                for slot, name in enumerate(perms, start=1):
                    assert (table_bytes(h.bp, slot), rec_bytes(res.records[slot])) == first, f"{inst.label()} [{path}, {name}]"
    finally:
        h.restore()


# ---- 3 ----------------------------------------------------------------------------------------------------------------

def _limits_check(bp, reqs, wants, form, lab):
    res = bp.plan_batch(reqs)
    assert bp.last_eval_form() == form, f"{lab}: {bp.last_eval_form()}"
    assert_no_flat_launch(bp, lab)
    for i, want in enumerate(wants):
        check_tables(bp, res, i, want, f"{lab} inst {i}")
    return res


@pytest.mark.parametrize("S,P,n_block,n_extra,high_only,label", wc.NAN_CASES, ids=[f"S{c[0]}-P{c[1]}" for c in wc.NAN_CASES])
def test_nan_tracks_beyond_every_cache_of_the_lazy_check_wide(S, P, n_block, n_extra, high_only, label):
    """tests/test_gpu_limits.py's test at sample ids j / P >= 64: the NaN tracks are no obstacles (fewer collisions than
    on the clean tensor), in every layout, dtype and through the resident entry point."""
    reqs, _ = wc.nan_cache_case(S, P, n_block, n_extra, high_only)
    wants = wc.limits_oracle(wc.NAN_KW, reqs)
    bp = BatchPlanner(waypoints=(wc.LIMITS_WX, wc.LIMITS_WY), sample_capacity=CAPACITY, **wc.NAN_KW)
    try:
        for path in PATHS:
            set_path(bp, path)
            res = _limits_check(bp, reqs, wants, "lean-wide", f"{label} [{path}]")
            assert res.records[0].stats[_abi.ST_COLLISION] < res.records[2].stats[_abi.ST_COLLISION], label
        set_eval_path(bp, "auto")
        for dtype in (np.float32, np.float64):
            spt = bp.plan_packed(PackedBatch(reqs, dtype))
            assert bp.last_eval_form() == "lean-wide"
            tsp = bp.plan_packed(PackedBatch(reqs, dtype, dyn_layout_tsp=True))
            assert bytes(spt.records) == bytes(tsp.records), label
            if dtype is np.float64:
                assert bytes(spt.records) == bytes(res.records), label
            for tsp_layout in (False, True):
                got = plan_resident(bp, PackedBatch(reqs, dtype, dyn_layout_tsp=tsp_layout))
                assert got == bytes(spt.records)[: len(got)], f"{label} (resident, time-major {tsp_layout}, {dtype.__name__})"
    finally:
        bp.close()


def test_distribution_larger_than_cull_cache_with_budget_wide():
    """200 samples x 26 pedestrians = 5200 points per step, eps = 0.1 (20 violating samples allowed), 3-circle footprint"""
    reqs = wc.cull_cache_case()
    wants = wc.limits_oracle(wc.CULL_KW, reqs, wc.CULL_FOOTPRINT)
    bp = BatchPlanner(waypoints=(wc.LIMITS_WX, wc.LIMITS_WY), footprint=wc.CULL_FOOTPRINT, sample_capacity=CAPACITY, **wc.CULL_KW)
    try:
        for path in PATHS:
            set_path(bp, path)
            _limits_check(bp, reqs, wants, "general-wide", f"cull cache [{path}]")
    finally:
        bp.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------

def scene_params(sc, **over):
    """the oracle's parameters of a boundary scene with some of them replaced"""
    okw = dict(sc.kw, **over)
    fp = okw.pop("footprint", None)
    if fp is not None:
        okw["footprint_offsets"], okw["footprint_radius"] = list(fp.offsets), fp.radius
    return orc.make_params(**okw)


FOOTPRINT3 = EgoFootprint.multi_circle(4.6, 1.9, 3)
BOUNDARY_CASES = [(scene, "dist", S, dict(chance_epsilon=eps)) for scene in ("arc30", "far", "long") for S in (65, 129, 254)
                  for eps in (0.0, 0.1)]
BOUNDARY_CASES += [("arc30", "mixed", 65, dict(chance_epsilon=1.0, collision_margin_inflation=1.2)),
                   ("far", "mixed", 129, dict(chance_epsilon=1.0, collision_margin_inflation=1.2)),
                   ("long", "mixed", 254, dict(chance_epsilon=1.0, collision_margin_inflation=1.2)),
                   ("far", "footprint3", 254, dict(chance_epsilon=0.1, footprint=FOOTPRINT3))]


@pytest.mark.parametrize("scene,kind,S,extra", BOUNDARY_CASES,
                         ids=[f"{s}-{k}-S{S}-eps{e['chance_epsilon']}" for s, k, S, e in BOUNDARY_CASES])
def test_boundary_obstacles_match_the_oracle_wide(scene, kind, S, extra):
    """test_gpu_collision_boundary.test_boundary_obstacles_match_the_oracle with wide tensors: its DELTAS, floors and
    judges A, C and D; wide_crowds_common.THIN states the thinning."""
    assert len(DELTAS) == 14
    sc = Scene(scene, extra, sample_capacity=CAPACITY)
    try:
        assert sc.bp.sample_capacity == CAPACITY and (sc.n_t > 64) == (scene == "long")
        build = {"dist": wc.kind_dist_wide, "mixed": wc.kind_mixed_wide, "footprint3": wc.kind_footprint_wide}[kind]
        reqs, meta = build(sc, S)
        assert len(reqs) >= 6
        wants = [oracle_plan_for_request(orc, sc.params, sc.sp, rq, table=True) for rq in reqs]
        wants32 = [oracle_plan_for_request(orc, sc.params, sc.sp, rounded32(rq), table=True) for rq in reqs]
        changed = sum(int((w.cand_status != sc.free.cand_status).any()) for w in wants)
        assert changed >= len(reqs) // 5, f"{scene}/{kind}: only {changed} of {len(reqs)} instances change a status"
        if kind == "mixed":       # the distribution is wholly forgiven: without the static obstacle nothing collides
            for rq in reqs[:2]:
                alone = oracle_plan_for_request(orc, sc.params, sc.sp, sc.request(dist=rq.dist), table=True)
                np.testing.assert_array_equal(alone.cand_status, sc.free.cand_status)
                hard = oracle_plan_for_request(orc, scene_params(sc, chance_epsilon=0.0), sc.sp, sc.request(dist=rq.dist), table=True)
                assert (hard.cand_status != sc.free.cand_status).any()       # ... and at eps = 0 it does
        # the launch rule of csrc/fot_host.cpp: lean where no instance has a budget, at most 64 steps, no footprint
        lean = wc.max_viol(sc.kw.get("chance_epsilon", 0.0), S) == 0 and sc.n_t <= 64 and "footprint" not in sc.kw
        form = "lean-wide" if lean else "general-wide"
        assert lean == (kind == "dist" and extra["chance_epsilon"] == 0.0 and scene != "long")
        judge_c = [[t for t in ts if isolated(sc, rq, t)] for rq, ts in zip(reqs, meta)]
        eligible = sum(t.own_radius and abs(t.delta) <= 1e-3 for ts in meta for t in ts)
        n_c = sum(len(v) for v in judge_c)
        assert n_c >= eligible // 2, f"{scene}/{kind}: judge C applies to {n_c} of {eligible} near targets only"

        def label(i, path):
            return f"{scene}/{kind} S {S} inst {i} [{path}] " + "; ".join(t.label() for t in meta[i][:3])

        for path in PATHS:
            set_path(sc.bp, path)
            res = sc.bp.plan_batch(reqs)
            assert sc.bp.last_eval_form() == form, f"{scene}/{kind} [{path}]: {sc.bp.last_eval_form()}"
            assert_no_flat_launch(sc.bp, f"{scene}/{kind} [{path}]")
            for i, want in enumerate(wants):
                lab = label(i, path)
                with Replay(meta[i]):
                    check_tables(sc.bp, res, i, want, lab)
                    m = sc.bp.margins(i)[:, MG_COLLISION]
                    for t in judge_c[i]:
                        assert m[t.c] <= t.margin_bound, \
                            f"{lab}: target not listed by k_cull ({t.label()}): collision margin {m[t.c]:.3e}"
            if path not in ("group", "split-wave"):
                continue
            # D: time-major float64 tensors give the very same records; float32 tensors the oracle's on rounded inputs
            tsp = sc.bp.plan_packed(PackedBatch(reqs, np.float64, dyn_layout_tsp=True))
            assert bytes(tsp.records) == bytes(res.records), f"{scene}/{kind} [{path}]: time-major layout changes the records"
            f32 = sc.bp.plan_batch(reqs, obstacle_dtype=np.float32)
            assert sc.bp.last_eval_form() == form
            assert_no_flat_launch(sc.bp, f"{scene}/{kind} [{path}, float32 tensors]")
            for i, want32 in enumerate(wants32):
                lab = label(i, f"{path}, float32 tensors")
                with Replay(meta[i]):
                    _, status, keep, _ = sc.bp.candidates(i)
                    np.testing.assert_array_equal(status, want32.cand_status, err_msg=lab)
                    np.testing.assert_array_equal(keep, want32.cand_keep, err_msg=lab)
                    assert_record_matches_oracle(f32.records[i], want32, label=lab)
    finally:
        set_eval_path(sc.bp, "auto")
        sc.bp.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------

def test_a_wide_crowd_in_company():
    """One launch on one raised handle with two scenarios: a dense wide instance with statics and NaN tracks, a single
    track, a static-only instance, an obstacle-free one and a 33-sample distribution, interleaved.  The narrow records are
    byte-identical to their records alone on a DEFAULT handle, the wide one to its record alone."""
    wide = max((i for i in wc.crowd_instances() if i.n_static and i.n_nan), key=lambda i: i.S * i.P)
    ch = wide.handle
    d = np.asarray(wide.req.dist)
    assert np.isnan(d).any() and wide.S * wide.P * wide.T >= 1000
    other = 0.1 if wide.eps != 0.1 else 0.3           # the second scenario: the 33 samples get a budget of their own
    assert wc.max_viol(other, 33) >= 3
    narrow = [("dyn", wc.with_tensors(wide.req, None, None), wide.eps), ("static", wc.with_tensors(wide.req, wide.req.static, None), other),
              ("free", wc.with_tensors(wide.req, None, None), wide.eps), ("33 samples", wc.with_tensors(wide.req, wide.req.static, d[:33]), other)]
    narrow[0][1].dyn = np.ascontiguousarray(d[wide.S - 1])
    wants = {name: ch.oracle(rq, eps) for name, rq, eps in narrow}
    raised, default = Handle(ch, [wide], extra_eps=[other]), Handle(ch, [wide], sample_capacity=None, extra_eps=[other])
    try:
        assert default.bp.sample_capacity == _abi.MAX_SAMPLES and raised.eps == default.eps == [wide.eps, other]
        alone = {}
        for name, rq, eps in narrow:
            res = default.bp.plan_batch([default.req(rq, eps)])
            assert default.bp.last_eval_form() in ("lean", "general")
            check_tables(default.bp, res, 0, wants[name], f"{name} alone, default handle")
            alone[name] = rec_bytes(res.records[0])
        with pytest.raises(_abi.FotError):
            default.bp.plan_batch([default.reqs[0]])
        res = raised.plan([raised.reqs[0]], "lean-wide" if wide.lean_eligible else "general-wide", "wide alone")
        check_tables(raised.bp, res, 0, wide.want, "wide alone")
        alone["wide"] = rec_bytes(res.records[0])
        group = [(n, raised.req(rq, eps)) for n, rq, eps in narrow]
        group = group[:2] + [("wide", raised.reqs[0])] + group[2:]
        form = "general-wide"                        # the 33-sample instance has a budget: no lean launch
        for path in PATHS:
            set_path(raised.bp, path)
            res = raised.plan([rq for _, rq in group], form, f"company [{path}]")
            for slot, (name, _) in enumerate(group):
                check_tables(raised.bp, res, slot, wide.want if name == "wide" else wants[name], f"{name} in company [{path}]")
                assert rec_bytes(res.records[slot]) == alone[name], f"{name} [{path}]: differs from its record alone"
    finally:
        for h in (raised, default):
            h.restore()
            h.bp.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------

def test_the_external_path_checkers_against_crowds(crowd_handles):
    """paths_collision_free / check_paths on raised engines (k_check_ext_wide) on the candidates' own paths of an
    obstacle-free plan, against the part-1 tensors with statics, NaN tracks, one row and n_t // 2 rows, and
    check_paths_common.collision_free / categorise.  A decision within 1e-7 of a threshold is not judged; there are few."""
    insts = wc.checker_instances()
    engines = {}
    pairs = skipped = collide = 0
    try:
        for inst in insts:
            k = next(k for k, (h, _) in enumerate(wc.handles()) if h is inst.handle)
            hd = crowd_handles(k)
            hd.bp.plan_batch([hd.req(wc.with_tensors(inst.req, None, None), inst.eps)])
            cands = wc.checker_candidates(inst)
            fps = [hd.bp.candidate_path(c) for c in cands]
            key = (k, inst.eps)
            if key not in engines:                   # (the checkers read scenario 0 of their handle: an engine per eps)
                engines[key] = BatchPlanner(waypoints=inst.handle.waypoints, sample_capacity=CAPACITY, **inst.handle.planner_kw(inst.eps))
            eng = engines[key]
            static = None if inst.req.static is None else np.asarray(inst.req.static)
            dist = np.asarray(inst.req.dist)
            free = eng.paths_collision_free(fps, static, None, dist)
            cats = eng.check_paths(fps, static, None, inst.req.overrides, dist)
            judged = wc.judge_paths(inst, [{f: list(getattr(fp, f)) for f in cp.FIELDS} for fp in fps])
            for j, (c, (want_free, want_cat, margin)) in enumerate(zip(cands, judged)):
                pairs += 1
                if margin <= wc.CHECK_SKIP_MARGIN:
                    skipped += 1
                    continue
                assert bool(free[j]) == want_free and int(cats[j]) == want_cat, \
                    f"{inst.label()} path of cand {c}: free {bool(free[j])} / {want_free}, category {int(cats[j])} / {want_cat}"
                collide += not want_free
        assert pairs >= 50 and collide >= pairs // 4
        assert skipped <= wc.CHECK_SKIP_CAP * pairs, f"{skipped} of {pairs} pairs decide within {wc.CHECK_SKIP_MARGIN:g}"
    finally:
        for eng in engines.values():
            eng.close()
