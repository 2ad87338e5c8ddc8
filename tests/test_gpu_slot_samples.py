"""A sample count per slot of a sweep loop on the GPU (fot_loop_set_slot_samples, fot_debug_loop_slot_samples;
RecordedSamples / SganSampler(slot_samples=...)): slot e plans against, and is scored on, the first slot_samples[e]
samples of its source.  The comparator is never the sweep under test: the uniform loop of a slot's own condition on a
source cut to that slot's count, the stepwise sweep, or the sweep built without the keyword.  Every comparison is byte
equality.  The crowd is loop_sweep_common's ragged one with pedestrians moved so that the counts matter on it
(slot_samples_common; tests/test_slot_samples_cpu.py holds that premise on the oracle, the tests here assert it again on
the device), so none of them passes with the counts ignored."""
import numpy as np
import pytest

import loop_crowd_common as cr
import loop_sweep_common as sw
import recorded_samples_common as rs
import sgan_common as sc
import slot_samples_common as ss
import wide_loop_common as wl
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop, constants_of, loop_config_from
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import RecordedSamples, SganSampler, SganWeights, record_samples
from pred_scores_common import METRIC_KEYS

pytestmark = pytest.mark.gpu

S, STEPS, COUNTS = sw.SWEEP_S, sw.SWEEP_STEPS, ss.COUNTS
SEED = 20240921
_cache = {}


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(name=cr.PER_PED_MODEL):
    if name not in _cache:
        a = sc.case_args(name)
        _cache[name] = SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)))
    return _cache[name]


# ---- 1. premises (pass without the feature): the first k samples of S are the samples of k ---------------------------------------------
def test_premise_a_samplers_first_samples_do_not_depend_on_its_count():
    """fot_sgan_noise and fot_sgan_sample at S = 20 equal the first 20 samples at S = 50, bit for bit: the counter noise is
    keyed by the sample index and the generator's samples are independent of one another."""
    w = _weights()
    rng = np.random.default_rng(5)
    off = np.array([0, 3, 20], np.int32)
    obs = rng.normal(0.0, 2.0, (w.desc.obs_len, 20, 2)).astype(np.float32)
    slots, steps = np.array([4, 7]), np.array([3, 9])
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        few, many = SganSampler(bp, w, 20, counter_seed=SEED), SganSampler(bp, w, 50, counter_seed=SEED)
        row_slot, row_step, row_idx = np.repeat(slots, [3, 17]), np.repeat(steps, [3, 17]), np.r_[0:3, 0:17]
        n20 = bp.sgan_noise(SEED, _abi.NOISE_GAUSSIAN, 20, 8, row_slot, row_step, row_idx)
        n50 = bp.sgan_noise(SEED, _abi.NOISE_GAUSSIAN, 50, 8, row_slot, row_step, row_idx)
        assert n20.tobytes() == np.ascontiguousarray(n50[:20]).tobytes() and np.abs(n20).max() > 0
        a = few.sample(obs, off, slots=slots, steps=steps).cpu().numpy()
        b = many.sample(obs, off, slots=slots, steps=steps).cpu().numpy()
        assert a.shape[0] == 20 and b.shape[0] == 50 and a.tobytes() == np.ascontiguousarray(b[:20]).tobytes()
        assert len({b[s].tobytes() for s in range(50)}) == 50


# ---- the ragged crowd under five conditions and five counts ------------------------------------------------------------------------------
def ragged(pred_len=12, steps=STEPS):
    """(configurations, tracks, egos, float64 host recording [steps, 6, pred_len, 129, 2]) of the ragged sweep."""
    key = ("ragged", pred_len, steps)
    if key not in _cache:
        cfgs, tracks = sw.ragged_conditions(pred_len), ss.tracks()
        rec = rs.scripted_recording(cfgs[0], tracks, S, steps, dtype=np.float64).samples
        _cache[key] = (cfgs, tracks, sw.ragged_egos(cfgs), rec)
    return _cache[key]


def uniform_views(key, cfgs, tracks, egos, make_source, counts, steps, **kw):
    """For every slot e: (slot views, step counts, terminations, prediction metrics, summary rows, chosen samples) of the
    resident uniform loop of condition e on the source cut to counts[e] samples -- one loop per distinct (condition, count)."""
    key = ("uniform", key, tuple(counts), steps, tuple(sorted(kw)))
    if key not in _cache:
        views, sims = [], {}
        for e, cfg in enumerate(cfgs):
            cond = (tuple(sorted((k, str(v)) for k, v in cfg.items())), int(counts[e]))
            if cond not in sims:
                with sw.loop(cfg, tracks, egos, make_source(int(counts[e])), True, **kw) as sim:
                    assert sim.scenarios is None and not sim._sweep and sim._slot_samples is None
                    sim.run(steps)
                    scored = bool(kw.get("prediction_scores"))
                    sims[cond] = ([rs.slot_view(sim, i) for i in range(len(cfgs))], sim.step_counts.copy(), sim.termination.copy(),
                                  sim.prediction_metrics() if scored else None, sim.aggregate_metrics() if scored else None,
                                  np.stack([np.asarray(s.best) if s.best is not None else np.full(len(cfgs), -2) for s in sim._steps])
                                  if sim._plan_rep else None)
            views.append(sims[cond])
        _cache[key] = views
    return _cache[key]


def assert_slots_equal_their_uniform_loops(sweep, uniform, label, modes=None):
    for e in range(len(uniform)):
        views, counts, term = uniform[e][:3]
        assert sweep.step_counts[e] == counts[e] and sweep.termination[e] == term[e], f"{label}: slot {e}"
        got, want = rs.slot_view(sweep, e), views[e]
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a == b, f"{label}: slot {e} differs from its uniform loop at lock step {k}"
        if modes is not None and modes[e] == sw.REP and sweep._resident:      # the chosen samples, in [0, count)
            best = np.stack([np.asarray(s.best) if s.best is not None else np.full(len(uniform), -2) for s in sweep._steps])[:, e]
            assert np.array_equal(best, uniform[e][5][:, e]), f"{label}: slot {e} best samples"
            assert best.max() < sweep._slot_samples[e]


def differs(view_a, view_b):
    return any(a != b for a, b in zip(view_a, view_b))


# ---- 2. a recording ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_slot_equals_the_uniform_loop_of_its_count_on_a_recording(dtype, where):
    """Counts (6, 1, 4, 6, 3) over one 6-sample recording of the ragged crowd: slot e of the sweep equals slot e of the
    uniform loop of its condition on RecordedSamples(rec[:, :S_e]) -- records, step counts, termination, best samples --
    and the resident sweep equals the stepwise one.  The counts matter: slot 1 (count 1) is not slot 1 of the sweep
    without counts."""
    cfgs, tracks, egos, rec = ragged()
    host = rec.astype(dtype)
    samples = _cuda(host) if where == "device" else host
    uniform = uniform_views(np.dtype(dtype).name, cfgs, tracks, egos, lambda k: RecordedSamples(ss.prefix(host, k)), COUNTS, STEPS)
    source = lambda **kw: RecordedSamples(samples, **kw)
    with sw.loop(cfgs, tracks, egos, source(slot_samples=COUNTS), True) as res, \
            sw.loop(cfgs, tracks, egos, source(slot_samples=COUNTS), False) as stp, sw.loop(cfgs, tracks, egos, source(), True) as plain:
        assert res._sweep and res._resident_recording and stp._sweep and stp._native and not stp._resident
        s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
        res.run(STEPS)
        stp.run(STEPS)
        plain.run(STEPS)
        ended = res.step_counts[[0, 2, 4]]
        assert (ended < STEPS).all() and (ended > 0).all() and res.alive[[1, 3]].all(), res.step_counts
        rs.assert_same_bytes(res, stp, s_res, s_stp, label=f"counts {np.dtype(dtype)} {where}")
        assert_slots_equal_their_uniform_loops(res, uniform, f"{np.dtype(dtype)} {where}", sw.modes_of(cfgs))
        assert differs(rs.slot_view(res, 1), rs.slot_view(plain, 1)), "the count of slot 1 changed nothing"
        for e in (0, 3):                                              # (count 6 = the source's: the slot of the plain sweep)
            assert not differs(rs.slot_view(res, e), rs.slot_view(plain, e))


@pytest.mark.parametrize("resident", [False, True], ids=["stepwise", "resident"])
def test_all_counts_equal_to_the_sources_is_the_sweep_without_the_keyword(resident):
    cfgs, tracks, egos, rec = ragged()
    with sw.loop(cfgs, tracks, egos, RecordedSamples(rec, slot_samples=[S] * 5), resident) as a, \
            sw.loop(cfgs, tracks, egos, RecordedSamples(rec), resident) as b:
        assert a._sweep and b._sweep and a._slot_samples is not None and b._slot_samples is None
        s_a, s_b = rs.spy_s_now(a), rs.spy_s_now(b)
        a.run(STEPS)
        b.run(STEPS)
        rs.assert_same_bytes(a, b, s_a, s_b, label="all counts 6")
        assert list(a.engine.debug_loop_slot_samples()) == [S] * len(a._steps[-1]["sel"])


@pytest.mark.parametrize("resident", [False, True], ids=["stepwise", "resident"])
def test_two_counts_over_one_crowd_and_one_configuration(resident):
    """ONE configuration with slot_samples builds the sweep loop of it.  chance_epsilon = 0.2 over one crowd (slot_col0 =
    [0, 0]): 6 samples allow floor(1.2) = 1 violating sample, 4 allow none -- the two slots select different candidates,
    and each is the uniform loop of its count."""
    cfg, crowd = sw.condition(*ss.EPS_CONDITION), ss.eps_crowd()
    rec = rs.scripted_recording(cfg, [crowd], S, STEPS, dtype=np.float64).samples
    tracks = [crowd, crowd]
    with sw.loop(cfg, tracks, None, RecordedSamples(_cuda(rec), slot_col0=[0, 0], slot_samples=[6, 4]), resident) as sim:
        assert sim._sweep and len(sim.scenarios) == 1 and list(sim.slot_scenario) == [0, 0] and sim.engine._loop_sweep
        sim.run(STEPS)
        views = [rs.slot_view(sim, e) for e in range(2)]
        assert differs(views[0], views[1]), "6 and 4 samples under chance_epsilon = 0.2 selected the same candidates"
        assert list(sim.engine.debug_loop_slot_samples()) == [6, 4]
        for e, k in enumerate((6, 4)):
            with sw.loop(cfg, [crowd], None, RecordedSamples(ss.prefix(rec, k)), True) as uni:
                assert not uni._sweep
                uni.run(STEPS)
                assert views[e] == rs.slot_view(uni, 0), f"slot {e} (count {k})"


# ---- 3. across the kernel boundary -------------------------------------------------------------------------------------------------------
WIDE_COUNTS = (130, 64, 65, 1, 20)


def _wide(counts, steps=STEPS, pred_len=3):
    cap = max(max(counts), 64)
    cfgs, tracks, egos, _ = ragged(pred_len, steps)
    key = ("wide rec", max(counts), pred_len, steps)
    if key not in _cache:
        _cache[key] = record_samples(cfgs[0], tracks, wl.wide_sample_source(max(counts), pred_len), steps, dtype=np.float64,
                                     sample_capacity=cap).samples
    return cfgs, tracks, egos, _cache[key], cap


def _wide_forms(sim):
    return int(_abi.lib().fot_debug_set_eval_form(sim.engine._h, -1)) & 12      # 4 | 8: a launch of the last plan call was wide


def test_counts_either_side_of_64_with_scores():
    """A handle raised to 130, a 130-sample recording, counts (130, 64, 65, 1, 20), representative-mode slots among them,
    prediction_scores=True (pred_len = 3: horizons complete within the run).  Every slot equals the uniform loop of its
    condition and count -- records, prediction_metrics() and aggregate_metrics() key for key --, and a lock step whose
    running counts are all <= 64 took narrow launches."""
    cfgs, tracks, egos, rec, cap = _wide(WIDE_COUNTS)
    kw = dict(prediction_scores=True, sample_capacity=cap)
    uniform = uniform_views("wide scores", cfgs, tracks, egos, lambda k: RecordedSamples(ss.prefix(rec, k), sample_capacity=cap),
                            WIDE_COUNTS, STEPS, **kw)
    with sw.loop(cfgs, tracks, egos, RecordedSamples(_cuda(rec), sample_capacity=cap, slot_samples=WIDE_COUNTS), True, **kw) as sim:
        assert sim._sweep and sim._resident_scores
        seen = set()
        for _ in range(STEPS):
            sel = np.flatnonzero(sim.alive)
            sim.run(1)
            counts = list(sim.engine.debug_loop_slot_samples())
            assert counts == [WIDE_COUNTS[e] for e in sel]
            forms = _wide_forms(sim)                                  # (of the step's last plan call: level 0, or its escalations)
            if all(c <= 64 for c in counts):
                assert forms == 0, (counts, forms)
                seen.add(False)
            elif forms:
                seen.add(True)
        assert seen == {True, False}
        assert_slots_equal_their_uniform_loops(sim, uniform, "wide counts", sw.modes_of(cfgs))
        got, rows = sim.prediction_metrics(), sim.aggregate_metrics()
        counted = 0
        for e in range(len(cfgs)):
            want, want_row = uniform[e][3][e], uniform[e][4][e]
            counted += want["ade_eval_count"]
            for k in METRIC_KEYS:
                assert sw.same_metric(got[e][k], want[k]), (e, k, got[e][k], want[k])
            assert set(rows[e]) == set(want_row)
            for k in want_row:
                assert sw.same_metric(rows[e][k], want_row[k]), (e, k, rows[e][k], want_row[k])
            if want["ade_eval_count"]:
                assert got[e]["pred_samples"] == WIDE_COUNTS[e]
        assert counted > 0


def test_a_count_of_254():
    counts = (254, 20, 254, 1, 64)
    cfgs, tracks, egos, rec, cap = _wide(counts, steps=8)
    uniform = uniform_views("254", cfgs, tracks, egos, lambda k: RecordedSamples(ss.prefix(rec, k), sample_capacity=cap), counts, 8,
                            sample_capacity=cap)
    with sw.loop(cfgs, tracks, egos, RecordedSamples(_cuda(rec), sample_capacity=cap, slot_samples=counts), True, sample_capacity=cap) as sim:
        sim.run(8)
        assert_slots_equal_their_uniform_loops(sim, uniform, "254", sw.modes_of(cfgs))


# ---- 4. the library's sampler ------------------------------------------------------------------------------------------------------------
SLOT_CROWD = [0, 1, 0, 1, 1, 0]
SAMPLER_COUNTS = [5, 5, 20, 20, 65, 65]
N_SAMPLER = 10


@pytest.mark.parametrize("form", ["shared", "models"])
def test_sampler_slots_equal_the_uniform_counter_seeded_loops(form):
    """Two crowds x three counts (5, 20, 65) on a handle raised to 65, one sampling per crowd and lock step
    (fot_debug_loop_sampler_shape); with slot_model, two models.  Every slot equals the uniform counter-seeded loop of
    its count, and the resident sweep the stepwise one, whose host-side sampler hands over all 65 samples."""
    cfg = sw.condition("base", True, 0.2, 1.0, pred_len=sc.PRED_LEN)
    pair = cr.crowds()
    tracks = [pair[c] for c in SLOT_CROWD]
    w = [_weights(cr.PER_PED_MODEL), _weights(cr.PER_SCENE_MODEL)]
    model = [0, 1, 1, 0, 0, 1]

    def source(k, **kw):
        if form == "models":
            return SganSampler(None, w, k, counter_seed=SEED, slot_crowd=SLOT_CROWD, slot_model=model, sample_capacity=65, **kw)
        return SganSampler(None, w[0], k, counter_seed=SEED, slot_crowd=SLOT_CROWD, sample_capacity=65, **kw)
    uniform = {}
    for k in sorted(set(SAMPLER_COUNTS)):
        with sw.loop(cfg, tracks, None, source(k), True, sample_capacity=65) as uni:
            assert not uni._sweep
            uni.run(N_SAMPLER)
            uniform[k] = [rs.slot_view(uni, e) for e in range(6)]
    with sw.loop(cfg, tracks, None, source(65, slot_samples=SAMPLER_COUNTS), True, sample_capacity=65) as res, \
            sw.loop(cfg, tracks, None, source(65, slot_samples=SAMPLER_COUNTS), False, sample_capacity=65) as stp:
        assert res._sweep and res._resident_sampler and stp._sweep and not stp._resident
        s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
        rows = sum(p.shape[1] for p in pair)
        for _ in range(N_SAMPLER):
            if not res.alive.all():
                break
            res.run(1)
            if form == "shared":
                assert res.engine.debug_loop_sampler_shape() == (2, rows)
            else:                                                     # (each (crowd, model) unit once: both crowds under both models)
                assert res.engine.debug_loop_sampler_shapes(2) == [(2, rows), (2, rows)]
            assert list(res.engine.debug_loop_slot_samples()) == SAMPLER_COUNTS
        assert len(res._steps) >= 4
        res.run(N_SAMPLER - len(res._steps))
        stp.run(N_SAMPLER)
        rs.assert_same_bytes(res, stp, s_res, s_stp, label=f"sampler counts, {form}")
        for e, k in enumerate(SAMPLER_COUNTS):
            assert rs.slot_view(res, e) == uniform[k][e], f"{form}: slot {e} (count {k})"
        assert any(differs(uniform[5][e], uniform[65][e]) for e in range(6)), "5 and 65 samples planned alike on both crowds"


# ---- 5. slots ending early ---------------------------------------------------------------------------------------------------------------
def test_blocks_and_counts_while_slots_end():
    """The first, a middle and the last slot end early, so the frame's blocks shrink and move.  At lock steps in the middle
    of the run fot_debug_loop_slot_samples names the running slots' counts and fot_debug_loop_block answers with the
    episode's own count of samples: the block of the uniform loop of that count."""
    cfgs, tracks, egos, rec = ragged()
    modes = sw.modes_of(cfgs)
    marks = (2, 8, 14)
    with sw.loop(cfgs, tracks, egos, RecordedSamples(_cuda(rec), slot_samples=COUNTS), True) as res, \
            sw.loop(cfgs, tracks, egos, RecordedSamples(rec, slot_samples=COUNTS), False) as stp:
        uni = {e: sw.loop(cfgs[e], tracks, egos, RecordedSamples(ss.prefix(rec, COUNTS[e])), True) for e in range(5)}
        try:
            done, running = 0, []
            for mark in marks:
                for sim in (res, stp, *uni.values()):
                    sim.run(mark - done)
                done = mark
                sel = [int(e) for e in res._steps[-1]["sel"]]
                running.append(tuple(sel))
                assert [int(e) for e in stp._steps[-1]["sel"]] == sel
                for sim in (res, stp):
                    assert list(sim.engine.debug_loop_slot_samples()) == [COUNTS[e] for e in sel]
                for i, e in enumerate(sel):
                    n = COUNTS[e] if modes[e] == sw.DIST else 1
                    blk, pre = res.engine.debug_loop_block(i, samples=n, cap_points=S * 65 * 64)
                    blk_s, pre_s = stp.engine.debug_loop_block(i, samples=n, cap_points=S * 65 * 64)
                    assert blk.shape[0] == n and blk.tobytes() == blk_s.tobytes() and pre == pre_s, (mark, e)
                    j = [int(v) for v in uni[e]._steps[-1]["sel"]].index(e)
                    blk_u, pre_u = uni[e].engine.debug_loop_block(j, samples=n, cap_points=S * 65 * 64)
                    assert blk.tobytes() == blk_u.tobytes() and pre == pre_u, (mark, e)
                    # a cap of one point less than the episode's own block is refused: the count is what the answer is sized by
                    if blk.size:
                        with pytest.raises(_abi.FotError):
                            res.engine.debug_loop_block(i, samples=n, cap_points=blk.size // 2 - 1)
            assert len(set(running)) == len(marks) and len(running[-1]) < len(running[0]) == 5
        finally:
            for sim in uni.values():
                sim.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _abi.lib()
    cfgs, tracks, egos, rec = ragged()
    n_run = STEPS                                                     # (the count of slot 1 shows late in the run)
    counts = np.array(COUNTS, np.int32)

    def run_bytes(sim):
        sim.run(n_run)
        return rs.run_bytes(sim)

    def refused(h, code, n, arr, text=b"fot_loop_set_slot_samples"):
        assert lib.fot_loop_set_slot_samples(h, n, None if arr is None else arr.ctypes.data) == code, (n, arr)
        assert text in lib.fot_last_error(h)
    with sw.loop(cfgs, tracks, egos, RecordedSamples(rec), True) as sim:
        want_plain = run_bytes(sim)
    with sw.loop(cfgs, tracks, egos, RecordedSamples(rec, slot_samples=COUNTS), True) as sim:
        want_counts = run_bytes(sim)
    assert want_plain != want_counts
    assert lib.fot_loop_set_slot_samples(None, 5, counts.ctypes.data) == _abi.ERR_INVALID
    # a sweep loop with its recording set: every refusal, then the plain sweep's bytes; the counts once, then after a step
    with sw.loop(cfgs, tracks, egos, RecordedSamples(rec), True) as sim:
        h = sim.engine._h
        refused(h, _abi.ERR_INVALID, 5, None)
        refused(h, _abi.ERR_INVALID, 4, counts)
        refused(h, _abi.ERR_INVALID, 6, np.array(COUNTS + (1,), np.int32))
        for bad in ((6, 0, 4, 6, 3), (6, 1, 4, 7, 3), (-1, 1, 4, 6, 3)):
            refused(h, _abi.ERR_INVALID, 5, np.array(bad, np.int32))
        assert run_bytes(sim) == want_plain
        refused(h, _abi.ERR_INVALID, 5, counts)                      # after the first step
    with sw.loop(cfgs, tracks, egos, RecordedSamples(rec, slot_samples=COUNTS), True) as sim:
        h = sim.engine._h
        refused(h, _abi.ERR_INVALID, 5, np.array((6, 1, 4, 7, 3), np.int32))
        refused(h, _abi.ERR_INVALID, 4, counts)
        assert run_bytes(sim) == want_counts                          # (a refused call leaves the accepted counts in force)
    # no source: a sweep loop with a replay and neither sampler nor recording
    cv = [dict(c, distribution_aware_planning=False, prediction_method="cv") for c in cfgs]
    with BatchedClosedLoop(cv, tracks, egos, resident=True) as sim:
        h = sim.engine._h
        want_cv = None
        refused(h, _abi.ERR_UNSUPPORTED, 5, counts)                   # a fot_loop_begin_scenarios loop is no sweep loop
        sim.engine.loop_begin_sweep([loop_config_from(k, constants_of(k), sim.MAX_REPLAN) for k in sim.scenarios], [False] * 4,
                                    np.array([0, 1, 2, 3, 0], np.int32), sw.modes_of(cfgs), sim.ego)
        sim.engine.loop_set_replay(sim.ped_off, sim.n_frames, sim._ped_all["trajectories"], sim._ped_all["velocities"],
                                   obs_len=cv[0]["obs_len"], pred_len=sim.resampler.pred_len, rp=sim.resampler.params,
                                   warmup_frames=int(cv[0]["obs_len"] * sim.sgan_dt / cv[0]["dt"]), ego_radius=sim.ego_radius,
                                   ped_radius=sim.ped_radius, use_footprint=False, s_end=float(np.ravel(sim.s_end)[0]),
                                   goal_distance=sim.GOAL_DISTANCE)
        refused(h, _abi.ERR_INVALID, 5, counts)                       # no source set
        sim.run(n_run)
        want_cv = rs.run_bytes(sim)
    with BatchedClosedLoop(cv, tracks, egos, resident=True) as sim:
        assert run_bytes(sim) == want_cv
    # loops that are no sweep loops: one configuration, resident and stepwise
    one = dict(cfgs[0])
    for resident in (True, False):
        with sw.loop(one, tracks, egos, RecordedSamples(rec), resident) as a, sw.loop(one, tracks, egos, RecordedSamples(rec), resident) as b:
            refused(a.engine._h, _abi.ERR_UNSUPPORTED, 5, counts)
            assert run_bytes(a) == run_bytes(b)
    # dropped with the source: a new set call, fot_loop_set_replay, fot_loop_begin_sweep
    with sw.loop(cfgs, tracks, egos, RecordedSamples(rec, slot_samples=COUNTS), True) as sim:
        sim.engine.loop_set_samples(rec.astype(np.float64), 0)
        assert run_bytes(sim) == want_plain
    # a stepwise sweep: a frame whose dist_S lies below a running slot's count is refused
    with sw.loop(cfgs, tracks, egos, RecordedSamples(rec, slot_samples=COUNTS), False) as a:
        a.run(3)
        short = RecordedSamples(ss.prefix(rec, 5))
        short.attach(a.ped_off, cfgs[0]["pred_len"], True)
        a.sample_source = short
        with pytest.raises(_abi.FotError, match="dist_S = 5 is below the sample count of slot"):
            a.step()
