"""Sampler loops whose slots name their Social-GAN model on the GPU (fot_sgan_load_model / fot_sgan_sample_model,
fot_loop_set_sampler_models, fot_debug_loop_sampler_shapes; SganSampler on several weights): the 'sgan' and 'lstm' conditions
of a campaign cell in one resident loop.  The comparator is never the models loop alone: the crowd-shared or slot-keyed loop
on a handle that holds only the slot's model, the stepwise loop, fot_sgan_sample on a one-model handle, or fot_sgan_noise fed
through fot_sgan_sample_model by hand.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import loop_crowd_common as cr
import loop_models_common as lm
import loop_sweep_common as sw
import recorded_samples_common as rs
import sgan_common as sc
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop, constants_of, loop_config_from
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import SganSampler, model_scenes
from pred_scores_common import METRIC_KEYS

pytestmark = pytest.mark.gpu

S, SEED = lm.S, lm.SEED
# (distribution_aware_planning, chance_epsilon, collision_margin_inflation): test_gpu_loop_sweep.py's K_CONDITIONS
K_CONDITIONS = ((False, 0.0, 1.0), (True, 0.0, 1.0), (True, 0.2, 1.0), (False, 0.0, 1.1))
N_ONE = 20                                        # lock steps of the one-crowd tests
N_TWO = 24                                        # ... of the two-crowd tests
NOISE_STEP = 3                                    # the lock step whose noise test 3 draws again: slots 2 and 4 still run

_cache = {}


def _shared(w, slot_crowd=None, **kw):
    """The parent's sampler: one model on the handle (fot_sgan_load), slot-keyed or crowd-shared."""
    return SganSampler(None, w, S, counter_seed=SEED, slot_crowd=slot_crowd, **kw)


def _models(ws, slot_crowd, slot_model):
    return SganSampler(None, list(ws), S, counter_seed=SEED, slot_crowd=slot_crowd, slot_model=slot_model)


def _shapes_while_running(sim, n, n_models):
    """Runs a resident loop one lock step per call: per step (running slots before it, fot_debug_loop_sampler_shapes)."""
    out = []
    for _ in range(n):
        sel = np.flatnonzero(sim.alive)
        if len(sel) == 0:
            break
        sim.run(1)
        out.append((sel, sim.engine.debug_loop_sampler_shapes(n_models)))
    return out


def _ran(view):
    """A slot's steps up to its last one (a loop goes on while any of its slots runs)."""
    while view and view[-1] is None:
        view = view[:-1]
    return view


def assert_slot_equals(sim, e, other, e_other, label):
    """Slot e of `sim` against slot e_other of `other`: step counts, termination and every step's bytes."""
    assert sim.step_counts[e] == other.step_counts[e_other] and sim.termination[e] == other.termination[e_other], f"{label}: slot {e}"
    got, want = _ran(rs.slot_view(sim, e)), _ran(rs.slot_view(other, e_other))
    assert len(got) == len(want) == sim.step_counts[e], f"{label}: slot {e}"
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{label}: slot {e} differs from its single-model loop at lock step {k}"


# ---- 1. one crowd, two models -------------------------------------------------------------------------------------------------------
def one_crowd(pred_len=sc.PRED_LEN):
    """(configurations, the crowd of the reference episode s6_eps02) under K_CONDITIONS."""
    ref, crowd, n_s, steps, _ = rs.reference_case("s6_eps02")
    assert n_s == S and crowd.shape[1] >= 10 and steps >= N_ONE
    cfgs = [dict(ref, pred_len=pred_len, distribution_aware_planning=a, chance_epsilon=e, collision_margin_inflation=m)
            for a, e, m in K_CONDITIONS]
    return cfgs, crowd


def test_one_crowd_two_models():
    """slot_model = [0, 0, 1, 1] over one crowd: slots 0, 1 are the two-slot crowd-shared loop on a handle whose only model is
    the pooled one, slots 2, 3 the one with the no-pooling model of other dimensions (noise width 4 against 8); the stepwise
    loop forms the same bytes; each model is handed 1 scene of P rows at every step."""
    cfgs, crowd = one_crowd()
    w = [lm.weights(lm.POOLED), lm.weights(lm.NO_POOLING)]
    assert w[0].desc.noise_dim == 8 and w[1].desc.noise_dim == 4 and w[1].desc.pooling_type == _abi.SGAN_POOL_NONE
    P, n, tracks = crowd.shape[1], N_ONE, [crowd] * 4
    with sw.loop(cfgs, tracks, None, _models(w, [0] * 4, [0, 0, 1, 1]), True) as res, \
            sw.loop(cfgs, tracks, None, _models(w, [0] * 4, [0, 0, 1, 1]), False) as stp:
        assert res._sweep and res._resident_sampler and stp._sweep and not stp._resident
        s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
        shapes = _shapes_while_running(res, n, 2)
        stp.run(n)
        assert len(shapes) == n and all(shape == [(1, P), (1, P)] for _, shape in shapes), shapes
        assert res.engine.debug_loop_sampler_shape() == (2, 2 * P)
        rs.assert_same_bytes(res, stp, s_res, s_stp, label="two models, resident against stepwise")
        for m in (0, 1):
            with sw.loop(cfgs[2 * m:2 * m + 2], tracks[:2], None, _shared(w[m], [0, 0]), True) as one:
                assert one._sweep and one._resident_sampler
                one.run(n)
                for e in (0, 1):
                    assert_slot_equals(res, 2 * m + e, one, e, f"model {m}")
        # (the conditions and the models matter on this crowd: the four egos have not all gone the same way)
        assert len({res.ego[e].tobytes() for e in range(4)}) > 1


# ---- 2. two crowds x two models, interleaved and ragged ---------------------------------------------------------------------------
SLOT_CROWD = [0, 1, 0, 1, 1, 0]
SLOT_MODEL = [0, 1, 1, 0, 0, 1]                   # units: (0, 0) = slot 0; (0, 1) = slots 2, 5; (1, 0) = slots 3, 4; (1, 1) = slot 1
# slot -> (path, distribution_aware_planning, chance_epsilon, collision_margin_inflation)
TWO_CONDITIONS = (("base", True, 0.2, 1.0), ("base", False, 0.0, 1.1), ("turn", True, 0.0, 1.1),
                  ("base", True, 0.2, 1.0), ("base", True, 0.0, 1.0), ("turn", False, 0.2, 1.0))
WALL_AHEAD = 9.0                                  # crowd 1's last three pedestrians charge at the ego from 9 m
SLOT1_AHEAD = 3.0                                 # ... and slot 1 starts 3 m closer to them: unit (1, 1) ends before unit (1, 0)


def two_crowds(pred_len=sc.PRED_LEN):
    """(configurations, the two crowds, tracks of the six slots, egos).  Slot 0 -- unit (0, 0) -- starts just short of the goal;
    crowd 1 runs into its wall, slot 1 -- unit (1, 1) -- first."""
    key = ("two", pred_len)
    if key not in _cache:
        cfgs = [sw.condition(*c, pred_len=pred_len) for c in TWO_CONDITIONS]
        c0, c1 = cr.crowds()
        pair = [c0, cr.walled(c1, WALL_AHEAD)]
        egos = [list(c["ego_initial_state"]) for c in cfgs]
        egos[0] = [rs.GOAL_START] + egos[0][1:]
        egos[1] = [egos[1][0] + SLOT1_AHEAD] + egos[1][1:]
        _cache[key] = (cfgs, pair, [pair[c] for c in SLOT_CROWD], egos)
    return _cache[key]


def assert_slots_equal_their_uniform_loops(sweep, w, pred_len, n, label, **kw):
    """Every slot e of the two-crowd sweep against slot SLOT_CROWD[e] of the fot_loop_begin loop of e's own configuration over
    [crowd 0, crowd 1] under the slot-keyed sampler on a handle that holds ONLY e's model: slot c draws crowd c's noise.
    Returns the uniform loops' (prediction_metrics, aggregate_metrics) rows where they score."""
    cfgs, pair, _, egos = two_crowds(pred_len)
    rows = []
    for e, cfg in enumerate(cfgs):
        c = SLOT_CROWD[e]
        ego_u = [list(cfg["ego_initial_state"]) for _ in pair]
        ego_u[c] = egos[e]
        with sw.loop(cfg, pair, ego_u, _shared(w[SLOT_MODEL[e]]), True, **kw) as one:
            assert not one._sweep and one.scenarios is None and one._resident_sampler
            one.run(n)
            assert_slot_equals(sweep, e, one, c, label)
            rows.append((one.prediction_metrics()[c], one.aggregate_metrics()[c]) if kw.get("prediction_scores") else None)
    return rows


def test_two_crowds_two_models_ragged_equal_their_uniform_loops():
    """Crowds of 3 and 17 pedestrians (17 crosses the generator's 16-row tile), six slots interleaved over crowds and models.
    Slot 0 reaches its goal at once (unit (0, 0) ends, crowd 0 runs on under model 1); crowd 1 ends in its wall, its unit
    under model 1 before its unit under model 0; then model 0 has no unit left and reports (0, 0) while model 1 goes on."""
    cfgs, pair, tracks, egos = two_crowds()
    w, n = [lm.weights(lm.POOLED), lm.weights(lm.NO_POOLING)], N_TWO
    counts = np.array([t.shape[1] for t in tracks])
    with sw.loop(cfgs, tracks, egos, _models(w, SLOT_CROWD, SLOT_MODEL), True) as res, \
            sw.loop(cfgs, tracks, egos, _models(w, SLOT_CROWD, SLOT_MODEL), False) as stp:
        assert res._sweep and res._resident_sampler and len(res.scenarios) >= 4
        s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
        shapes = _shapes_while_running(res, n, 2)
        stp.run(n)
        steps = res.step_counts
        # the premises: unit (0, 0) ended at once, unit (1, 1) ended before unit (1, 0), crowd 1 ended wholly while (0, 1) ran
        assert 0 < steps[0] < min(steps[2], steps[5]), steps
        assert 0 < steps[1] + 3 <= min(steps[3], steps[4]), steps      # (several steps: 7 against 11 when this was written)
        assert max(steps[[1, 3, 4]]) < n == steps[2] == steps[5], steps
        seen = set()
        for k, (sel, shape) in enumerate(shapes):
            units, _, _ = model_scenes(sel, counts[sel], [k] * len(sel), SLOT_CROWD, SLOT_MODEL)
            want = [(len(rep), int(counts[sel][rep].sum())) for _, rep, _ in units]
            assert shape == want, (k, sel, shape, want)
            seen.add(tuple(shape))
        # both models on both crowds; model 1 without crowd 1 while model 0 still samples it; model 0 with nothing left
        assert ((2, 20), (2, 20)) in seen and ((1, 17), (1, 3)) in seen and ((0, 0), (1, 3)) in seen, seen
        rs.assert_same_bytes(res, stp, s_res, s_stp, label="two crowds x two models, resident against stepwise")
        assert_slots_equal_their_uniform_loops(res, w, sc.PRED_LEN, n, "two crowds x two models")


# ---- 3. the noise: per pedestrian and Gaussian beside per scene and uniform -----------------------------------------------------
def test_fot_sgan_noise_through_sample_model_reproduces_a_step():
    """Model 0 mixes Gaussian noise per pedestrian, model 1 FOT_NOISE_UNIFORM_SYM noise per scene.  For a slot of either at a
    middle step: fot_sgan_noise(seed, the model's kind, row_slot = crowd id, the step, row_index) fed through
    fot_sgan_sample_model on the unit's window and resampled is the distribution block fot_debug_loop_block returns."""
    import torch
    cfgs, pair, tracks, egos = two_crowds()
    w = [lm.weights(lm.POOLED), lm.weights(lm.PER_SCENE, noise_type="uniform")]
    assert w[1].desc.noise_mix_type == _abi.SGAN_NOISE_GLOBAL and w[0].desc.noise_mix_type == _abi.SGAN_NOISE_PED
    k = NOISE_STEP
    with sw.loop(cfgs, tracks, egos, _models(w, SLOT_CROWD, SLOT_MODEL), True) as sim:
        assert sim.sample_source.model_kinds == [_abi.NOISE_GAUSSIAN, _abi.NOISE_UNIFORM_SYM]
        sim.run(k + 1)
        rec = sim._steps[k]
        what, window, sel, steps, o32, stale = rec["pred_src"][:6]
        counts = np.array([tracks[e].shape[1] for e in sel])
        units, _, _ = model_scenes(sel, counts, steps, SLOT_CROWD, SLOT_MODEL)
        assert what == "sgan" and sim.engine.debug_loop_sampler_shapes(2) == [(len(rep), int(counts[rep].sum())) for _, rep, _ in units]
        for slot in (4, 2):                                           # unit (1, 0), not its lowest slot; unit (0, 1)
            m, c, P = SLOT_MODEL[slot], SLOT_CROWD[slot], tracks[slot].shape[1]
            assert sim.alive[slot] and sim._slot_aware[slot]
            i = int(np.flatnonzero(sel == slot)[0])
            lo, hi = int(rec["off"][i]), int(rec["off"][i + 1])
            step = int(sim.step_counts[slot]) - 1                     # fot_loop_run_out.steps, before the step
            assert hi - lo == P and step == k == int(steps[i])
            blk, pre = sim.engine.debug_loop_block(i, samples=S, cap_points=S * 64 * 64)
            assert pre == -1 and blk.shape[:2] == (S, P)
            d = w[m].desc
            per_scene = d.noise_mix_type == _abi.SGAN_NOISE_GLOBAL
            n_rows = 1 if per_scene else P
            rows = dict(row_slot=np.full(n_rows, c), row_step=np.full(n_rows, step), row_index=np.arange(n_rows))
            noise = sim.engine.sgan_noise(SEED, sim.sample_source.model_kinds[m], S, d.noise_dim, **rows)
            assert noise.shape == (S, n_rows, d.noise_dim)
            raw = sim.sample_source.sample(window[:, lo:hi], np.array([0, P], np.int32), noise=noise, model=m)
            out = torch.zeros((S, P, blk.shape[2], 2), dtype=torch.float64, device=raw.device)
            torch.cuda.synchronize()
            T, _ = sim.resampler.resample_device(raw.data_ptr(), np.float32, S, P, o32[1][lo:hi].astype(np.float64), rec["pos"][lo:hi],
                                                 stale, out.data_ptr(), np.float64)
            torch.cuda.synchronize()
            assert T == blk.shape[2] and out.cpu().numpy().tobytes() == blk.tobytes(), slot
            # ... and not through the other model's kind
            other = sim.engine.sgan_noise(SEED, sim.sample_source.model_kinds[1 - m], S, d.noise_dim, **rows)
            assert other.tobytes() != noise.tobytes()


# ---- 4 / 5. a model that pools at every decoder step; scores -----------------------------------------------------------------------
STEP_MODEL = [0, 1, 0, 1]


def step_pool_case():
    """(configurations, tracks, weights): four conditions over the crowd of 17 pedestrians, pred_len 3; model 0 pools at every
    decoder step (its per-step state buffers are per model), model 1 does not pool."""
    cfgs = [sw.condition(*c, pred_len=3) for c in TWO_CONDITIONS[:4]]
    crowd17 = cr.crowds()[1]
    w = [lm.weights(lm.POOL_STEPS, pred_len=3), lm.weights(lm.NO_POOLING, pred_len=3)]
    assert w[0].desc.pool_every_timestep and w[0].desc.pooling_type == _abi.SGAN_POOL_NET
    return cfgs, [crowd17] * 4, w


def single_model_pairs(cfgs, tracks, w, n, **kw):
    """The two-slot crowd-shared loops of slots (0, 2) on model 0 alone and of slots (1, 3) on model 1 alone, run n steps."""
    for m in (0, 1):
        with sw.loop([cfgs[m], cfgs[m + 2]], tracks[:2], None, _shared(w[m], [0, 0]), True, **kw) as one:
            one.run(n)
            yield m, one


def test_a_model_that_pools_at_every_decoder_step():
    cfgs, tracks, w = step_pool_case()
    n = 14
    with sw.loop(cfgs, tracks, None, _models(w, [0] * 4, STEP_MODEL), True) as res:
        shapes = _shapes_while_running(res, n, 2)
        assert all(shape == [(1, 17), (1, 17)] for _, shape in shapes), shapes
        for m, one in single_model_pairs(cfgs, tracks, w, n):
            for e in (0, 1):
                assert_slot_equals(res, m + 2 * e, one, e, f"model {m}")
        assert len({res.ego[e].tobytes() for e in range(4)}) > 1


def test_scores_of_every_slot_equal_its_single_model_loop():
    """pred_len = 3: an origin's horizon is 12 lock steps, so the 24 steps complete some.  Every slot's prediction_metrics()
    and aggregate_metrics() row (fot_loop_score_summaries) equals its single-model loop's."""
    cfgs, tracks, w = step_pool_case()
    with sw.loop(cfgs, tracks, None, _models(w, [0] * 4, STEP_MODEL), True, prediction_scores=True) as sim:
        assert sim._sweep and sim._resident_scores
        sim.run(N_TWO)
        got, rows = sim.prediction_metrics(), sim.aggregate_metrics()
        counted, differ = 0, 0
        for m, one in single_model_pairs(cfgs, tracks, w, N_TWO, prediction_scores=True):
            want, want_rows = one.prediction_metrics(), one.aggregate_metrics()
            for e in (0, 1):
                assert_slot_equals(sim, m + 2 * e, one, e, f"scores, model {m}")
                counted += want[e]["ade_eval_count"]
                for k in METRIC_KEYS:
                    assert sw.same_metric(got[m + 2 * e][k], want[e][k]), (m, e, k, got[m + 2 * e][k], want[e][k])
                assert set(rows[m + 2 * e]) == set(want_rows[e])
                for k in want_rows[e]:
                    assert sw.same_metric(rows[m + 2 * e][k], want_rows[e][k]), (m, e, k)
        differ = sum(not sw.same_metric(got[0][k], got[1][k]) for k in METRIC_KEYS)
        assert counted > 0 and differ > 0                             # (the two models score differently on this crowd)


# ---- 6. degenerate forms -------------------------------------------------------------------------------------------------------------
def test_one_model_is_the_shared_loop():
    """slot_model all zero is fot_loop_set_sampler_shared -- with model 0 loaded through fot_sgan_load (the single SganWeights)
    or through fot_sgan_load_model(0) (a list of one), and also while a second model is loaded that no slot names."""
    cfgs, pair, tracks, egos = two_crowds()
    w0, w1, n = lm.weights(lm.POOLED), lm.weights(lm.NO_POOLING), N_TWO
    runs = {}
    for name, source in (("shared", _shared(w0, SLOT_CROWD)), ("list of one", _models([w0], SLOT_CROWD, [0] * 6)),
                         ("second model unnamed", _models([w0, w1], SLOT_CROWD, [0] * 6))):
        with sw.loop(cfgs, tracks, egos, source, True) as res:
            s_res = rs.spy_s_now(res)
            per_step = []
            for _ in range(n):
                res.run(1)
                per_step.append((res.engine.debug_loop_sampler_shape(), res.engine.debug_loop_sampler_shapes(2)))
            runs[name] = ([rs.slot_view(res, e) for e in range(6)], rs.run_bytes(res), per_step, [s.tobytes() for s in s_res])
    for name in ("list of one", "second model unnamed"):
        for part in (0, 1, 3):
            assert runs[name][part] == runs["shared"][part], (name, part)
        assert [a for a, _ in runs[name][2]] == [a for a, _ in runs["shared"][2]], name
    assert all(both == [one, (0, 0)] for one, both in runs["shared"][2] + runs["list of one"][2] + runs["second model unnamed"][2])
    assert set(one for one, _ in runs["shared"][2]) == {(2, 20), (1, 3)}    # both crowds, then crowd 0 alone


# ---- 7. stand-alone sampling -----------------------------------------------------------------------------------------------------------
def test_sample_model_equals_sample_on_a_handle_of_its_own():
    """fot_sgan_sample_model(m) is fot_sgan_sample on a handle that holds only that model, with the other model loaded
    before it, after it, and sampled in between.  Scenes [1, 3, 17], S = 3."""
    lib = _abi.lib()
    w = [lm.weights(lm.POOLED), lm.weights(lm.NO_POOLING), lm.weights(lm.POOL_STEPS)]
    off = np.array([0, 1, 4, 21], np.int32)
    rng = np.random.default_rng(11)
    obs = np.cumsum(rng.normal(0.0, 0.4, (sc.OBS_LEN, 21, 2)), axis=0).astype(np.float32)
    noise = [rng.normal(0.0, 1.0, (3, 21, v.desc.noise_dim)).astype(np.float32) for v in w]
    want = []
    for m, v in enumerate(w):
        with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
            want.append(SganSampler(bp, v, 3).sample(obs, off, noise=noise[m]).cpu().numpy().tobytes())
    assert len(set(want)) == 3
    crowd, model = [0, 0, 0], [0, 1, 2]
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        def load(m, v):
            _abi.check(bp._h, lib.fot_sgan_load_model(bp._h, m, C.byref(v.desc), v.blob.size, v.blob.ctypes.data))

        two = SganSampler(bp, w[:2], 3, counter_seed=SEED, slot_crowd=crowd[:2], slot_model=model[:2])      # loads 0, then 1
        got = lambda s, m: s.sample(obs, off, noise=noise[m], model=m).cpu().numpy().tobytes()
        assert got(two, 1) == want[1]                                 # the other model loaded before it
        assert got(two, 0) == want[0]
        assert got(two, 1) == want[1] and got(two, 0) == want[0]      # ... and sampled in between
        load(2, w[2])                                                 # ... and another loaded after
        three = SganSampler(None, w, 3, counter_seed=SEED, slot_crowd=crowd, slot_model=model)
        three.engine, three.device = bp, two.device                   # (the models are on the handle already)
        for m in (2, 1, 0, 2):
            assert got(three, m) == want[m], m
        load(1, w[2])                                                 # a model replaced: the others keep their numbers
        three.models[1], noise[1], want[1] = w[2], noise[2], want[2]
        for m in (0, 1, 2):
            assert got(three, m) == want[m], m
        assert lib.fot_sgan_unload_model(bp._h, 0) == _abi.OK
        assert got(three, 2) == want[2]
        assert lib.fot_sgan_sample_model(bp._h, 0, 0, off.ctypes.data, None, 3, None, 0, None, None) == _abi.ERR_INVALID
        assert b"fot_sgan_sample_model" in lib.fot_last_error(bp._h)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def _rebegin_cv(sim, cfg, ego0):
    """fot_loop_begin and fot_loop_set_replay on the loop's handle again: whatever predictor was set is dropped."""
    c = sim.config
    sim.engine.loop_begin(loop_config_from(c, constants_of(c), sim.MAX_REPLAN), ego0)
    sim.engine.loop_set_replay(sim.ped_off, sim.n_frames, sim._ped_all["trajectories"], sim._ped_all["velocities"],
                               obs_len=cfg["obs_len"], pred_len=sim.resampler.pred_len, rp=sim.resampler.params,
                               warmup_frames=int(cfg["obs_len"] * sim.sgan_dt / cfg["dt"]), ego_radius=sim.ego_radius,
                               ped_radius=sim.ped_radius, use_footprint=sim.footprint is not None,
                               s_end=float(np.ravel(sim.s_end)[0]), goal_distance=sim.GOAL_DISTANCE)


def test_refusals_change_nothing():
    lib = _abi.lib()
    w = [lm.weights(lm.POOLED), lm.weights(lm.NO_POOLING)]
    G, U = _abi.NOISE_GAUSSIAN, _abi.NOISE_UNIFORM_SYM
    c0, c1 = cr.crowds()
    aware = cr.base_config(distribution_aware_planning=True, pred_len=sc.PRED_LEN)
    cv_cfg = dict(aware, distribution_aware_planning=False, prediction_method="cv")
    n_run, tracks = 5, [c0, c1, c0, c1]

    def ids(*v):
        return np.array(v, np.int32)

    def refused(h, code, *args, call="fot_loop_set_sampler_models", names=()):
        assert getattr(lib, call)(h, *args) == code, (call, args)
        msg = lib.fot_last_error(h)
        assert call.encode() in msg and all(s.encode() in msg for s in names), msg

    def load(h, m, v, code=_abi.OK, call="fot_sgan_load_model"):
        args = (m,) if call == "fot_sgan_load_model" else ()
        assert getattr(lib, call)(h, *args, C.byref(v.desc), v.blob.size, v.blob.ctypes.data) == code

    crowd, model, kinds = ids(0, 1, 0, 1), ids(0, 0, 1, 1), ids(G, G)
    accepted = dict(S=S, seed=SEED, n_models=2, kinds=kinds, n_crowds=2, crowd=crowd, model=model)
    keep = []                                                         # (the arrays a call points into stay alive)

    def with_(**kw):
        """The arguments of the accepted call with some replaced (an array, or None for a NULL pointer)."""
        args = dict(accepted, **kw)
        keep.extend(v for v in args.values() if isinstance(v, np.ndarray))
        return tuple(v.ctypes.data if isinstance(v, np.ndarray) else v for v in args.values())

    ok = with_()

    with BatchedClosedLoop(cv_cfg, tracks, resident=True) as sim:
        sim.run(n_run)
        want_cv = rs.run_bytes(sim)
    with BatchedClosedLoop(aware, tracks, sample_source=_models(w, crowd, model), device_samples=True, resident=True) as twin:
        twin.run(n_run)
        want_models, want_shapes = rs.run_bytes(twin), twin.engine.debug_loop_sampler_shapes(2)
    assert want_shapes == [(2, 20), (2, 20)]

    # -- section 1: the models of a handle
    with BatchedClosedLoop(cv_cfg, tracks, resident=True) as sim:
        h, ego0 = sim.engine._h, sim.ego.copy()
        top = lib.fot_sgan_max_models()
        for m in (-1, top):
            load(h, m, w[0], _abi.ERR_INVALID)
            assert b"fot_sgan_load_model" in lib.fot_last_error(h)
            refused(h, _abi.ERR_INVALID, m, call="fot_sgan_unload_model")
            refused(h, _abi.ERR_INVALID, m, 0, None, None, S, None, 0, None, None, call="fot_sgan_sample_model")
        refused(h, _abi.ERR_INVALID, 1, call="fot_sgan_unload_model", names=("not loaded",))
        refused(h, _abi.ERR_INVALID, 1, 0, crowd.ctypes.data, None, S, None, 0, None, None, call="fot_sgan_sample_model")
        assert lib.fot_sgan_unload(h) == _abi.OK                      # (the old entry keeps its behaviour: nothing to drop)
        # -- section 2, before any model is loaded, and with model 1 missing
        refused(h, _abi.ERR_INVALID, *ok, names=("not loaded",))
        refused(h, _abi.ERR_INVALID, 2, None, None, call="fot_debug_loop_sampler_shapes")   # no sampler
        load(h, 0, w[0])
        refused(h, _abi.ERR_INVALID, *ok, names=("slot 2 names model 1", "not loaded"))
        load(h, 1, w[1])
        refused(h, _abi.ERR_INVALID, *with_(model=None), names=("NULL",))
        refused(h, _abi.ERR_INVALID, *with_(kinds=None), names=("NULL",))
        for bad in (0, top + 1):
            refused(h, _abi.ERR_INVALID, *with_(n_models=bad), names=("n_models",))
        for bad in (ids(0, 0, 1, 2), ids(0, -1, 1, 1)):
            refused(h, _abi.ERR_INVALID, *with_(model=bad), names=("slot_model[",))
        refused(h, _abi.ERR_INVALID, *with_(kinds=ids(G, _abi.NOISE_RAW)), names=("kind",))
        load(h, 1, lm.weights(lm.NO_POOLING, pred_len=3))
        refused(h, _abi.ERR_INVALID, *ok, names=("pred_len", "model 1"))
        load(h, 1, w[1])
        # ... everything the shared entry refuses
        refused(h, _abi.ERR_INVALID, *with_(crowd=None))
        refused(h, _abi.ERR_INVALID, *with_(n_crowds=0))
        refused(h, _abi.ERR_INVALID, *with_(crowd=ids(0, 1, 0, 2)))
        refused(h, _abi.ERR_INVALID, *with_(n_crowds=6, crowd=ids(5, 5, 5, 5)), names=("slots 0 and 1", "pedestrian counts"))
        refused(h, _abi.ERR_INVALID, *with_(S=0))
        refused(h, _abi.ERR_UNSUPPORTED, *with_(S=_abi.MAX_SAMPLES + 1))
        refused(h, _abi.ERR_INVALID, 2, None, None, call="fot_debug_loop_sampler_shapes")   # still no sampler
        sim.run(n_run)
        assert rs.run_bytes(sim) == want_cv                           # nothing changed: the constant-velocity loop
        refused(h, _abi.ERR_INVALID, *ok, names=("begun",))            # after the first step
        # summaries enabled / a plain scenario loop: FOT_ERR_UNSUPPORTED, as the shared entry
        _rebegin_cv(sim, cv_cfg, ego0)
        sim.engine.loop_summary_enable(True, 1)
        refused(h, _abi.ERR_UNSUPPORTED, *ok, names=("summaries",))
    # -- a refused call leaves an accepted one in force; loads and unloads are refused while it is; begin drops it
    with BatchedClosedLoop(aware, tracks, sample_source=_models(w, crowd, model), device_samples=True, resident=True) as sim:
        h, ego0 = sim.engine._h, sim.ego.copy()
        refused(h, _abi.ERR_INVALID, *with_(seed=SEED + 1, model=ids(0, 0, 1, 2)))
        refused(h, _abi.ERR_INVALID, *with_(seed=SEED + 1, n_models=0))
        for m in (0, 1, 2):                                           # any model, named by the loop or not
            load(h, m, w[1], _abi.ERR_INVALID)
            assert b"sampler" in lib.fot_last_error(h)
            refused(h, _abi.ERR_INVALID, m, call="fot_sgan_unload_model", names=("sampler",))
        load(h, 0, w[1], _abi.ERR_INVALID, call="fot_sgan_load")
        assert lib.fot_sgan_unload(h) == _abi.ERR_INVALID
        assert sim.engine.debug_loop_sampler_shapes(2) == [(0, 0), (0, 0)]                     # (no lock step yet)
        sim.run(n_run)
        assert rs.run_bytes(sim) == want_models and sim.engine.debug_loop_sampler_shapes(2) == want_shapes
        _rebegin_cv(sim, cv_cfg, ego0)
        refused(h, _abi.ERR_INVALID, 2, None, None, call="fot_debug_loop_sampler_shapes")       # the sampler went with the replay
        assert lib.fot_sgan_unload_model(h, 1) == _abi.OK                                      # ... and the models are free again
        load(h, 1, w[1])
        o = sim.engine.loop_run(n_run)
        with BatchedClosedLoop(cv_cfg, tracks, resident=True) as ref:
            want_o = ref.engine.loop_run(n_run)
        for key in ("ego", "jerk", "state", "stats", "followed", "keep", "cost", "after", "s_now", "steps", "termination"):
            assert np.ascontiguousarray(o[key]).tobytes() == np.ascontiguousarray(want_o[key]).tobytes(), key
    # -- a plain scenario loop plans against no distribution
    with BatchedClosedLoop([cv_cfg, dict(cv_cfg, collision_margin_inflation=1.1)] * 2, tracks, resident=True) as sim:
        assert sim.scenarios is not None and not sim._sweep
        for m in (0, 1):
            load(sim.engine._h, m, w[m])
        refused(sim.engine._h, _abi.ERR_UNSUPPORTED, *ok, names=("scenario loop",))
    # -- a slot of more than 256 pedestrians
    big = np.repeat(c1[:, :1], _abi.SGAN_MAX_PEDS + 1, axis=1) + np.arange(_abi.SGAN_MAX_PEDS + 1)[None, :, None] * 0.01
    with BatchedClosedLoop(cv_cfg, [big, c1], resident=True) as sim:
        for m in (0, 1):
            load(sim.engine._h, m, w[m])
        refused(sim.engine._h, _abi.ERR_UNSUPPORTED, *with_(crowd=ids(0, 1), model=ids(0, 1)), names=("FOT_SGAN_MAX_PEDS",))
    assert U != G
