"""Sampler loops whose slots share crowds on the GPU (fot_loop_set_sampler_shared, fot_debug_loop_sampler_shape;
SganSampler(slot_crowd=...)): the conditions of a sweep over one crowd plan against ONE sampling per lock step.  The
comparator is never the crowd loop alone: the same sweep on a recording of the parent's slot-keyed sampler, the uniform
loops of the slots' own conditions under that sampler, the stepwise loop, or fot_sgan_noise fed through the sampler by
hand.  Every comparison is byte equality."""
import numpy as np
import pytest

import loop_crowd_common as cr
import loop_sweep_common as sw
import noise_common as nc
import recorded_samples_common as rs
import sgan_common as sc
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop, constants_of, loop_config_from
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import RecordedSamples, SganSampler, SganWeights, record_samples
from pred_scores_common import METRIC_KEYS

pytestmark = pytest.mark.gpu

S, SEED = cr.S, cr.SEED
# (distribution_aware_planning, chance_epsilon, collision_margin_inflation): test_gpu_loop_sweep.py's K_CONDITIONS
K_CONDITIONS = ((False, 0.0, 1.0), (True, 0.0, 1.0), (True, 0.2, 1.0), (False, 0.0, 1.1))
N_ONE = 20                                        # lock steps of the one-crowd tests
N_TWO = 24                                        # ... of the two-crowd tests
NOISE_STEP = 3                                    # the lock step whose noise test 6 draws again: slots 3 and 4 of crowd 1 still run

_cache = {}


def _weights(name=cr.PER_PED_MODEL, **over):
    key = (name, tuple(sorted(over.items())))
    if key not in _cache:
        a = dict(sc.case_args(name), **over)
        _cache[key] = SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)))
    return _cache[key]


def _source(w, slot_crowd=None, **kw):
    return SganSampler(None, w, S, counter_seed=SEED, slot_crowd=slot_crowd, **kw)


def _shapes_while_running(sim, n):
    """Runs a resident loop one lock step per call: per step (running slots before it, fot_debug_loop_sampler_shape)."""
    out = []
    for _ in range(n):
        sel = np.flatnonzero(sim.alive)
        if len(sel) == 0:
            break
        sim.run(1)
        out.append((sel, sim.engine.debug_loop_sampler_shape()))
    return out


def _blocks(sim):
    """fot_debug_loop_block of every episode of the most recent frame, in its own mode."""
    out = []
    for i, slot in enumerate(int(e) for e in sim._steps[-1]["sel"]):
        n = S if sim._slot_aware[slot] else 1
        out.append((slot,) + sim.engine.debug_loop_block(i, samples=n, cap_points=S * 64 * 64))
    return out


# ---- 1 / 4. one crowd, K = 4 conditions -------------------------------------------------------------------------------------------
def one_crowd(pred_len=sc.PRED_LEN):
    """(configurations, the crowd of the reference episode s6_eps02) under K_CONDITIONS."""
    ref, crowd, n_s, steps, _ = rs.reference_case("s6_eps02")
    assert n_s == S and crowd.shape[1] >= 10 and steps >= N_ONE
    cfgs = [dict(ref, pred_len=pred_len, distribution_aware_planning=a, chance_epsilon=e, collision_margin_inflation=m)
            for a, e, m in K_CONDITIONS]
    return cfgs, crowd


def _recording_of(cfg, tracks, w, n, **kw):
    """The parent's slot-keyed sampler recorded over `tracks`: slot c of a loop without crowds (prediction.record_samples)."""
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        return record_samples(cfg, tracks, SganSampler(bp, w, S, counter_seed=SEED, **kw), n, device="cuda").samples.clone()


@pytest.mark.parametrize("model", [cr.PER_PED_MODEL, cr.PER_SCENE_MODEL], ids=["noise_per_pedestrian", "noise_per_scene"])
def test_conditions_over_one_crowd_share_one_sampling(model):
    """slot_crowd = [0, 0, 0, 0]: the resident sweep equals the same sweep on a recording of the slot-keyed sampler run over
    the crowd alone (RecordedSamples(slot_col0 = [0, 0, 0, 0])), and the stepwise sweep with the shared sampler; the
    generator is handed 1 scene of P rows while any slot runs."""
    cfgs, crowd = one_crowd()
    w, P, n = _weights(model), crowd.shape[1], N_ONE
    tracks = [crowd] * 4
    rec = _recording_of(cfgs[0], [crowd], w, n)
    assert tuple(rec.shape) == (n, S, sc.PRED_LEN, P, 2)
    with sw.loop(cfgs, tracks, None, _source(w, [0, 0, 0, 0]), True) as res, \
            sw.loop(cfgs, tracks, None, RecordedSamples(rec, slot_col0=[0, 0, 0, 0]), True) as want, \
            sw.loop(cfgs, tracks, None, _source(w, [0, 0, 0, 0]), False) as stp:
        assert res._sweep and res._resident_sampler and want._resident_recording and stp._sweep and not stp._resident
        s_res, s_want, s_stp = rs.spy_s_now(res), rs.spy_s_now(want), rs.spy_s_now(stp)
        shapes = _shapes_while_running(res, n)
        want.run(n)
        stp.run(n)
        assert len(shapes) == n and all(shape == (1, P) for _, shape in shapes), shapes
        rs.assert_same_bytes(res, want, s_res, s_want, label="shared sampler against the shared recording")
        rs.assert_same_bytes(res, stp, s_res, s_stp, label="shared sampler, resident against stepwise")
        # (the conditions matter on this crowd: the four egos over the same pedestrians have not all gone the same way)
        assert len({res.ego[e].tobytes() for e in range(4)}) > 1
        for (slot, blk, pre), (_, blk_w, pre_w), (_, blk_s, pre_s) in zip(_blocks(res), _blocks(want), _blocks(stp)):
            assert blk.size > 0 and blk.tobytes() == blk_w.tobytes() == blk_s.tobytes() and pre == pre_w == pre_s, slot


# ---- 2. two crowds x three conditions, interleaved and ragged ----------------------------------------------------------------------
SLOT_CROWD = [0, 1, 0, 1, 1, 0]
# slot -> (path, distribution_aware_planning, chance_epsilon, collision_margin_inflation)
TWO_CONDITIONS = (("base", True, 0.2, 1.0), ("base", False, 0.0, 1.1), ("turn", True, 0.0, 1.1),
                  ("base", True, 0.2, 1.0), ("base", True, 0.0, 1.0), ("turn", False, 0.2, 1.0))
WALL_AHEAD = 9.0                                  # crowd 1's last three pedestrians charge at the ego from 9 m
SLOT1_AHEAD = 3.0                                 # ... and slot 1 starts 3 m closer to them: crowd 1's lowest slot ends first


def two_crowds(pred_len=sc.PRED_LEN):
    """(configurations, the two crowds, tracks of the six slots, egos).  Slot 0 -- the lowest of crowd 0 -- starts just short
    of the goal; crowd 1 runs into its wall, slot 1 first."""
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


def uniform_views(w, pred_len=sc.PRED_LEN, n=N_TWO, **kw):
    """For every slot e of the two-crowd sweep: (slot_view, step count, termination, metrics, summary row) of slot
    SLOT_CROWD[e] of the fot_loop_begin loop of e's own configuration and mode over [crowd 0, crowd 1] under the slot-keyed
    sampler -- the parent's loop, in which slot c draws crowd c's noise."""
    key = ("uniform", id(w), pred_len, n, tuple(sorted(kw)))
    if key not in _cache:
        cfgs, pair, _, egos = two_crowds(pred_len)
        out = []
        for e, cfg in enumerate(cfgs):
            c = SLOT_CROWD[e]
            ego_u = [list(cfg["ego_initial_state"]) for _ in pair]
            ego_u[c] = egos[e]
            with sw.loop(cfg, pair, ego_u, _source(w), True, **kw) as sim:
                assert not sim._sweep and sim.scenarios is None and sim._resident_sampler
                sim.run(n)
                scored = kw.get("prediction_scores")
                out.append((rs.slot_view(sim, c), int(sim.step_counts[c]), int(sim.termination[c]),
                            sim.prediction_metrics()[c] if scored else None, sim.aggregate_metrics()[c] if scored else None))
        _cache[key] = out
    return _cache[key]


def _ran(view):
    """A slot's steps up to its last one (a loop goes on while any of its slots runs)."""
    while view and view[-1] is None:
        view = view[:-1]
    return view


def assert_slots_equal_their_uniform_loops(sweep, uniform, label):
    for e in range(len(SLOT_CROWD)):
        view, count, term = uniform[e][:3]
        assert sweep.step_counts[e] == count and sweep.termination[e] == term, f"{label}: slot {e}"
        got, want = _ran(rs.slot_view(sweep, e)), _ran(view)
        assert len(got) == len(want) == count
        for k, (a, b) in enumerate(zip(got, want)):
            assert a == b, f"{label}: slot {e} differs from its uniform loop at lock step {k}"


def test_two_crowds_interleaved_and_ragged_equal_their_uniform_loops():
    """Crowds of 3 and 17 pedestrians (17 crosses the generator's 16-row tile), slot_crowd = [0, 1, 0, 1, 1, 0], six conditions
    on two paths in both plan modes.  Slot 0 reaches its goal at once (crowd 0's representative moves to slot 2); crowd 1 ends
    wholly in its wall, slot 1 first (its representative moves to slot 3), while crowd 0 runs on."""
    cfgs, pair, tracks, egos = two_crowds()
    w, n = _weights(), N_TWO
    uniform = uniform_views(w)
    counts = np.array([t.shape[1] for t in tracks])
    with sw.loop(cfgs, tracks, egos, _source(w, SLOT_CROWD), True) as res, \
            sw.loop(cfgs, tracks, egos, _source(w, SLOT_CROWD), False) as stp:
        assert res._sweep and res._resident_sampler and len(res.scenarios) >= 4
        s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
        shapes = _shapes_while_running(res, n)
        stp.run(n)
        steps = res.step_counts
        # the premises: the lowest slot of a crowd ended while another of its slots ran on -- in both crowds --, and crowd 1
        # ended wholly while crowd 0 ran
        assert 0 < steps[0] < min(steps[2], steps[5]), steps
        assert 0 < steps[1] < min(steps[3], steps[4]), steps
        assert max(steps[[1, 3, 4]]) < n == steps[2] == steps[5], steps
        # ... and the sampler's shape followed: the tables of the running slots, step by step
        seen = set()
        for k, (sel, shape) in enumerate(shapes):
            t = cr.crowd_tables(counts[sel], list(sel), SLOT_CROWD)
            assert shape == (len(t["scene_slot"]), t["scene_off"][-1]), (k, sel, shape)
            seen.add((shape, tuple(t["scene_slot"])))
        assert ((2, 20), (0, 1)) in seen and ((2, 20), (2, 1)) in seen and ((2, 20), (2, 3)) in seen and ((1, 3), (2,)) in seen, seen
        rs.assert_same_bytes(res, stp, s_res, s_stp, label="two crowds, resident against stepwise")
        assert_slots_equal_their_uniform_loops(res, uniform, "two crowds")


# ---- 3. slot_crowd = arange(n) is today's loop ---------------------------------------------------------------------------------------
def test_one_crowd_per_slot_is_todays_loop():
    """slot_crowd = arange(n) gives the bytes and the sampler shape (scenes = running slots) of the loop without the keyword,
    resident and stepwise."""
    cfgs, pair, tracks, egos = two_crowds()
    w, n = _weights(), N_TWO
    counts = np.array([t.shape[1] for t in tracks])
    every = list(range(len(tracks)))
    runs = {}
    # (sparse: one slot per crowd in the slots' order, the last crowd's id not its slot's -- no gather, another noise key;
    #  reversed: one slot per crowd in the opposite order -- the gather permutes)
    for name, crowd in (("parent", None), ("arange", every), ("sparse", every[:-1] + [9]), ("reversed", every[::-1])):
        with sw.loop(cfgs, tracks, egos, _source(w, crowd), True) as res, sw.loop(cfgs, tracks, egos, _source(w, crowd), False) as stp:
            s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
            shapes = _shapes_while_running(res, n)
            stp.run(n)
            rs.assert_same_bytes(res, stp, s_res, s_stp, label=f"{name}: resident against stepwise")
            for sel, shape in shapes:                                 # scenes = running slots, rows = their pedestrians
                assert shape == (len(sel), int(counts[sel].sum())), (name, sel, shape)
            runs[name] = ([rs.slot_view(res, e) for e in every], rs.run_bytes(res), [shape for _, shape in shapes], s_res)
    assert runs["arange"][0] == runs["parent"][0] and runs["arange"][1] == runs["parent"][1]
    assert runs["arange"][2] == runs["parent"][2] and len(set(runs["parent"][2])) > 2
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs["arange"][3], runs["parent"][3]))
    # crowd id = slot number for all slots but the last: those draw the parent's noise, the last one does not
    assert runs["sparse"][0][:-1] == runs["parent"][0][:-1] and runs["sparse"][0][-1] != runs["parent"][0][-1]
    assert runs["sparse"][2][0] == runs["parent"][2][0] == (len(every), int(counts.sum()))


# ---- 5. scores -------------------------------------------------------------------------------------------------------------------------
def test_scores_of_every_slot_equal_its_uniform_loop():
    """pred_len = 3: an origin's horizon is 12 lock steps, so the 24 steps complete some.  Every slot's prediction_metrics()
    and aggregate_metrics() row equals its uniform loop's."""
    cfgs, pair, tracks, egos = two_crowds(3)
    w = _weights(pred_len=3)
    uniform = uniform_views(w, 3, prediction_scores=True)
    with sw.loop(cfgs, tracks, egos, _source(w, SLOT_CROWD), True, prediction_scores=True) as sim:
        assert sim._sweep and sim._resident_scores
        sim.run(N_TWO)
        got, rows = sim.prediction_metrics(), sim.aggregate_metrics()
        assert_slots_equal_their_uniform_loops(sim, uniform, "scores")
        counted = 0
        for e in range(len(cfgs)):
            want, want_row = uniform[e][3], uniform[e][4]
            counted += want["ade_eval_count"]
            for k in METRIC_KEYS:
                assert sw.same_metric(got[e][k], want[k]), (e, k, got[e][k], want[k])
            assert set(rows[e]) == set(want_row)
            for k in want_row:
                assert sw.same_metric(rows[e][k], want_row[k]), (e, k, rows[e][k], want_row[k])
        assert counted > 0


# ---- 6. the noise key ---------------------------------------------------------------------------------------------------------------
def test_fot_sgan_noise_with_the_crowd_id_reproduces_a_step():
    """A slot of crowd 1 at a middle step: the raw words of fot_sgan_noise(seed, FOT_NOISE_RAW, row_slot = 1, the step of
    fot_loop_run_out.steps, row_index = 0 .. 16), mapped to [-1, 1) as the header states (exact in float32), fed through
    SganSampler.sample(window, noise=...) on the crowd's window and resampled, are the distribution block
    fot_debug_loop_block returns.  The loop's model draws noise_type 'uniform': of the two kinds a model reads, the one whose
    map from the raw words is exact."""
    import torch
    cfgs, pair, tracks, egos = two_crowds()
    w, k = _weights(), NOISE_STEP
    slot = 4                                                          # crowd 1, distribution mode, not its representative
    P = tracks[slot].shape[1]
    with sw.loop(cfgs, tracks, egos, _source(w, SLOT_CROWD, noise_type="uniform"), True) as sim:
        sim.run(k + 1)
        assert sim.alive[slot] and sim.alive[3] and sim._slot_aware[slot] and sim.engine.debug_loop_sampler_shape() == (2, 20)
        step = int(sim.step_counts[slot]) - 1                         # fot_loop_run_out.steps, before the step
        rec = sim._steps[k]
        what, window, sel, steps, o32, stale = rec["pred_src"][:6]
        i = int(np.flatnonzero(sel == slot)[0])
        lo, hi = int(rec["off"][i]), int(rec["off"][i + 1])
        assert what == "sgan" and hi - lo == P and step == k == int(steps[i])
        blk, pre = sim.engine.debug_loop_block(i, samples=S, cap_points=S * 64 * 64)
        assert pre == -1 and blk.shape[:2] == (S, P)
        nd = w.desc.noise_dim
        rows = dict(row_slot=np.full(P, SLOT_CROWD[slot]), row_step=np.full(P, step), row_index=np.arange(P))
        words = sim.engine.sgan_noise(SEED, _abi.NOISE_RAW, S, nd, **rows)
        noise = ((nc.uniform(words) - np.float32(0.5)) * np.float32(2.0)).astype(np.float32)
        assert noise.tobytes() == sim.engine.sgan_noise(SEED, _abi.NOISE_UNIFORM_SYM, S, nd, **rows).tobytes()
        # (the loop's own sampler object: handed its noise, it is fot_sgan_sample of one scene and looks at no crowd)
        raw = sim.sample_source.sample(window[:, lo:hi], np.array([0, P], np.int32), noise=noise)
        out = torch.zeros((S, P, blk.shape[2], 2), dtype=torch.float64, device=raw.device)
        torch.cuda.synchronize()
        T, _ = sim.resampler.resample_device(raw.data_ptr(), np.float32, S, P, o32[1][lo:hi].astype(np.float64), rec["pos"][lo:hi],
                                             stale, out.data_ptr(), np.float64)
        torch.cuda.synchronize()
        assert T == blk.shape[2] and out.cpu().numpy().tobytes() == blk.tobytes()
        # ... and not with the slot's own number in the key
        other = sim.engine.sgan_noise(SEED, _abi.NOISE_UNIFORM_SYM, S, nd, **dict(rows, row_slot=np.full(P, slot)))
        assert other.tobytes() != noise.tobytes()


def test_stepwise_sample_expands_the_crowds_and_refuses_other_windows():
    """SganSampler.sample with slot_crowd on its own: the slots of a crowd get the columns of ONE sampling -- the bytes the
    sampler without crowds gives slot c = crowd id --, in the order they were asked for; two slots of a crowd that observe
    different windows, or stand at different steps, are a ValueError."""
    import torch
    w = _weights()
    rng = np.random.default_rng(3)
    a, b = rng.normal(0.0, 2.0, (sc.OBS_LEN, 3, 2)).astype(np.float32), rng.normal(0.0, 2.0, (sc.OBS_LEN, 17, 2)).astype(np.float32)
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        plain = SganSampler(bp, w, S, counter_seed=SEED)
        want = plain.sample(np.concatenate([a, b], axis=1), np.array([0, 3, 20], np.int32), slots=[0, 1], steps=[7, 7]).cpu().numpy()
        shared = SganSampler(bp, w, S, counter_seed=SEED, slot_crowd=SLOT_CROWD)
        slots = [1, 2, 4, 5]                                          # crowds 1, 0, 1, 0: slot 0 is not asked for
        obs = np.concatenate([b, a, b, a], axis=1)
        off = np.array([0, 17, 20, 37, 40], np.int32)
        got = shared.sample(obs, off, slots=slots, steps=[7] * 4).cpu().numpy()
        cols = np.concatenate([np.arange(3, 20), np.arange(3), np.arange(3, 20), np.arange(3)])
        assert got.shape == (S, sc.PRED_LEN, 40, 2) and got.tobytes() == np.ascontiguousarray(want[:, :, cols]).tobytes()
        other = obs.copy()
        other[-1, 39, 0] = np.nextafter(other[-1, 39, 0], np.float32(np.inf))
        with pytest.raises(ValueError, match="crowd 0 do not observe the same window"):
            shared.sample(other, off, slots=slots, steps=[7] * 4)
        with pytest.raises(ValueError, match="slots 1 and 4 of crowd 1 differ"):
            shared.sample(obs, off, slots=slots, steps=[7, 7, 8, 7])
        with pytest.raises(ValueError, match="needs every scene's slot and step"):
            shared.sample(obs, off)
        assert torch.equal(shared.sample(obs, off, slots=slots, steps=[7] * 4), torch.from_numpy(got).to(shared.device))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_begin_drops_the_mode():
    lib = _abi.lib()
    w, G = _weights(), _abi.NOISE_GAUSSIAN
    c0, c1 = cr.crowds()
    aware = cr.base_config(distribution_aware_planning=True, pred_len=sc.PRED_LEN)
    cv_cfg = dict(aware, distribution_aware_planning=False, prediction_method="cv")
    n_run = 5

    def cv_run(tracks):
        with BatchedClosedLoop(cv_cfg, tracks, resident=True) as sim:
            sim.run(n_run)
            return rs.run_bytes(sim)

    def refused(h, code, *args, call="fot_loop_set_sampler_shared", names=()):
        assert getattr(lib, call)(h, *args) == code, (call, args)
        msg = lib.fot_last_error(h)
        assert call.encode() in msg and all(s.encode() in msg for s in names), msg

    def ids(*v):
        return np.array(v, np.int32)

    tracks = [c0, c1, c0, c1]
    want = cv_run(tracks)
    ok = ids(0, 1, 0, 1)
    with BatchedClosedLoop(cv_cfg, tracks, resident=True) as sim:
        h = sim.engine._h
        refused(h, _abi.ERR_INVALID, S, SEED, G, 2, ok.ctypes.data)                           # no model loaded
        refused(h, _abi.ERR_INVALID, None, None, call="fot_debug_loop_sampler_shape")          # no sampler
        SganSampler(sim.engine, w, S)
        refused(h, _abi.ERR_INVALID, S, SEED, G, 2, None)                                     # slot_crowd NULL
        refused(h, _abi.ERR_INVALID, S, SEED, G, 0, ok.ctypes.data)                           # n_crowds < 1
        for bad in (ids(0, 1, 0, 2), ids(0, -1, 0, 1)):                                       # an id out of range
            refused(h, _abi.ERR_INVALID, S, SEED, G, 2, bad.ctypes.data)
        both = ids(5, 5, 5, 5)
        refused(h, _abi.ERR_INVALID, S, SEED, G, 6, both.ctypes.data, names=("slots 0 and 1", "pedestrian counts"))
        refused(h, _abi.ERR_INVALID, 0, SEED, G, 2, ok.ctypes.data)                           # fot_loop_set_sampler's own: S < 1
        refused(h, _abi.ERR_UNSUPPORTED, _abi.MAX_SAMPLES + 1, SEED, G, 2, ok.ctypes.data)
        refused(h, _abi.ERR_INVALID, S, SEED, _abi.NOISE_RAW, 2, ok.ctypes.data)
        refused(h, _abi.ERR_INVALID, None, None, call="fot_debug_loop_sampler_shape")          # still no sampler
        sim.run(n_run)
        assert rs.run_bytes(sim) == want
        refused(h, _abi.ERR_INVALID, S, SEED, G, 2, ok.ctypes.data)                           # after the first step
    # two slots of a crowd that differ in n_frames / in one coordinate of the last frame
    last = c1.copy()
    last[-1, 16, 1] = np.nextafter(last[-1, 16, 1], np.inf)
    for other, names in ((c1[:-10], ("slots 1 and 3", "n_frames")), (last, ("slots 1 and 3", "pos"))):
        differ = [c0, c1, c0, other]
        want_d = cv_run(differ)
        with BatchedClosedLoop(cv_cfg, differ, resident=True) as sim:
            SganSampler(sim.engine, w, S)
            ego0 = sim.ego.copy()
            refused(sim.engine._h, _abi.ERR_INVALID, S, SEED, G, 2, ok.ctypes.data, names=names)
            sim.engine.loop_set_sampler(S, SEED, G, slot_crowd=[0, 1, 0, 3])                  # (each on a crowd of its own: accepted)
            _rebegin_cv(sim, cv_cfg, ego0)
            sim.run(n_run)
            assert rs.run_bytes(sim) == want_d
    # a refused call leaves an accepted one in force; fot_loop_begin* / fot_loop_set_replay drop the mode
    tracks = [c0, c1, c0, c1]
    with BatchedClosedLoop(aware, tracks, sample_source=_source(w, ok), device_samples=True, resident=True) as twin:
        twin.run(n_run)
        want_shared, shape = rs.run_bytes(twin), twin.engine.debug_loop_sampler_shape()
    assert shape == (2, 20)
    with BatchedClosedLoop(aware, tracks, sample_source=_source(w, ok), device_samples=True, resident=True) as sim:
        h, ego0 = sim.engine._h, sim.ego.copy()
        bad = ids(0, 1, 0, 2)
        refused(h, _abi.ERR_INVALID, S, SEED + 1, G, 2, bad.ctypes.data)
        refused(h, _abi.ERR_INVALID, S, SEED + 1, G, 2, None)
        assert sim.engine.debug_loop_sampler_shape() == (0, 0)                                 # (no lock step yet)
        sim.run(n_run)
        assert rs.run_bytes(sim) == want_shared and sim.engine.debug_loop_sampler_shape() == shape
        _rebegin_cv(sim, cv_cfg, ego0)
        refused(h, _abi.ERR_INVALID, None, None, call="fot_debug_loop_sampler_shape")          # the sampler went with the replay
        o = sim.engine.loop_run(n_run)
        with BatchedClosedLoop(cv_cfg, tracks, resident=True) as ref:
            want_o = ref.engine.loop_run(n_run)
        for key in ("ego", "jerk", "state", "stats", "followed", "keep", "cost", "after", "s_now", "steps", "termination"):
            assert np.ascontiguousarray(o[key]).tobytes() == np.ascontiguousarray(want_o[key]).tobytes(), key
        # ... and the slot-keyed sampler after a shared one is today's: scenes = running slots
        _rebegin_cv(sim, cv_cfg, ego0)
        sim.engine.loop_set_sampler(S, SEED, G)
        sim.engine.loop_run(1)
        assert sim.engine.debug_loop_sampler_shape() == (4, 40)


def _rebegin_cv(sim, cfg, ego0):
    """fot_loop_begin and fot_loop_set_replay on the loop's handle again: whatever predictor was set is dropped."""
    c = sim.config
    sim.engine.loop_begin(loop_config_from(c, constants_of(c), sim.MAX_REPLAN), ego0)
    sim.engine.loop_set_replay(sim.ped_off, sim.n_frames, sim._ped_all["trajectories"], sim._ped_all["velocities"],
                               obs_len=cfg["obs_len"], pred_len=sim.resampler.pred_len, rp=sim.resampler.params,
                               warmup_frames=int(cfg["obs_len"] * sim.sgan_dt / cfg["dt"]), ego_radius=sim.ego_radius,
                               ped_radius=sim.ped_radius, use_footprint=sim.footprint is not None,
                               s_end=float(np.ravel(sim.s_end)[0]), goal_distance=sim.GOAL_DISTANCE)
