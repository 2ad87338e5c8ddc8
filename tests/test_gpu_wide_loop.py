"""Closed loops, samplers and scores on sample distributions of more than 64 samples (a handle whose sample capacity was
raised: fot_set_sample_capacity, BatchPlanner / BatchedClosedLoop(sample_capacity=)) on the GPU: the capacity rule of every
entry that takes a distribution; the wide score kernel against the NumPy restatement; narrow launches on a raised handle
byte for byte against a fresh one; the wide selection and its planning block; reference episodes of 100 and 130 samples
through the one-call step and the resident loop; the resident Social-GAN sampler at 100 samples; a sweep at 100 samples.

On the parent commit every entry refuses S = 65, whatever the handle's capacity: the tests marked so below fail there."""
import numpy as np
import pytest

import loop_crowds_common as lc
import loop_sweep_common as sw
import recorded_samples_common as rs
from closed_loop_common import assert_episode_matches
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import (PredictionResampler, RecordedSamples, SganSampler, prediction_scores,
                                                     record_samples)
from pred_scores_common import assert_records_close, layouts, origin_terms, random_origin
from test_gpu_loop_sgan import SEED, _assert_same_bytes, _slot_view, _spy_s_now, case_weights, crowd_config, headline_episodes
from test_gpu_loop_sgan_scores import assert_metrics_equal
from test_gpu_rep_sample import REP, Frame, _begin, _check_frame, _requests
from wide_loop_common import load_wide_episodes, wide_sample_source

pytestmark = pytest.mark.gpu

MODEL = "a_pool_step_ped_bn"


def _engine(cap=None):
    return BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, sample_capacity=cap, **syn.CONFIG3_PLANNER)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _refused(call, S, cap, code=_abi.ERR_UNSUPPORTED):
    """The call raises the library's refusal; the message names S and the capacity."""
    with pytest.raises(_abi.FotError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if code == _abi.ERR_UNSUPPORTED:
        assert str(S) in str(e.value) and str(cap) in str(e.value), str(e.value)


# ---- 1. the capacity rule ---------------------------------------------------------------------------------------------------------
def test_every_entry_follows_the_handle_s_capacity():
    """One handle raised to 128: every entry that takes a distribution accepts 128 samples and refuses 129 with
    FOT_ERR_UNSUPPORTED; raised to 254, 254 pass.  (The parent refuses 65 everywhere.)"""
    rng = np.random.default_rng(1)
    w = case_weights(MODEL)
    with _engine(128) as bp:
        assert bp.sample_capacity == 128
        # fot_sgan_noise
        rows = (np.arange(3), np.zeros(3, np.int64), np.arange(3))
        assert bp.sgan_noise(SEED, _abi.NOISE_GAUSSIAN, 128, 4, *rows).shape == (128, 3, 4)
        _refused(lambda: bp.sgan_noise(SEED, _abi.NOISE_GAUSSIAN, 129, 4, *rows), 129, 128)
        # fot_prediction_scores
        dense, truth, stride = random_origin(rng, S=128, P=3, E=2, stride=1)
        rec = prediction_scores(bp, dense, truth, stride)
        assert_records_close(rec[0], origin_terms(dense, truth, stride), "S 128")
        dense9, truth9, _ = random_origin(rng, S=129, P=3, E=2, stride=1)
        _refused(lambda: prediction_scores(bp, dense9, truth9, 1), 129, 128)
        # fot_sgan_sample
        obs = rng.normal(0.0, 1.0, (w.desc.obs_len, 5, 2)).astype(np.float32)
        off = np.array([0, 2, 5], np.int32)
        out = SganSampler(bp, w, 128, seed=7, sample_capacity=128).sample(obs, off)
        assert tuple(out.shape) == (128, w.desc.pred_len, 5, 2)
        _refused(lambda: SganSampler(bp, w, 129, seed=7, sample_capacity=254).sample(obs, off), 129, 128)
        # fot_sgan_sample_model: two models on the handle, the scenes through model 1 under a given noise
        two = dict(counter_seed=SEED, slot_crowd=[0, 1], slot_model=[0, 1])
        noise = lambda S: rng.normal(0.0, 1.0, (S, 5, w.desc.noise_dim)).astype(np.float32)
        assert w.desc.noise_mix_type == _abi.SGAN_NOISE_PED
        out = SganSampler(bp, [w, w], 128, sample_capacity=128, **two).sample(obs, off, noise=noise(128), model=1)
        assert tuple(out.shape) == (128, w.desc.pred_len, 5, 2) and bool(np.isfinite(out.cpu().numpy()).all())
        _refused(lambda: SganSampler(bp, [w, w], 129, sample_capacity=254, **two).sample(obs, off, noise=noise(129), model=1),
                 129, 128)
        # fot_loop_plan / fot_loop_step frames with dist_raw, and fot_loop_prediction_scores on what they leave
        rsm = PredictionResampler(bp, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
        _begin(bp, 2)
        F = Frame(rsm, (3, 2), 128, seed=11)
        frame, eps = F.frame()
        recs, _ = bp.loop_plan(_requests(bp, F.egos[eps], range(2)), frame)
        assert len(recs) == 2 and (recs["stats_valid"] == 1).all()
        blk, _ = bp.debug_loop_block(0, samples=128)
        scored = bp.loop_prediction_scores(2, 4, 12, np.zeros((5, 12, 2)))
        assert list(scored["n_samples"]) == [128, 128] and list(scored["n_peds"]) == [3, 2]
        assert_records_close(scored[0], origin_terms(blk[:, :, 1:], np.zeros((3, 12, 2)), 4), "the frame's block")
        F9 = Frame(rsm, (3, 2), 129, seed=12)
        frame9, _ = F9.frame()
        _refused(lambda: bp.loop_plan(_requests(bp, F9.egos[eps], range(2)), frame9), 129, 128)
        again, _ = bp.loop_plan(_requests(bp, F.egos[eps], range(2)), F.frame()[0])          # (the handle goes on)
        assert again.tobytes() == recs.tobytes()
        # fot_loop_step: the same frames behind the one-call step
        step_frame = lambda fr: {k: v for k, v in fr.items() if k != "ego"}
        _begin(bp, 2)
        _refused(lambda: bp.loop_step(step_frame(frame9), np.arange(2)), 129, 128)
        stepped = bp.loop_step(step_frame(F.frame()[0]), np.arange(2))
        assert len(stepped["ego"]) == 2 and len(stepped["records"]) >= 2
        bp.set_sample_capacity(254)
        again9, _ = bp.loop_plan(_requests(bp, F9.egos[eps], range(2)), frame9)
        assert len(again9) == 2
        assert bp.sgan_noise(SEED, _abi.NOISE_GAUSSIAN, 254, 4, *rows).shape == (254, 3, 4)
        dense254, truth254, _ = random_origin(rng, S=254, P=3, E=2, stride=1)
        assert_records_close(prediction_scores(bp, dense254, truth254, 1)[0], origin_terms(dense254, truth254, 1), "S 254")


def test_resident_entries_follow_the_handle_s_capacity():
    """fot_loop_set_samples(_shared), fot_loop_set_sampler(_shared, _models) and fot_loop_scores_enable on a loop whose
    engine was raised to 128; a refused call changes nothing; the capacity cannot fall below a loop that is set up."""
    cfg, tracks = headline_episodes()
    w = case_weights(MODEL)
    n_cols, L = sum(t.shape[1] for t in tracks), int(cfg["pred_len"])
    G = _abi.NOISE_GAUSSIAN
    cv_cfg = dict(cfg, prediction_method="cv", distribution_aware_planning=False)     # (the predictor is set on the engine below)
    with BatchedClosedLoop(cv_cfg, tracks, resident=True, sample_capacity=128) as sim:
        eng = sim.engine
        assert eng.sample_capacity == 128
        SganSampler(eng, w, 4, counter_seed=SEED)                                         # (loads the model into the handle)
        wide = np.zeros((2, 129, L, n_cols, 2), np.float32)
        _refused(lambda: eng.loop_set_samples(wide), 129, 128)
        _refused(lambda: eng.loop_set_samples(wide, slot_col0=[0, tracks[0].shape[1], tracks[0].shape[1]]), 129, 128)
        for kw in ({}, dict(slot_crowd=[0, 1, 2]), dict(slot_crowd=[0, 1, 2], slot_model=[0, 0, 0], model_kinds=[G])):
            _refused(lambda kw=kw: eng.loop_set_sampler(129, SEED, G, **kw), 129, 128)
        _refused(lambda: eng.loop_scores_enable(True), 0, 0, code=_abi.ERR_INVALID)       # nothing was set: no predictor
        eng.set_sample_capacity(64)                                                       # ... and no loop holds the capacity up
        eng.set_sample_capacity(128)
        eng.loop_set_sampler(128, SEED, G)
        eng.loop_scores_enable(True)
        _refused(lambda: eng.set_sample_capacity(127), 0, 0, code=_abi.ERR_INVALID)
        assert eng.sample_capacity == 128
        out = eng.loop_run(2, keep_paths=False)
        assert out["n_steps"] == 2
        eng.set_sample_capacity(254)
        assert eng.sample_capacity == 254
    # accepted at 128 and run: crowd-shared sampler, a model per slot, a shared recording (slots 0 and 1 replay one crowd)
    pair = [tracks[2], tracks[2], tracks[0]]
    P2 = tracks[2].shape[1]
    accepted = (lambda e: e.loop_set_sampler(128, SEED, G, slot_crowd=[0, 0, 1]),
                lambda e: e.loop_set_sampler(128, SEED, G, slot_crowd=[0, 0, 1], slot_model=[0, 1, 0], model_kinds=[G, G]),
                lambda e: e.loop_set_samples(np.zeros((2, 128, L, P2 + 3, 2), np.float32), slot_col0=[0, 0, P2]))
    for k, accept in enumerate(accepted):
        with BatchedClosedLoop(cv_cfg, pair, resident=True, sample_capacity=128) as sim:
            SganSampler(sim.engine, [w, w], 4, counter_seed=SEED, slot_crowd=[0, 0, 1], slot_model=[0, 1, 0])   # (models 0 and 1)
            SganSampler(sim.engine, w, 4, counter_seed=SEED)                                               # (fot_sgan_load)
            accept(sim.engine)
            sim.engine.loop_scores_enable(True)
            out = sim.engine.loop_run(2, keep_paths=False)
            assert out["n_steps"] == 2 and (out["followed"][0] >= 0).all(), f"form {k}"
            if k < 2:                                                 # one sampling per crowd / per (crowd, model) unit
                assert sim.engine.debug_loop_sampler_shape() == ((2, P2 + 3), (3, 2 * P2 + 3))[k], f"form {k}"
    with BatchedClosedLoop(cv_cfg, tracks, resident=True, sample_capacity=128) as sim:
        sim.engine.loop_set_samples(np.zeros((2, 128, L, n_cols, 2), np.float32))
        sim.engine.loop_scores_enable(True)
        _refused(lambda: sim.engine.set_sample_capacity(64), 0, 0, code=_abi.ERR_INVALID)


# ---- 2. fot_prediction_scores ------------------------------------------------------------------------------------------------------
WIDE_S, WIDE_P = (65, 128, 129, 254), (1, 33, 65, 270)


@pytest.fixture(scope="module")
def raised():
    with _engine(254) as bp:
        yield bp


@pytest.mark.parametrize("t_major", [False, True], ids=["spt", "tsp"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("E", [1, 12])
def test_wide_scores_equal_the_restatement(raised, E, dtype, t_major):
    """S on both sides of 128 and at the top, P on both sides of a wave and of the 256-lane pass; an origin without
    pedestrians and one of 254 equal samples (no KDE) among them, all in ONE launch."""
    rng = np.random.default_rng(200 + E)
    cases = [random_origin(rng, S=S, P=P, E=E, stride=1) for S in WIDE_S for P in WIDE_P]
    same = random_origin(rng, S=254, P=7, E=E, stride=1)
    same[0][:] = same[0][:1]
    none = (np.zeros((254, 0, E + 1, 2)), np.zeros((0, E, 2)), 1)
    cases += [same, none]
    blocks = [layouts(d, t_major, 1, dtype) for d, _, _ in cases]
    recs = prediction_scores(raised, blocks, [t for _, t, _ in cases], 1, t_major=t_major, skip=1)
    assert len(recs) == len(cases)
    for (dense, truth, _), rec in zip(cases, recs):
        seen = dense.astype(dtype).astype(np.float64)                  # (a float32 tensor: the scores of the rounded samples)
        assert_records_close(rec, origin_terms(seen, truth, 1), f"S {dense.shape[0]} P {dense.shape[1]} E {E}")
    assert recs[-2]["flags"] & _abi.PRED_NLL == 0 and recs[-2]["nll_count"] == 0 and recs[-2]["n_samples"] == 254
    assert recs[-1]["n_peds"] == 0 and recs[-1]["n_samples"] == 254


def test_an_origin_s_record_does_not_depend_on_its_company(raised):
    """S = 20 and S = 200 origins in one launch (the wide kernel runs both): each record is the bytes of the origin alone
    (the narrow one alone: today's kernel)."""
    rng = np.random.default_rng(21)
    cases = [random_origin(rng, S=S, P=P, E=12, stride=1) for S, P in ((20, 33), (200, 65), (20, 270), (200, 1))]
    blocks, truths = [d for d, _, _ in cases], [t for _, t, _ in cases]
    together = prediction_scores(raised, blocks, truths, 1)
    for i, (b, t) in enumerate(zip(blocks, truths)):
        alone = prediction_scores(raised, [b], [t], 1)
        assert alone[0].tobytes() == together[i].tobytes(), f"origin {i}"


# ---- 3. narrow launches are today's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 20, 64])
def test_narrow_launches_on_a_raised_handle_are_a_fresh_handle_s_bytes(S):
    rng = np.random.default_rng(30 + S)
    cases = [random_origin(rng, S=S, P=P, E=12, stride=1) for P in (1, 65, 270)]
    blocks, truths = [d for d, _, _ in cases], [t for _, t, _ in cases]
    got = []
    for cap in (None, 254):
        with _engine(cap) as bp:
            got.append(prediction_scores(bp, blocks, truths, 1).tobytes())
    assert got[0] == got[1]
    # a 10-step resident recorded loop that plans on the representative sample and scores: records, choices, metrics
    cfg = dict(rs.ragged_config(), distribution_aware_planning=False)
    tracks, egos = rs.ragged_tracks(), rs.ragged_egos(cfg)
    rec = rs.scripted_recording(cfg, tracks, S, 10, dtype=np.float64).samples
    runs = []
    for cap in (None, 254):
        with BatchedClosedLoop(cfg, tracks, egos, sample_source=RecordedSamples(rec), device_samples=True, resident=True,
                               plan_on_representative_sample=True, prediction_scores=True, sample_capacity=cap) as sim:
            assert sim.engine.sample_capacity == (cap or 64)
            sim.run(10)
            best = [None if s.best is None else np.asarray(s.best).tobytes() for s in sim._steps]
            blocks_ = [sim.engine.debug_loop_block(i)[0].tobytes() for i in range(len(sim._steps[-1]["sel"]))]
            runs.append((rs.run_bytes(sim), [rs.slot_view(sim, e) for e in range(len(tracks))], best, blocks_,
                         repr(sim.prediction_metrics()), sim.engine.loop_score_summaries().tobytes()))
    assert runs[0] == runs[1]
    assert any(b is not None for b in runs[0][2])


# ---- 4. the representative sample --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [65, 254])
def test_wide_selection_and_planning_block_equal_the_host_construction(raised, S):
    """Episodes of 1, 5, 6, 65, 0 and 3 pedestrians in one loop (n_dense = 50: 250 and 300 points fall either side of 256
    lanes): fot_loop_last_best_sample is NumPy's predict_single_best, fot_debug_loop_block that sample's block bit for bit,
    the records those of a plan call on the host-built block."""
    bp = raised
    rsm = PredictionResampler(bp, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
    assert rsm.n_dense == 50
    counts = (1, 5, 6, 65, 0, 3)
    _begin(bp, len(counts))
    bp.loop_plan_sample(REP)
    F = Frame(rsm, counts, S, seed=5100 + S)
    _, want = _check_frame(bp, F)
    assert [b >= 0 for _, _, b in want] == [c > 0 for c in counts]


def test_wide_selection_exact_tie_across_sample_64(raised):
    """Samples 63 and 64 are the same numbers and lie at the centre of the fan: an exact tie of the two smallest deviation
    sums; the first wins, on the device as in NumPy."""
    import torch
    bp = raised
    rsm = PredictionResampler(bp, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
    counts = (5, 65, 6)
    _begin(bp, len(counts))
    bp.loop_plan_sample(REP)
    F = Frame(rsm, counts, 130, seed=5200)
    centre = F.raw.mean(axis=0)
    F.raw[63] = centre
    F.raw[64] = centre
    F.raw_dev = torch.from_numpy(np.ascontiguousarray(F.raw)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    _, want = _check_frame(bp, F, gap=False)
    assert [b for _, _, b in want] == [63, 63, 63]


# ---- 5. the reference episodes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s100_eps01", "s130_eps0"])
def test_reference_episodes_of_more_than_64_samples(name):
    """100 samples under a budget of exactly one, 130 samples with none: the one-call step on the scripted source's device
    tensor and the resident loop on its recording, each against the reference simulator's episode; resident and stepwise
    byte for byte.  (The parent refuses the first frame.)"""
    import torch
    ep = load_wide_episodes()
    var = ep["meta"]["variants"][name]
    cfg, S = dict(var["config"]), int(var["n_samples"])
    host_src = wide_sample_source(S, cfg["pred_len"])
    dev = torch.device("cuda", 0)
    dev_src = lambda last, prev: torch.from_numpy(np.ascontiguousarray(host_src(last, prev), dtype=np.float64)).to(dev)
    tracks = [ep[name + "_ped_traj"]] * 2
    with BatchedClosedLoop(cfg, tracks, sample_source=dev_src, device_samples=True, sample_capacity=S) as sim:
        assert sim._native and sim._device_samples and sim.distribution_aware
        hists = sim.run()
        for h, e in zip(hists, sim.episodes):
            assert_episode_matches(h, e.termination_reason, ep, name)
    rec = record_samples(cfg, tracks, host_src, int(var["steps"]), dtype=np.float64, device="cuda", sample_capacity=S)
    assert rec.num_samples == S and rec.samples.is_cuda
    with BatchedClosedLoop(cfg, tracks, sample_source=rec, device_samples=True, resident=True, sample_capacity=S) as res, \
            BatchedClosedLoop(cfg, tracks, sample_source=rec, device_samples=True, sample_capacity=S) as stp:
        assert res._resident and res._resident_recording and stp._native and not stp._resident
        s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
        hists = res.run()
        stp.run()
        for h, e in zip(hists, res.episodes):
            assert_episode_matches(h, e.termination_reason, ep, name)
        rs.assert_same_bytes(res, stp, s_res, s_stp, label=name)


# ---- 6. the resident Social-GAN sampler --------------------------------------------------------------------------------------------
S_GAN, N_GAN = 100, 12


def _gan_source(w, S=S_GAN):
    return SganSampler(None, w, S, counter_seed=SEED, sample_capacity=max(S, 64))


def test_resident_sampler_at_100_samples():
    """Crowds of 1, 65 and 0 pedestrians, 12 lock steps: resident == stepwise byte for byte, the prediction metrics equal,
    a slot alone == the slot in company, and -- the noise is keyed by the sample's id -- samples 0 .. 63 of a step's
    tensor are what a sampler of 64 samples with the same seed draws."""
    cfg = crowd_config()
    counts = (1, 65, 0)
    tracks = lc.crowd_tracks(counts, 60, lc.TRACK_SEED)
    w = case_weights(MODEL)
    kw = dict(device_samples=True, prediction_scores=True, sample_capacity=S_GAN)
    with BatchedClosedLoop(cfg, tracks, sample_source=_gan_source(w), resident=True, **kw) as res, \
            BatchedClosedLoop(cfg, tracks, sample_source=_gan_source(w), **kw) as stp:
        assert res._resident and res._resident_sampler and res._resident_scores and stp._native and not stp._resident
        s_res, s_stp = _spy_s_now(res), _spy_s_now(stp)
        res.run(N_GAN)
        stp.run(N_GAN)
        _assert_same_bytes(res, stp, s_res, s_stp, label="S 100")
        assert_metrics_equal(res.prediction_metrics(), stp.prediction_metrics(), "S 100")
        company = _slot_view(res, 1)
        # the prefix property, on the stepwise loop's engine: the window of lock step 0 under both sample counts
        obs = np.stack(list(stp.observer.history), axis=0).astype(np.float32)
        off = stp.ped_off.astype(np.int32)
        slots, steps = np.arange(len(counts)), np.full(len(counts), 5)
        wide = SganSampler(stp.engine, w, S_GAN, counter_seed=SEED, sample_capacity=S_GAN).sample(obs, off, slots=slots, steps=steps)
        narrow = SganSampler(stp.engine, w, 64, counter_seed=SEED).sample(obs, off, slots=slots, steps=steps)
        assert tuple(wide.shape)[0] == S_GAN and tuple(narrow.shape)[0] == 64
        assert wide[:64].cpu().numpy().tobytes() == narrow.cpu().numpy().tobytes()
    solo = [tracks[0][:, :0], tracks[1], tracks[2]]
    with BatchedClosedLoop(cfg, solo, sample_source=_gan_source(w), resident=True, **kw) as sim:
        sim.run(N_GAN)
        assert _slot_view(sim, 1) == company


# ---- 7. a sweep ---------------------------------------------------------------------------------------------------------------------
def test_sweep_at_100_samples_over_one_shared_recording():
    """4 slots = 2 crowds x {the whole distribution under eps = 0.01 -- one sample may hit --, the representative sample}
    over ONE recording (slot_col0): every slot's history is the bits of the uniform loop of its own configuration."""
    ep = load_wide_episodes()
    var = ep["meta"]["variants"]["s100_eps01"]
    base, S, n = dict(var["config"]), 100, 30
    crowd_a = ep["s100_eps01_ped_traj"]
    crowd_b = ep["s130_eps0_ped_traj"][:, :7]
    conds = [dict(base, distribution_aware_planning=True, chance_epsilon=0.01), dict(base, distribution_aware_planning=False)]
    cfgs = [conds[0], conds[1], conds[0], conds[1]]
    tracks = [crowd_a, crowd_a, crowd_b, crowd_b]
    Pa = crowd_a.shape[1]
    both = np.concatenate([crowd_a, crowd_b], axis=1)
    one = record_samples(cfgs[0], [both], wide_sample_source(S, base["pred_len"]), n, dtype=np.float64, sample_capacity=S).samples
    col0 = [0, 0, Pa, Pa]
    shared = lambda: RecordedSamples(_cuda(one), slot_col0=col0, sample_capacity=S)
    with sw.loop(cfgs, tracks, None, shared(), True, sample_capacity=S) as sweep:
        assert sweep._sweep and sweep._resident_recording and list(sweep._slot_aware) == [True, False, True, False]
        sweep.run(n)
        views = [rs.slot_view(sweep, e) for e in range(4)]
        counts, term = sweep.step_counts.copy(), sweep.termination.copy()
        assert (np.asarray(sweep._steps[-1].best)[[1, 3]] >= 0).all() or not sweep.alive[[1, 3]].all()
    for c, cond in enumerate(conds):
        with sw.loop(cond, tracks, None, shared(), True, sample_capacity=S) as uni:
            assert not uni._sweep
            uni.run(n)
            for e in (c, c + 2):
                assert uni.step_counts[e] == counts[e] and uni.termination[e] == term[e], f"slot {e}"
                assert rs.slot_view(uni, e) == views[e], f"slot {e} differs from the uniform loop of its configuration"
    assert views[0] != views[1] or views[2] != views[3]                 # (the plan mode matters on these crowds)


# ---- 8. crowd-shared sampling and a model per slot --------------------------------------------------------------------------------
def test_shared_crowd_and_per_slot_models_at_100_samples():
    """Four conditions over one crowd, slot_model = [0, 0, 1, 1] (a pooled model and one without pooling, of other
    dimensions), 100 samples: the resident loop equals the stepwise one byte for byte (one sampling per (crowd, model) unit
    and lock step, the per-model raw tensors gathered into the step's), and slots 0, 1 are the crowd-shared loop on a handle
    whose only model is the pooled one -- itself resident == stepwise."""
    import loop_models_common as lm
    import sgan_common as sc
    from test_gpu_loop_models import K_CONDITIONS, assert_slot_equals
    ref, crowd, _, steps, _ = rs.reference_case("s6_eps02")
    n, S = 12, 100
    assert steps >= n
    cfgs = [dict(ref, pred_len=sc.PRED_LEN, distribution_aware_planning=a, chance_epsilon=e, collision_margin_inflation=m)
            for a, e, m in K_CONDITIONS]
    w = [lm.weights(lm.POOLED), lm.weights(lm.NO_POOLING)]
    P, tracks = crowd.shape[1], [crowd] * 4
    models = lambda: SganSampler(None, list(w), S, counter_seed=SEED, slot_crowd=[0] * 4, slot_model=[0, 0, 1, 1], sample_capacity=S)
    shared = lambda: SganSampler(None, w[0], S, counter_seed=SEED, slot_crowd=[0, 0], sample_capacity=S)
    with sw.loop(cfgs, tracks, None, models(), True, sample_capacity=S) as res, \
            sw.loop(cfgs, tracks, None, models(), False, sample_capacity=S) as stp:
        assert res._sweep and res._resident_sampler and stp._sweep and not stp._resident
        s_res, s_stp = rs.spy_s_now(res), rs.spy_s_now(stp)
        res.run(n)
        stp.run(n)
        assert res.engine.debug_loop_sampler_shapes(2) == [(1, P), (1, P)]
        rs.assert_same_bytes(res, stp, s_res, s_stp, label="two models at 100 samples")
        with sw.loop(cfgs[:2], tracks[:2], None, shared(), True, sample_capacity=S) as one, \
                sw.loop(cfgs[:2], tracks[:2], None, shared(), False, sample_capacity=S) as one_stp:
            assert one._sweep and one._resident_sampler
            s_one, s_one_stp = rs.spy_s_now(one), rs.spy_s_now(one_stp)
            one.run(n)
            one_stp.run(n)
            assert one.engine.debug_loop_sampler_shape() == (1, P)
            rs.assert_same_bytes(one, one_stp, s_one, s_one_stp, label="shared crowd at 100 samples")
            for e in (0, 1):
                assert_slot_equals(res, e, one, e, "the pooled model")
