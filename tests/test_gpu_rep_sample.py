"""Planning on the representative prediction sample with the samples resident in HBM (fot_loop_plan_sample,
k_loop_rep_block, BatchedClosedLoop(plan_on_representative_sample=True)) on the GPU: the reference's own default
configuration (s5_best_only) through the one-call step; the fixed-shape block and the step's records against the host's
construction, kernel shape by kernel shape; the per-episode prepend at its threshold; the resident sampler loop byte for
byte against the stepwise loop and step by step against the five-call route; the mode left off; the refusals.

Every test here fails without the feature: the entry points and the keyword do not exist."""
import math

import numpy as np
import pytest

import rep_sample_common as rc
from closed_loop_common import (assert_episode_matches, load_dist_episodes, load_episodes, scenario_config,
                                scripted_sample_source)
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop, constants_of, loop_config_from
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import PredictionResampler, SganSampler
from pred_scores_common import METRIC_KEYS
from test_gpu_closed_loop import _same_histories
from test_gpu_loop_sgan import SEED, _assert_same_bytes, _run_bytes, _spy_s_now, case_weights

pytestmark = pytest.mark.gpu

REP = _abi.LOOP_PLAN_REPRESENTATIVE
NAME = "s5_best_only"


def _nan_equal(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


# ---- 5. the reference's default configuration ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_runs():
    """s5_best_only (distribution_aware_planning unset, 5 samples): two copies through the one-call step with the scripted
    source's samples as a device tensor, and through the host hand-over; both scored."""
    import torch
    ep = load_dist_episodes()
    var = ep["meta"]["variants"][NAME]
    cfg = dict(var["config"])
    assert not cfg.get("distribution_aware_planning", False)
    host_src = scripted_sample_source(var["n_samples"], cfg["pred_len"])
    dev = torch.device("cuda", 0)
    dev_src = lambda last, prev: torch.from_numpy(np.ascontiguousarray(host_src(last, prev), dtype=np.float64)).to(dev)
    tracks = [ep[NAME + "_ped_traj"]] * 2
    out = dict(ep=ep)
    with BatchedClosedLoop(cfg, tracks, sample_source=dev_src, device_samples=True, plan_on_representative_sample=True,
                           prediction_scores=True) as sim:
        assert sim._native and sim._device_samples and not sim.distribution_aware
        hists = sim.run()
        out["dev"] = [list(h) for h in hists]
        out["dev_term"] = [e.termination_reason for e in sim.episodes]
        out["dev_metrics"] = sim.prediction_metrics()
    with BatchedClosedLoop(cfg, tracks, sample_source=host_src, prediction_scores=True) as sim:
        assert not sim._native
        out["host"] = [list(h) for h in sim.run()]
        out["host_metrics"] = sim.prediction_metrics()
    return out


def test_reference_episode_with_its_samples_never_leaving_hbm(reference_runs):
    r = reference_runs
    for h, term in zip(r["dev"], r["dev_term"]):
        assert_episode_matches(h, term, r["ep"], NAME)
    _same_histories(r["host"], r["dev"])


def test_reference_episode_scores_equal_the_host_run_s(reference_runs):
    r = reference_runs
    for got, want in zip(r["dev_metrics"], r["host_metrics"]):
        assert tuple(got) == METRIC_KEYS
        for k in METRIC_KEYS:
            assert _nan_equal(got[k], want[k]), (k, got[k], want[k])
    assert r["dev_metrics"][0]["ade_eval_count"] > 0


# ---- 6. the kernel against the host's construction ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bp():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as b:
        yield b


def _loop_cfg():
    c = type("Cfg", (), scenario_config(load_episodes()["meta"], "base"))
    return loop_config_from(c, constants_of(c), 3)


def _begin(bp, n):
    ego5 = np.zeros((n, 5))
    bp.loop_begin(_loop_cfg(), ego5)
    bp.loop_set_static(None)


def _requests(bp, egos, episodes, target=8.0):
    req = np.zeros(len(egos), dtype=bp.LOOP_REQUEST_DT)
    for j, (e, ep) in enumerate(zip(egos, episodes)):
        for col, f in enumerate(("x", "y", "yaw", "v", "a")):
            req["ego"][f][j] = e[col]
        req["overrides"][j] = (np.nan, np.nan, np.nan, np.nan)
        req["target_speed"][j], req["max_stop_distance"][j], req["episode"][j] = target, np.nan, ep
    return req


def _same_records(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    for name in a.dtype.names:
        if not name.startswith("_"):
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)


class Frame:
    """A lock step's frame with raw samples of a multi-sample predictor in device memory: `counts` pedestrians per
    episode walking near the ego's lattice, S samples each; the episodes of `stand` stand still and all their samples
    equal the anchor (the first dense sample then IS the current position)."""

    def __init__(self, rs, counts, S, seed, stand=(), stale=0.1, equal_samples=False):
        import torch
        rng = np.random.default_rng(seed)
        self.off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n, L = int(self.off[-1]), rs.pred_len
        pos = np.column_stack([rng.uniform(8.0, 45.0, n), rng.uniform(-4.0, 4.0, n)])
        vel = rng.normal(0.0, 1.0, (n, 2))
        last = (pos + rng.normal(0.0, 0.01, pos.shape)).astype(np.float32)
        prev = (last.astype(np.float64) - 0.4 * vel).astype(np.float32)
        a = last.astype(np.float64)
        raw = np.zeros((S, L, n, 2))
        for s in range(S):
            v = vel * (1.0 + 0.1 * rng.normal(size=(n, 1))) + rng.normal(0.0, 0.15, (n, 2))
            raw[s] = a[None] + ((np.arange(L) + 1.0) * 0.4)[:, None, None] * v[None]
        if equal_samples:
            raw[1:] = raw[0]
        for e in stand:
            lo, hi = self.off[e], self.off[e + 1]
            pos[lo:hi] = a[lo:hi]
            vel[lo:hi] = 0.0
            prev[lo:hi] = last[lo:hi]
            raw[:, :, lo:hi] = a[lo:hi]
        self.pos, self.vel, self.last, self.prev, self.raw, self.S, self.stale, self.rs = pos, vel, last, prev, raw, S, stale, rs
        self.n_ep = len(counts)
        self.egos = np.column_stack([rng.uniform(0.0, 6.0, self.n_ep), rng.normal(0.0, 0.3, self.n_ep), np.zeros(self.n_ep),
                                     rng.uniform(4.0, 8.0, self.n_ep), np.zeros(self.n_ep)])
        self.raw_dev = torch.from_numpy(np.ascontiguousarray(raw)).to(torch.device("cuda", 0))
        torch.cuda.synchronize()

    def frame(self, episodes=None):
        """The frame of all episodes, or of the episodes `episodes` alone (their rows of every array)."""
        import torch
        eps = list(range(self.n_ep)) if episodes is None else list(episodes)
        rows = np.concatenate([np.arange(self.off[e], self.off[e + 1]) for e in eps]).astype(np.int64) if eps else np.zeros(0, np.int64)
        off = np.concatenate([[0], np.cumsum([self.off[e + 1] - self.off[e] for e in eps])]).astype(np.int64)
        raw_dev = self.raw_dev if episodes is None else self.raw_dev[:, :, torch.from_numpy(rows).to(self.raw_dev.device)].contiguous()
        torch.cuda.synchronize()
        f = dict(ped_off=off, ped_pos=self.pos[rows], ped_vel=self.vel[rows], obs_last=self.last[rows], obs_prev=self.prev[rows],
                 prepend=np.ones(len(eps), bool), staleness=self.stale, pred_len=self.rs.pred_len, rp=self.rs.params,
                 ego=self.egos[eps, :4], ego_radius=1.0, ped_radius=0.3, use_footprint=False)
        if len(rows):
            f.update(dist_raw=raw_dev.data_ptr(), dist_S=self.S, dist_dtype=_abi.F64, _raw=raw_dev)
        return f, eps

    def host_blocks(self, best=None):
        """Per episode (block [P, n_dense + 1, 2], prepended, chosen sample) from fot_resample_predictions' output of the
        same raw samples, NumPy's selection (or the given one) and the rule; the deviation gaps beside them."""
        dist = self.rs.process_prediction(self.raw, anchor_pos=self.last.astype(np.float64), staleness=self.stale)
        best = rc.host_choice(dist, self.off) if best is None else best
        out = []
        for e in range(self.n_ep):
            lo, hi = self.off[e], self.off[e + 1]
            if hi == lo:
                out.append((np.zeros((0, self.rs.n_dense + 1, 2)), -1, -1))
                continue
            blk, pre = rc.host_block(dist[best[e], lo:hi], self.pos[lo:hi])
            out.append((blk, int(pre), int(best[e])))
        return out, rc.gaps(dist, self.off)


def _check_frame(bp, F, episodes=None, gap=True, device_choice=False):
    """One lock step in mode 1 through fot_loop_plan: blocks, flags and the chosen samples against the host's, the records
    against fot_plan_batch on the host-built tensor with FOT_DYN_SINGLE.  Returns the records.  device_choice: the host
    builds its blocks from the samples the device reports (sums that tie to rounding: the rule leaves the choice open)."""
    frame, eps = F.frame(episodes)
    req = _requests(bp, F.egos[eps], range(len(eps)))
    rec, _ = bp.loop_plan(req, frame)
    rec = rec.copy()
    best = bp.loop_last_best_sample()
    if device_choice:
        assert episodes is None
        counts = np.diff(F.off)
        assert ((best[:F.n_ep] >= 0) & (best[:F.n_ep] < F.S))[counts > 0].all() and (best[:F.n_ep][counts == 0] == -1).all()
    want, g = F.host_blocks(best[:F.n_ep].copy() if device_choice else None)
    if gap:
        assert (g > rc.GAP).all(), f"a near-tie among the deviation sums ({g.min()}): choose another seed"
    blocks, d_off, dims, cursor = [], [], [], 0
    for i, e in enumerate(eps):
        blk, pre, b = want[e]
        got, got_pre = bp.debug_loop_block(i)
        assert got.shape == (1,) + blk.shape, (e, got.shape, blk.shape)
        assert got_pre == pre, f"episode {e}: prepended {got_pre}, host {pre}"
        assert got.tobytes() == np.ascontiguousarray(blk).tobytes(), f"episode {e}: block differs"
        assert best[i] == b, f"episode {e}: sample {best[i]}, host {b}"
        d_off.append(cursor)
        dims.append((1 if len(blk) else 0, 1, len(blk), blk.shape[1]))
        blocks.append(blk.reshape(-1, 2))
        cursor += len(blk) * blk.shape[1]
    assert (best[len(eps):] == -1).all()
    ego = np.zeros(len(eps), dtype=bp.EGO_DT)
    for col, f in enumerate(("x", "y", "yaw", "v", "a")):
        ego[f] = F.egos[eps, col]
    d_xy = np.concatenate(blocks) if cursor else None
    ref = bp.plan_arrays(ego, np.full(len(eps), 8.0), np.full((len(eps), 4), np.nan), np.full(len(eps), np.nan), None, None,
                         d_xy, np.array(d_off) if cursor else None, np.array(dims) if cursor else None)
    _same_records(rec, ref)
    return rec, want


SHAPES = [((1,), 2), ((5,), 2), ((6,), 2), ((63,), 2), ((64,), 2), ((65,), 2),      # 250 / 300 points: either side of 256 lanes
          ((5,), 1), ((6,), 64), ((65,), 64),                                        # S of 1 and FOT_MAX_SAMPLES
          ((0, 5, 3), 2), ((4, 0, 7), 2), ((6, 2, 0), 2),                            # no pedestrians first / in the middle / last
          ((1, 65, 5, 64, 6), 3)]                                                    # episodes that differ in P


@pytest.mark.parametrize("counts,S", SHAPES, ids=[f"P{'_'.join(map(str, c))}_S{s}" for c, s in SHAPES])
def test_block_and_records_equal_the_host_construction(bp, counts, S):
    rs = PredictionResampler(bp, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
    assert rs.n_dense == 50
    _begin(bp, len(counts))
    bp.loop_plan_sample(REP)
    # (two samples lie symmetrically about their mean: their sums tie to rounding and the order of summation decides.  With
    #  both samples equal the tie is exact and the first one wins under any order; two distinct samples: the test below)
    F = Frame(rs, counts, S, seed=4100 + 17 * sum(counts) + S, equal_samples=S == 2)
    rec, want = _check_frame(bp, F, gap=S != 2)
    if len(counts) == 5:
        assert (rec["stats"][:, _abi.ST_COLLISION] > 0).any()       # (the blocks matter to the records)
    if S == 2:
        assert all(b == 0 for blk, _, b in want if len(blk))
    assert all(pre == 1 for blk, pre, _ in want if len(blk))        # walking crowds: the current positions lead
    # the escalation levels arrive without a frame and plan against the same blocks
    e = int(np.argmax(counts))
    again, none = bp.loop_plan(_requests(bp, F.egos[[e]], [e]))
    assert none is None
    _same_records(again, rec[[e]])


@pytest.mark.parametrize("counts", [(5,), (6,), (65, 0, 3)], ids=["P5", "P6", "P65_0_3"])
def test_two_distinct_samples_plan_on_the_sample_the_device_reports(bp, counts):
    """S = 2 with different samples: |q0 - m| and |q1 - m| are equal up to the rounding of the mean, so the sums differ by
    some 1e-16 relative and no summation order is 'the' choice.  The block and the records must be those of the sample
    fot_loop_last_best_sample reports, whichever it is."""
    rs = PredictionResampler(bp, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
    _begin(bp, len(counts))
    bp.loop_plan_sample(REP)
    F = Frame(rs, counts, 2, seed=4300 + sum(counts))
    _, g = F.host_blocks()
    assert (g < rc.GAP).all()                                        # (the premise: ties to rounding)
    _check_frame(bp, F, gap=False, device_choice=True)


# ---- 7. the prepend decided per episode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["standing", "moved_across_the_threshold"])
def test_prepend_is_decided_per_episode(bp, moved):
    rs = PredictionResampler(bp, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
    F = Frame(rs, (7, 5, 0, 3), 4, seed=77, stand=(1, 3), stale=0.0)
    lo = int(F.off[1])
    if moved:
        # one coordinate of one pedestrian of episode 1 just past atol + rtol |cur| from its first predicted sample
        a = F.pos[lo, 0]
        F.pos[lo, 0] = a + (rc.ATOL + rc.RTOL * abs(a)) * (1.0 + 1e-3)
        assert rc.prepend_rule([a], [F.pos[lo, 0]]) and not rc.prepend_rule([a], [a + (rc.ATOL + rc.RTOL * abs(a)) * (1.0 - 1e-3)])
    _begin(bp, F.n_ep)
    bp.loop_plan_sample(REP)
    rec, want = _check_frame(bp, F, gap=False)                       # (the standing crowds' samples are identical: sample 0)
    assert [pre for _, pre, _ in want] == [1, 1 if moved else 0, -1, 0]
    assert want[1][2] == 0 and want[3][2] == 0
    # batch independence: every episode alone in its frame leaves the same record
    for e in range(F.n_ep):
        _begin(bp, 1)
        bp.loop_plan_sample(REP)
        solo, _ = _check_frame(bp, F, episodes=[e], gap=False)
        _same_records(solo, rec[[e]])


# ---- 8. the resident sampler loop -------------------------------------------------------------------------------------------------------
S_LOOP, N_LOOP = rc.LOOP_SAMPLES, rc.LOOP_STEPS
assert SEED == rc.LOOP_SEED                      # (the seed test_rep_sample_cpu.py checks for near-ties)


def _loop_inputs():
    cfg, tracks = rc.loop_inputs()
    return cfg, tracks, case_weights(rc.LOOP_MODEL)


def _spy_best(sim):
    """The chosen samples of every lock step of the loop: loop_last_best_sample after each one-call step; of a resident
    loop the rows of loop_run_best_samples after each loop_run call, whose last row is loop_last_best_sample."""
    got = []
    name = "loop_run" if sim._resident else "loop_step"
    orig = getattr(sim.engine, name)

    def call(*a, **kw):
        o = orig(*a, **kw)
        last = sim.engine.loop_last_best_sample().copy()
        if sim._resident:
            rows = sim.engine.loop_run_best_samples(o["n_steps"])
            assert rows.shape == (o["n_steps"], len(last)) and (o["n_steps"] == 0 or (rows[-1] == last).all())
            got.extend(r.copy() for r in rows)
        else:
            got.append(last)
        return o
    setattr(sim.engine, name, call)
    return got


@pytest.fixture(scope="module")
def loop_runs():
    cfg, tracks, w = _loop_inputs()
    src = lambda: SganSampler(None, w, S_LOOP, counter_seed=SEED)
    kw = dict(device_samples=True, plan_on_representative_sample=True)
    out = {}
    res = BatchedClosedLoop(cfg, tracks, sample_source=src(), resident=True, **kw)
    stp = BatchedClosedLoop(cfg, tracks, sample_source=src(), **kw)
    host = BatchedClosedLoop(cfg, tracks, sample_source=src())
    with res, stp, host:
        assert res._resident and res._resident_sampler and not res.distribution_aware
        assert stp._native and stp._device_samples and not host._native
        s_res, s_stp = _spy_s_now(res), _spy_s_now(stp)
        b_res, b_stp = _spy_best(res), _spy_best(stp)
        chosen = []
        orig = host._best_sample

        def spy(dist, off):
            chosen.append((rc.host_choice(dist, np.asarray(off)), rc.gaps(dist, np.asarray(off))))
            return orig(dist, off)
        host._best_sample = spy
        res.run(5)                                                   # (two fot_loop_run calls of several steps each)
        h_res = [list(h) for h in res.run(N_LOOP - 5)]
        h_stp = [list(h) for h in stp.run(N_LOOP)]
        h_host = [list(h) for h in host.run(N_LOOP)]
        _assert_same_bytes(res, stp, s_res, s_stp, label="representative")
        out.update(h_res=h_res, h_stp=h_stp, h_host=h_host, b_res=b_res, b_stp=b_stp, chosen=chosen,
                   sels=[np.asarray(s["sel"]).copy() for s in stp._steps], bytes=_run_bytes(res), n=len(tracks))
    return out


def test_resident_loop_equals_the_stepwise_loop_and_the_host_route(loop_runs):
    r = loop_runs
    assert len(r["h_res"][2]) == N_LOOP                               # (byte equality of the two loops: in the fixture)
    _same_histories(r["h_host"], r["h_stp"])
    _same_histories(r["h_host"], r["h_res"])


def test_last_best_sample_equals_the_host_choice_at_every_step(loop_runs):
    r = loop_runs
    assert len(r["b_res"]) == len(r["b_stp"]) == len(r["chosen"]) == N_LOOP     # (the observer is full after the warm-up)
    seen = set()
    for k in range(N_LOOP):
        want = np.full(r["n"], -1)
        want[r["sels"][k]] = r["chosen"][k][0]
        assert (r["chosen"][k][1] > rc.GAP).all(), f"step {k}: a near-tie among the deviation sums: choose another seed"
        np.testing.assert_array_equal(r["b_stp"][k], want, err_msg=f"stepwise, step {k}")
        np.testing.assert_array_equal(r["b_res"][k], want, err_msg=f"resident, step {k}")
        seen |= set(int(v) for v in want if v >= 0)
    assert len(seen) >= 2


def test_scored_resident_loop_plans_and_scores_on_one_selection(loop_runs):
    cfg, tracks, w = _loop_inputs()
    kw = dict(device_samples=True, plan_on_representative_sample=True, prediction_scores=True)
    res = BatchedClosedLoop(cfg, tracks, sample_source=SganSampler(None, w, S_LOOP, counter_seed=SEED), resident=True, **kw)
    stp = BatchedClosedLoop(cfg, tracks, sample_source=SganSampler(None, w, S_LOOP, counter_seed=SEED), **kw)
    with res, stp:
        assert res._resident_scores
        b_res = _spy_best(res)
        res.run(N_LOOP)
        stp.run(N_LOOP)
        assert _run_bytes(res) == loop_runs["bytes"] == _run_bytes(stp)          # the scores leave the steps alone
        for a, b in zip(b_res, loop_runs["b_res"]):
            np.testing.assert_array_equal(a, b)
        got, want = res.prediction_metrics(), stp.prediction_metrics()
        for a, b in zip(got, want):
            assert tuple(a) == METRIC_KEYS == tuple(b)
            for k in METRIC_KEYS:
                assert type(a[k]) is type(b[k]) and _nan_equal(a[k], b[k]), (k, a[k], b[k])
        row = res.aggregate_metrics()
        for a, g in zip(row, got):
            for k in METRIC_KEYS:
                assert _nan_equal(a[k], g[k]), k


# ---- 9. off means off; the refusals ---------------------------------------------------------------------------------------------------
def _dist_loop(**kw):
    import torch
    ep = load_dist_episodes()
    var = ep["meta"]["variants"]["s4_eps0"]
    cfg = dict(var["config"])
    host_src = scripted_sample_source(var["n_samples"], cfg["pred_len"])
    dev = torch.device("cuda", 0)
    dev_src = lambda last, prev: torch.from_numpy(np.ascontiguousarray(host_src(last, prev), dtype=np.float64)).to(dev)
    return BatchedClosedLoop(cfg, [ep["s4_eps0_ped_traj"]] * 2, sample_source=dev_src, device_samples=True, **kw)


def _cv_loop(**kw):
    ep = load_episodes()
    return BatchedClosedLoop(scenario_config(ep["meta"]), [ep["base_ped_traj"], ep["shift_ped_traj"]], **kw)


def _step_bytes(sim):
    keys = ("sel", "ego", "jerk", "state", "stats", "keep", "cost", "after", "has_path")
    out = [tuple(np.ascontiguousarray(s[k]).tobytes() for k in keys) for s in sim._steps]
    paths = [tuple(s["paths"][f].tobytes() for f in _abi.PATH_FIELDS) for s in sim._steps]
    return out, paths, sim.ego.tobytes()


@pytest.mark.parametrize("make,kw", [(_dist_loop, {}), (_cv_loop, {}), (_cv_loop, dict(resident=True))],
                         ids=["distribution_aware", "constant_velocity", "constant_velocity_resident"])
def test_mode_zero_is_the_loop_as_it_was(make, kw):
    runs = []
    for call in (False, True):
        with make(**kw) as sim:
            if call:
                sim.engine.loop_plan_sample(_abi.LOOP_PLAN_DISTRIBUTION)
            sim.run(15)
            runs.append(_step_bytes(sim))
    assert runs[0] == runs[1]


def test_refusals_change_nothing(bp):
    lib = _abi.lib()

    def refused(h, code, mode):
        assert lib.fot_loop_plan_sample(h, mode) == code, mode
        assert b"fot_loop_plan_sample" in lib.fot_last_error(h)

    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as fresh:
        refused(fresh._h, _abi.ERR_INVALID, REP)                     # no loop has begun
        refused(fresh._h, _abi.ERR_INVALID, 0)
    with _dist_loop() as sim:
        sim.run(10)
        want = _step_bytes(sim)
    with _dist_loop() as sim:
        for mode in (2, -1):
            refused(sim.engine._h, _abi.ERR_INVALID, mode)           # unknown modes
        with pytest.raises(_abi.FotError, match="scores are not enabled"):
            sim.engine.loop_last_best_sample()                       # (the mode is still off)
        assert lib.fot_loop_run_best_samples(sim.engine._h, 0, 2, None) == _abi.ERR_INVALID      # (no resident run)
        sim.run(10)
        assert _step_bytes(sim) == want
    with _cv_loop(resident=True) as sim:
        sim.run(6)
        want = _step_bytes(sim)
    with _cv_loop(resident=True) as sim:
        sim.run(3)
        refused(sim.engine._h, _abi.ERR_INVALID, REP)                # after a resident run's first step
        refused(sim.engine._h, _abi.ERR_INVALID, 0)
        assert lib.fot_loop_run_best_samples(sim.engine._h, 3, 2, None) == _abi.ERR_INVALID      # (the mode is off)
        sim.run(3)
        assert _step_bytes(sim) == want
    meta = load_episodes()["meta"]
    import loop_crowds_common as lc
    cfgs = [scenario_config(meta, "base"), scenario_config(meta, "turn")]
    two = lc.crowd_tracks((2, 3), 40, lc.TRACK_SEED)
    with BatchedClosedLoop(cfgs, two) as sim:
        sim.run(4)
        want = _step_bytes(sim)
    with BatchedClosedLoop(cfgs, two) as sim:
        assert sim.scenarios is not None
        refused(sim.engine._h, _abi.ERR_UNSUPPORTED, REP)            # a loop begun with fot_loop_begin_scenarios
        sim.run(4)
        assert _step_bytes(sim) == want
    # fot_loop_begin resets the mode: the handle plans against the whole distribution again
    _begin(bp, 1)
    bp.loop_plan_sample(REP)
    _begin(bp, 1)
    rs = PredictionResampler(bp, pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
    F = Frame(rs, (5,), 3, seed=5)
    frame, eps = F.frame()
    bp.loop_plan(_requests(bp, F.egos[eps], [0]), frame)
    blk, pre = bp.debug_loop_block(0, samples=3)
    assert blk.shape == (3, 5, rs.n_dense + 1, 2) and pre == -1
    with pytest.raises(_abi.FotError, match="scores are not enabled"):
        bp.loop_last_best_sample()


def test_python_refusals():
    ep = load_dist_episodes()
    cfg = dict(ep["meta"]["variants"]["s4_eps0"]["config"])
    src = scripted_sample_source(4, cfg["pred_len"])
    with pytest.raises(ValueError, match="plan_on_representative_sample.*distribution_aware_planning"):
        BatchedClosedLoop(cfg, [ep["s4_eps0_ped_traj"]], sample_source=src, device_samples=True,
                          plan_on_representative_sample=True)
