"""Crowds around the wave and workgroup width for the closed-loop kernels, the part that needs no GPU: the builders'
preconditions (tests/loop_crowds_common.py), and the resident crowds' slots run stepwise on the oracle-backed stand-ins
-- every slot of 64 and more pedestrians runs long enough for standard prediction-error origins to complete, and the
slots of 33, 64, 65 and 257 reproduce the reference simulator's own runs
(tests/golden/closed_loop/reference_crowd_episodes.npz)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import loop_crowds_common as lc
from closed_loop_common import OracleEngine, OracleResampler, assert_episode_matches, load_episodes, scenario_config
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from summary_common import assert_summary_matches_reference, reference_summary, summary_of_history


@pytest.fixture(scope="module")
def cfg():
    return scenario_config(load_episodes()["meta"])


@pytest.fixture(scope="module")
def n_dense(cfg):
    rp = _abi.ResampleParams(0.4, float(cfg["dt"]), float(cfg["max_t"]))
    return int(_abi.lib().fot_resample_n_dense(C.byref(rp), int(cfg["pred_len"])))


def test_matter_count_keeps_to_the_last_run_of_64():
    assert [lc.matter_count(p) for p in (0, 1, 2, 3, 5, 63, 64, 65, 66, 128, 129, 130, 257, 300)] == \
        [0, 1, 2, 3, 3, 3, 3, 1, 2, 3, 1, 2, 1, 3]


@pytest.mark.parametrize("counts, seed", list(lc.FRAME_CASES.values()) + list(lc.GROWTH_FRAMES)
                         + [(c, s) for _, c, s in lc.DIST_CASES.values()])
def test_frame_preconditions(counts, seed):
    fr = lc.crowd_frame(counts, seed)
    assert fr["ped_off"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert fr["obs_last"].dtype == np.float32 and fr["obs_prev"].dtype == np.float32
    lc.assert_frame_preconditions(fr)
    again = lc.crowd_frame(counts, seed)
    assert all(np.array_equal(fr[k], again[k]) for k in ("ped_pos", "ped_vel", "obs_last", "obs_prev", "egos"))
    # the check itself notices a crowd whose nearest pedestrian is not the last one
    if max(counts) >= 2:
        e = int(np.argmax(counts))
        bad = dict(fr, ped_pos=fr["ped_pos"].copy())
        bad["ped_pos"][fr["ped_off"][e]] = fr["egos"][e, :2] + 1.0
        with pytest.raises(AssertionError):
            lc.assert_frame_preconditions(bad)


def test_track_preconditions(n_dense):
    tracks = lc.slot_tracks()
    assert [t.shape for t in tracks] == [(f, p, 2) for p, f in zip(lc.SLOT_COUNTS, lc.SLOT_FRAMES)]
    assert all(np.array_equal(a, b) for a, b in zip(tracks, lc.slot_tracks()))
    lc.assert_track_preconditions(tracks, n_dense + lc.EXTRA_STEPS, n_dense)
    # every decoy's constant-velocity error differs: amplitude and phase grow with the index
    tr = tracks[lc.SLOT_COUNTS.index(257)]
    per = [lc.rolling_mean_displacement(tr, n_dense + lc.EXTRA_STEPS, n_dense, keep=[j]) for j in (0, 63, 64, 128, 254)]
    assert min(per) > 1e-2 and len({round(v, 6) for v in per}) == len(per), per
    # the short recordings end inside the run: their last frame is held
    warm = 8 * 4
    assert all(f < warm + n_dense + lc.EXTRA_STEPS for p, f in zip(lc.SLOT_COUNTS, lc.SLOT_FRAMES) if p in (33, 129))


@pytest.fixture(scope="module")
def oracle_run(cfg, n_dense):
    """All slots stepwise on the oracle-backed stand-ins, n_dense + 15 lock steps."""
    sim = BatchedClosedLoop(cfg, lc.slot_tracks(), engine=OracleEngine(cfg), resampler=OracleResampler(cfg))
    hists = [list(h) for h in sim.run(n_dense + lc.EXTRA_STEPS)]
    return hists, [ep.termination_reason for ep in sim.episodes]


def _kw(cfg):
    return dict(dt=cfg["dt"], sgan_dt=0.4, pred_len=cfg["pred_len"], num_samples=cfg.get("num_samples", 1))


def test_large_slots_run_long_enough_for_standard_origins(cfg, n_dense, oracle_run):
    """Precondition (f) of the GPU test for the chosen seed: every slot of 64 and more pedestrians runs n_dense + 5 steps
    or more and counts standard origins; the planner reacts to the crossing pedestrian in some of them."""
    hists, _ = oracle_run
    reacted = 0
    for P, h in zip(lc.SLOT_COUNTS, hists):
        if P >= 64:
            assert len(h) >= n_dense + 5, f"P = {P}: {len(h)} steps"
            assert summary_of_history(h, **_kw(cfg))["ade_eval_count"] > 0, P
        reacted += any(r.metrics.get("n_collision_rejected", 0) > 0 for r in h)
    assert reacted >= 6


def test_restated_rolling_displacement_agrees_with_the_loop(cfg, n_dense, oracle_run):
    """The precondition's NumPy restatement against summary_of_history of the oracle loop's history.  The loop rounds the
    observer's samples to float32 (half an ulp of 2^-17 at 64 .. 128 m = 3.8e-6 m per coordinate), the restatement does
    not: a predicted point moves by at most 3.8e-6 (1 + 2 t / sgan_dt) <= 1.05e-4 m per coordinate at t <= 5.3 s, a
    mean of distances is 1-Lipschitz in every point: atol sqrt(2) x 1.05e-4."""
    hists, _ = oracle_run
    for P, h, tr in zip(lc.SLOT_COUNTS, hists, lc.slot_tracks()):
        if P == 0:
            continue
        want = summary_of_history(h, **_kw(cfg))["planning_ade"]
        got = lc.rolling_mean_displacement(tr, len(h), n_dense)
        assert abs(got - want) <= math.sqrt(2.0) * 1.05e-4, (P, got, want)


def test_fixture_holds_what_the_tests_need(n_dense):
    fix = lc.load_crowd_episodes()
    meta = fix["meta"]
    assert set(meta["variants"]) == {f"p{p}" for p in lc.REFERENCE_SLOTS} and meta["track_seed"] == lc.TRACK_SEED
    assert meta["steps"] == n_dense + lc.EXTRA_STEPS
    assert tuple(meta["keys"]) == BatchedClosedLoop.SUMMARY_KEYS and tuple(meta["int_keys"]) == BatchedClosedLoop.SUMMARY_INT_KEYS
    for p in lc.REFERENCE_SLOTS:
        v = meta["variants"][f"p{p}"]
        assert v["n_peds"] == p and v["n_frames"] == lc.SLOT_FRAMES[lc.SLOT_COUNTS.index(p)]
        assert not any(k.endswith("ped_traj") for k in fix)         # the recordings are rebuilt from the seed
        s = reference_summary(fix, f"p{p}")
        assert s["planning_eval_count"] > 0 and s["planning_ade"] > 1e-2
        assert v["steps"] == meta["steps"] and s["ade_eval_count"] > 0 and s["ade"] > 1e-2
    path = os.path.join(ROOT, "tests", "golden", "closed_loop", "reference_crowd_episodes.npz")
    assert os.path.getsize(path) < (1 << 20)


@pytest.mark.parametrize("P", lc.REFERENCE_SLOTS)
def test_oracle_loop_matches_the_reference_simulator(cfg, oracle_run, P):
    """The slot in the oracle loop (beside ten others) against the reference simulator's own run of its recording: every
    step, and the summary restated over the loop's history against calculate_aggregate_metrics."""
    fix = lc.load_crowd_episodes()
    hists, term = oracle_run
    e = lc.SLOT_COUNTS.index(P)
    name = f"p{P}"
    assert fix["meta"]["variants"][name]["steps"] == len(hists[e])
    assert_episode_matches(hists[e], term[e], fix, name)
    assert_summary_matches_reference(summary_of_history(hists[e], **_kw(cfg)), reference_summary(fix, name), name)
