"""Episode summary metrics accumulated on the device by the resident loop (fot_loop_summary_enable / fot_loop_summaries,
BatchedClosedLoop(resident=True, summaries=True).aggregate_metrics()): against the reference's
calculate_aggregate_metrics of its own runs (tests/golden/closed_loop/reference_summary_episodes.npz: the thirteen
straight-line variants and five whose pedestrians weave), against the NumPy restatement over the loop's own history, in
chunks, twice, mixed against separate handles, and the C ABI with its refusals.  Tolerances: tests/summary_common.py."""
import copy
import ctypes as C

import numpy as np
import pytest

from closed_loop_common import load_episodes, scenario_config
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop, merge_configs
from summary_common import (assert_summary_matches_own_history, assert_summary_matches_reference, load_summaries,
                            reference_summary, summary_of_history)

pytestmark = pytest.mark.gpu

# interleaved: neighbouring slots are on different scenarios (test_gpu_loop_scenarios.py's order, the weave variants between)
NAMES = ("base", "walls", "weave2", "turn", "footprint", "weave0", "inflate", "fast", "rnd3", "weave1", "rnd2", "shift",
         "weave_short", "rnd4", "rnd0", "weave3", "rnd1", "rnd5")
WEAVE = ("weave0", "weave1", "weave2", "weave3", "weave_short")


@pytest.fixture(scope="module")
def data():
    return load_episodes(), load_summaries()


def _cfg(data, name):
    episodes, fix = data
    return dict(fix["meta"]["variants"][name]["config"]) if name in WEAVE else scenario_config(episodes["meta"], name)


def _tracks(data, name):
    episodes, fix = data
    return fix[name + "_ped_traj"] if name in WEAVE else episodes[name + "_ped_traj"]


def _build(data, names, **kw):
    kw.setdefault("resident", True)
    kw.setdefault("summaries", True)
    return BatchedClosedLoop([_cfg(data, n) for n in names], [_tracks(data, n) for n in names], **kw)


def _step_outputs(sim):
    """Every per-step output of fot_loop_run the loop keeps, per episode, as bytes."""
    out = [[] for _ in sim.episodes]
    for s in sim._steps:
        for e in range(len(sim.episodes)):
            i = int(s["slot"][e])
            if i < 0:
                continue
            kn = int(s["keep"][i])
            out[e].append(b"".join([np.array(s["ego"][i]).tobytes(), np.array(s["jerk"][i]).tobytes(),
                                    np.array(s["state"][i]).tobytes(), np.array(s["stats"][i]).tobytes(),
                                    np.array(s["keep"][i]).tobytes(), np.array(s["has_path"][i]).tobytes(),
                                    np.array(s["after"][i]).tobytes()]
                                   + [np.array(s["paths"][f][i, :kn]).tobytes() for f in _abi.PATH_FIELDS]))
    return out


def _summary_kw(data, name):
    _, fix = data
    v = fix["meta"]["variants"][name]
    c = _cfg(data, name)
    return dict(dt=c["dt"], sgan_dt=v["sgan_dt"], pred_len=v["pred_len"], num_samples=c.get("num_samples", 1))


@pytest.fixture(scope="module")
def mixed(data):
    """All eighteen episodes on ONE handle (five scenarios), paths kept: the summaries, their raw records, the restatement
    over the loop's own history and the per-step outputs."""
    lib = _abi.lib()
    before = lib.fot_live_handles()
    with _build(data, NAMES) as sim:
        handles, scenarios = lib.fot_live_handles() - before, sim.engine.n_scenarios
        hists = sim.run()
        raw = sim.engine.loop_summaries().copy()
        agg = sim.aggregate_metrics()
        own = [summary_of_history(list(h), **_summary_kw(data, n)) for h, n in zip(hists, NAMES)]
        per_step = _step_outputs(sim)
        # extrema and counts over the loop's own per-step outputs (jerk, ego[..., 4], after), as fot_loop_run wrote them
        direct = []
        for e in range(len(NAMES)):
            rows = [(s, int(s["slot"][e])) for s in sim._steps if int(s["slot"][e]) >= 0]
            jerk = np.array([abs(float(s["jerk"][i])) for s, i in rows])
            acc = np.array([abs(float(s["ego"][i][4])) for s, i in rows])
            after = [s["after"][i] for s, i in rows]
            ttc = [float(a["ttc"]) for a in after if 0 < float(a["ttc"]) < float("inf")]
            direct.append(dict(steps=len(rows), max_jerk=float(jerk.max()), max_accel=float(acc.max()),
                               min_dist=min(float(a["min_distance"]) for a in after),
                               collision_count=sum(int(a["collision"]) != 0 for a in after),
                               min_ttc=min(ttc) if ttc else float("inf")))
        term = [ep.termination_reason for ep in sim.episodes]
    return dict(agg=agg, raw=raw, own=own, per_step=per_step, direct=direct, term=term, handles=handles, scenarios=scenarios)


@pytest.fixture(scope="module")
def separate(data):
    """The same episodes on five single-configuration handles of their own, paths not kept."""
    _, slot, _ = merge_configs([_cfg(data, n) for n in NAMES])
    agg, raw = [None] * len(NAMES), [None] * len(NAMES)
    for k in range(int(slot.max()) + 1):
        members = [i for i in range(len(NAMES)) if slot[i] == k]
        names = [NAMES[i] for i in members]
        with BatchedClosedLoop(_cfg(data, names[0]), [_tracks(data, n) for n in names], resident=True, summaries=True) as alone:
            assert alone.scenarios is None
            alone.run(keep_paths=False)
            a, r = alone.aggregate_metrics(), alone.engine.loop_summaries().copy()
        for j, i in enumerate(members):
            agg[i], raw[i] = a[j], r[j:j + 1]
    return dict(agg=agg, raw=raw)


# ---- 1. against the reference ---------------------------------------------------------------------------------------------
def test_mixed_handle_matches_the_reference(data, mixed):
    _, fix = data
    assert mixed["handles"] == 1 and mixed["scenarios"] == 5
    for name, got, term in zip(NAMES, mixed["agg"], mixed["term"]):
        v = fix["meta"]["variants"][name]
        assert (got["steps"], got["termination_reason"], term) == (v["steps"], v["termination"], v["termination"]), name
        assert abs(got["total_time"] - v["steps"] * 0.1) < 1e-9 and got["collision"] == (v["termination"] == "collision")
        assert_summary_matches_reference(got, reference_summary(fix, name), f"{name} (mixed)")


def test_single_scenario_handles_match_the_reference(data, separate):
    _, fix = data
    for name, got in zip(NAMES, separate["agg"]):
        v = fix["meta"]["variants"][name]
        assert (got["steps"], got["termination_reason"]) == (v["steps"], v["termination"]), name
        assert_summary_matches_reference(got, reference_summary(fix, name), f"{name} (alone)")


def test_value_types_are_the_reference_s(mixed):
    for got in mixed["agg"]:
        for k in BatchedClosedLoop.SUMMARY_KEYS:
            assert type(got[k]) is (int if k in BatchedClosedLoop.SUMMARY_INT_KEYS else float), k
        assert np.isnan(got["nll"]) and got["nll_eval_count"] == 0
        assert type(got["steps"]) is int and type(got["collision"]) is bool


# ---- 2. against the restatement over the loop's own history ---------------------------------------------------------------
def test_device_summary_equals_the_restatement_on_own_history(mixed):
    for name, got, own, direct in zip(NAMES, mixed["agg"], mixed["own"], mixed["direct"]):
        assert_summary_matches_own_history(got, own, name)
        for k, v in direct.items():                                # equal to min / max / count over fot_loop_run's outputs
            assert got[k] == v, f"{name} {k}: {got[k]!r}, per-step outputs give {v!r}"


# ---- 3. chunks, repeats, neighbours, and the loop itself ------------------------------------------------------------------
def test_summaries_between_runs_and_byte_identity(data, mixed, separate):
    _, fix = data
    names = ("base", "weave0", "fast")
    with _build(data, names) as sim:
        sim.run(60)
        at60 = sim.aggregate_metrics()
        sim.run(40)
        at100 = sim.aggregate_metrics()
        again100 = sim.engine.loop_summaries().tobytes()
        assert again100 == sim.engine.loop_summaries().tobytes()   # (a summary changes nothing)
        sim.run()
        final = sim.engine.loop_summaries().copy()
        final_agg = sim.aggregate_metrics()
        chunked_steps = _step_outputs(sim)
    assert at60[0]["steps"] == 60 and at100[0]["steps"] == 100
    assert_summary_matches_reference(at60[0], reference_summary(fix, "base", 60), "base after 60 steps")
    assert_summary_matches_reference(at100[0], reference_summary(fix, "base", 100), "base after 100 steps")
    assert at100[2]["steps"] == fix["meta"]["variants"]["fast"]["steps"]          # (ended before step 60; its summary stands)
    assert_summary_matches_reference(at100[2], reference_summary(fix, "fast"), "fast, asked again later")
    for j, n in enumerate(names):
        i = NAMES.index(n)
        assert_summary_matches_reference(final_agg[j], reference_summary(fix, n), f"{n} (chunked)")
        # chunked == unchunked, on another handle, beside other neighbours, on one scenario or five: the same bytes
        assert final[j:j + 1].tobytes() == mixed["raw"][i:i + 1].tobytes(), f"{n}: chunked against the unchunked mixed run"
        assert final[j:j + 1].tobytes() == separate["raw"][i].tobytes(), f"{n}: against a handle of its own scenario"
        assert chunked_steps[j] == mixed["per_step"][i], f"{n}: per-step outputs"


def test_mixed_handle_equals_separate_handles_byte_for_byte(mixed, separate):
    for i, n in enumerate(NAMES):
        assert mixed["raw"][i:i + 1].tobytes() == separate["raw"][i].tobytes(), n


def test_two_runs_are_byte_identical_and_summaries_leave_the_loop_alone(data, mixed):
    """A second mixed run gives the same records; a run WITHOUT summaries gives the same per-step outputs of fot_loop_run
    (ego, jerk, state, stats, keep, after, the followed paths) byte for byte."""
    with _build(data, NAMES) as sim:
        sim.run(keep_paths=False)
        assert sim.engine.loop_summaries().tobytes() == mixed["raw"].tobytes()
    with _build(data, NAMES, summaries=False) as plain:
        plain.run()
        per = _step_outputs(plain)
        with pytest.raises(ValueError, match="summaries=True"):
            plain.aggregate_metrics()
    for i, n in enumerate(NAMES):
        assert per[i] == mixed["per_step"][i], f"{n}: per-step outputs with and without summaries"


def test_keep_paths_false_never_fills_a_step_record(data, tmp_path):
    """run(keep_paths=False) + aggregate_metrics() + save_summaries(): no step record is materialised (no per-step
    fot_predict_cv, no history read)."""
    from integrated_path_planning_amd import closed_loop as cl
    _, fix = data

    def boom(self):
        raise AssertionError("_ResidentStep._fill was called")

    with _build(data, ("base", "weave1")) as sim:
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(cl._ResidentStep, "_fill", boom)
            sim.run(keep_paths=False)
            agg = sim.aggregate_metrics()
            sim.save_summaries(str(tmp_path))
    assert [a["steps"] for a in agg] == [fix["meta"]["variants"][n]["steps"] for n in ("base", "weave1")]


def test_save_summaries_writes_one_row_per_episode(data, tmp_path):
    import csv
    with _build(data, ("fast", "weave3")) as sim:
        sim.run(keep_paths=False)
        agg = sim.aggregate_metrics()
        f = sim.save_summaries(str(tmp_path))
        files = sim.save_results(str(tmp_path))
    assert f.endswith("metrics_summary.csv") and len(files) == 2 and all(p.endswith("trajectory.npz") for p in files)
    rows = list(csv.DictReader(open(f)))
    assert len(rows) == 2
    for k in BatchedClosedLoop.SUMMARY_KEYS + ("termination_reason", "steps", "total_time", "collision"):
        assert k in rows[0], k
    assert not any(k.endswith("_time") and k != "total_time" for k in rows[0])
    for row, a in zip(rows, agg):
        assert int(row["steps"]) == a["steps"] and row["termination_reason"] == a["termination_reason"]
        assert int(row["planning_eval_count"]) == a["planning_eval_count"]
        assert float(row["planning_ade"]) == a["planning_ade"]
    assert rows[0]["ade"] == "nan" and int(rows[0]["ade_eval_count"]) == 0


# ---- 4. nothing to evaluate -------------------------------------------------------------------------------------------------
def test_a_slot_without_pedestrians_and_a_slot_that_stops_early(data):
    """No pedestrians: no prediction, nothing counted (NaN / 0, min_dist and min_ttc infinite), as the reference's empty
    sums; `fast` collides at step 41, before any standard origin has a complete horizon (ade NaN, count 0) while the
    rolling metric has counted."""
    _, fix = data
    cfg = _cfg(data, "base")
    with BatchedClosedLoop(cfg, [np.zeros((400, 0, 2)), _tracks(data, "fast"), _tracks(data, "base")[:, :1]], resident=True,
                           summaries=True) as sim:
        hists = sim.run()
        agg = sim.aggregate_metrics()
        own = [summary_of_history(list(h), **_summary_kw(data, "base")) for h in hists]
    empty, fast, one = agg
    assert empty["steps"] > 0
    for k in ("ade", "fde", "ade_per_agent", "fde_per_agent", "planning_ade", "planning_fde", "nll"):
        assert np.isnan(empty[k]), k
    for k in ("ade_eval_count", "planning_eval_count", "pred_samples", "nll_eval_count", "collision_count"):
        assert empty[k] == 0, k
    assert empty["min_dist"] == float("inf") and empty["min_ttc"] == float("inf")
    assert_summary_matches_reference(fast, reference_summary(fix, "fast"), "fast")
    assert np.isnan(fast["ade"]) and fast["ade_eval_count"] == 0 and fast["pred_samples"] == 0
    assert fast["planning_eval_count"] == 560 and fast["steps"] == 41
    assert one["ade_eval_count"] > 0 and one["pred_samples"] == cfg.get("num_samples", 1)
    for got, o, label in zip(agg, own, ("no pedestrians", "fast", "one pedestrian")):
        assert_summary_matches_own_history(got, o, label)


# ---- 5. the C ABI alone ------------------------------------------------------------------------------------------------------
def _raw_summaries(lib, h, n, n_alloc=None):
    out = np.zeros(max(n_alloc or n, 1), dtype=np.dtype(_abi.LoopSummary))
    out["steps"] = -7                                              # (a refused call must not write)
    return lib.fot_loop_summaries(h, n, out.ctypes.data), out


@pytest.mark.parametrize("names", [("base", "fast"), ("weave1", "base", "turn")], ids=["loop_begin", "loop_begin_scenarios"])
def test_c_abi_summaries_and_refusals(data, names):
    """fot_loop_summary_enable / fot_loop_summaries through ctypes on a handle begun with fot_loop_begin and with
    fot_loop_begin_scenarios: every refusal returns FOT_ERR_INVALID with a message and changes nothing -- the run goes
    on and ends with the reference's numbers."""
    _, fix = data
    lib = _abi.lib()
    n = len(names)
    with _build(data, names, summaries=False) as sim:
        assert (sim.scenarios is not None) == (len(names) == 3)
        bp = sim.engine
        h = bp._h
        # not enabled
        rc, out = _raw_summaries(lib, h, n)
        assert rc == _abi.ERR_INVALID and (out["steps"] == -7).all() and b"not enabled" in lib.fot_last_error(h)
        assert lib.fot_loop_summary_enable(h, 1, 0) == _abi.ERR_INVALID              # num_samples < 1
        rc, _ = _raw_summaries(lib, h, n)
        assert rc == _abi.ERR_INVALID                                                # (the refused enable changed nothing)
        assert lib.fot_loop_summary_enable(h, 1, 20) == _abi.OK
        assert lib.fot_loop_summary_enable(h, 0, 20) == _abi.OK                      # off again ...
        assert _raw_summaries(lib, h, n)[0] == _abi.ERR_INVALID
        assert lib.fot_loop_summary_enable(h, 1, 20) == _abi.OK                      # ... and on
        # a wrong slot count, a NULL record array
        for bad in (n - 1, n + 1):
            rc, out = _raw_summaries(lib, h, bad, n + 1)
            assert rc == _abi.ERR_INVALID and (out["steps"] == -7).all() and b"n_slots" in lib.fot_last_error(h)
        assert lib.fot_loop_summaries(h, n, None) == _abi.ERR_INVALID
        # before the first step: the reference's values of an empty history
        rc, out = _raw_summaries(lib, h, n)
        assert rc == _abi.OK and (out["steps"] == 0).all() and (out["min_dist"] == 0.0).all() and np.isinf(out["min_ttc"]).all()
        assert np.isnan(out["ade"]).all() and np.isnan(out["planning_ade"]).all() and (out["termination"] == 0).all()
        bp.loop_run(30, keep_paths=False)
        # after the first step the switch is refused, either way, and the accumulation goes on
        assert lib.fot_loop_summary_enable(h, 1, 20) == _abi.ERR_INVALID and b"begun" in lib.fot_last_error(h)
        assert lib.fot_loop_summary_enable(h, 0, 20) == _abi.ERR_INVALID
        rc, mid = _raw_summaries(lib, h, n)
        assert rc == _abi.OK and (mid["steps"] == 30).all() and (mid["planning_eval_count"] > 0).all()
        while bp.loop_run(64, keep_paths=False)["n_steps"]:
            pass
        rc, out = _raw_summaries(lib, h, n)
        assert rc == _abi.OK
        for e, name in enumerate(names):
            got = {k: (int(out[k][e]) if k in BatchedClosedLoop.SUMMARY_INT_KEYS else float(out[k][e]))
                   for k in BatchedClosedLoop.SUMMARY_KEYS}
            assert_summary_matches_reference(got, reference_summary(fix, name), f"{name} (C ABI)")
            v = fix["meta"]["variants"][name]
            assert int(out["steps"][e]) == v["steps"] and int(out["termination"][e]) == {"collision": 1, "goal": 2}[v["termination"]]
            assert abs(float(out["total_time"][e]) - v["steps"] * 0.1) < 1e-9 and int(out["_pad"][e]) == 0
        # a predictor step that is no multiple of the simulation step: refused (metrics.py:22-28), the handle stays usable
        rp = copy.copy(sim.resampler.params)
        rp.sgan_dt = 0.45
        cfg0 = sim.config
        replay = dict(obs_len=cfg0.obs_len, pred_len=sim.resampler.pred_len, warmup_frames=32, ego_radius=sim.ego_radius,
                      ped_radius=sim.ped_radius, use_footprint=False, s_end=float(np.ravel(sim.s_end)[0]))
        bp.loop_set_replay(sim.ped_off, sim.n_frames, sim._ped_all["trajectories"], sim._ped_all["velocities"], rp=rp, **replay)
        assert _raw_summaries(lib, h, n)[0] == _abi.ERR_INVALID                      # (a new recording: off until enabled)
        assert lib.fot_loop_summary_enable(h, 1, 20) == _abi.ERR_INVALID and b"multiple" in lib.fot_last_error(h)
        assert _raw_summaries(lib, h, n)[0] == _abi.ERR_INVALID
        bp.loop_set_replay(sim.ped_off, sim.n_frames, sim._ped_all["trajectories"], sim._ped_all["velocities"],
                           rp=sim.resampler.params, **replay)
        assert lib.fot_loop_summary_enable(h, 1, 20) == _abi.OK
        # fot_loop_begin* drops the replay and the accumulators with it
        if sim.scenarios is None:
            from integrated_path_planning_amd.closed_loop import _VectorStateMachine, loop_config_from
            bp.loop_begin(loop_config_from(cfg0, _VectorStateMachine.constants_of(cfg0), 3), sim.ego)
            assert lib.fot_loop_summary_enable(h, 1, 20) == _abi.ERR_INVALID and b"fot_loop_set_replay" in lib.fot_last_error(h)
            rc, out = _raw_summaries(lib, h, n)
            assert rc == _abi.ERR_INVALID and (out["steps"] == -7).all()
