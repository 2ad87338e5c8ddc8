"""Encounter fidelity on the GPU: fot_fidelity_eval against the NumPy restatement (tests/fidelity_common.py, itself pinned to
the reference's answers by tests/test_fidelity_common.py) on identical inputs, at the shapes where the kernels can go wrong;
its byte-identical invariances; the exact thresholds; NaN coordinates; the cross-check with fot_footprint_recheck; its
refusals.

Decisions (onset steps, counts, closest_step) are equal, except for pedestrians inside the band 1e-9 (relative) around
accel_threshold or max_distance at some step up to their onset: only the two-term sum and the square root could differ
between device and host there.  At most 1 % of a test's pedestrians may be left out so; the inputs are chosen so that none
are.  Values are expected to be the same bits and are held to 2 ulp; the largest difference seen goes to the file that
FOT_FIDELITY_PROFILE names, from where scripts/fidelity_bench.py takes it into profiles/r28_fidelity.json (a test run by
itself leaves the committed profile alone)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fidelity_common as fc
from integrated_path_planning_amd import _abi, batch, fidelity, safety, synthetic as syn
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
WORST = {"ulp": 0.0, "pedestrians": 0, "left_out": 0, "onsets": 0}


@pytest.fixture(scope="module")
def engine():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        yield bp


@pytest.fixture(scope="module", autouse=True)
def note_worst():
    yield
    path = os.environ.get("FOT_FIDELITY_PROFILE")
    if path:
        with open(path, "w") as f:
            json.dump({"largest_value_difference_ulp": WORST["ulp"], "pedestrians_compared": WORST["pedestrians"],
                       "pedestrians_left_out_in_band": WORST["left_out"], "onsets": WORST["onsets"]}, f)


def poisoned(n, dtype):
    return np.frombuffer(bytearray([SENTINEL]) * (np.dtype(dtype).itemsize * max(n, 1)), dtype).copy()


def call(engine, encs, with_vel=False, truth=None, accel_threshold=0.3, max_distance=5.0, interaction_distance=None,
         null=(), **override):
    """fot_fidelity_eval through ctypes with every output pre-filled: (rc, records, series, onset_dist, onset_step,
    untouched)."""
    p = batch.PackedEncounters([e["ego_xy"] for e in encs], [e["ped_xy"] for e in encs], [e["dt"] for e in encs],
                               ped_vel=[e["ped_vel"] for e in encs] if with_vel else None, truth_xy=truth)
    n = override.get("n_enc", p.n)
    step_off = np.ascontiguousarray(override.get("step_off", p.step_off), np.int32)
    n_ped = np.ascontiguousarray(override.get("n_ped", p.n_ped if p.n else [0]), np.int32)
    dt = np.ascontiguousarray(override.get("dt", p.dt if p.n else [1.0]), np.float64)
    steps, peds = int(p.step_off[-1]), int(p.ped_base[-1])
    par = _abi.FidelityParams(accel_threshold, max_distance, np.nan if interaction_distance is None else interaction_distance)
    rec, series = poisoned(p.n, fc.ENC_DT), poisoned(steps, np.float64)
    dist, step = poisoned(peds, np.float64), poisoned(peds, np.int32)
    ptr = lambda a, name: None if (a is None or name in null) else a.ctypes.data
    rc = _abi.lib().fot_fidelity_eval(engine._h, None if "p" in null else C.byref(par), n, ptr(step_off, "step_off"),
                                      ptr(n_ped, "n_ped"), ptr(dt, "dt"), ptr(p.ego, "ego_xy"), ptr(p.ped, "ped_xy"),
                                      ptr(p.vel, "ped_vel"), ptr(p.truth, "truth_xy"), ptr(series, "sep_series"),
                                      ptr(dist, "onset_dist"), ptr(step, "onset_step"), ptr(rec, "out"))
    untouched = all(np.all(a.view(np.uint8) == SENTINEL) for a in (rec, series, dist, step))
    return rc, rec[:p.n], series[:steps], dist[:peds], step[:peds], untouched


def good(engine, encs, **kw):
    rc, rec, series, dist, step, _ = call(engine, encs, **kw)
    assert rc == _abi.OK, _abi.lib().fot_last_error(engine._h)
    return rec, series, dist, step


def compare(got, want, label):
    """decisions equal outside the band, values within ULPS; returns nothing, notes the worst"""
    rec, series, dist, step = got
    w_rec, w_series, w_dist, w_step, band = want
    assert len(band) == len(step)
    assert band.sum() <= 0.01 * max(len(band), 1), f"{label}: {int(band.sum())} of {len(band)} pedestrians inside the band"
    ok = ~band
    assert np.array_equal(step[ok], w_step[ok]), f"{label}: onset steps"
    worst = max(fc.ulp_diff(series, w_series), fc.ulp_diff(dist[ok], w_dist[ok]), fc.ulp_diff(rec["closest"], w_rec["closest"]))
    assert np.array_equal(rec["closest_step"], w_rec["closest_step"]), f"{label}: closest_step"
    assert np.array_equal(rec["err_count"], w_rec["err_count"]), f"{label}: err_count"
    if not band.any():
        assert np.array_equal(rec["n_onset"], w_rec["n_onset"]), f"{label}: n_onset"
    worst = max(worst, fc.ulp_diff(rec["err_sum"], w_rec["err_sum"]))
    assert worst <= fc.ULPS, f"{label}: {worst} ulp"
    WORST["ulp"] = max(WORST["ulp"], worst)
    WORST["pedestrians"] += int(ok.sum()); WORST["left_out"] += int(band.sum()); WORST["onsets"] += int(np.sum(w_step >= 0))


# ---- against the restatement --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuzz_set():
    """about 300 ragged encounters with their roll-outs' drift, and the restatement's answers, computed once"""
    rng = np.random.default_rng(2028)
    encs = [fc.with_drift(rng, e) for e in fc.fuzz(31, 300)]
    sims = [dict(e, ped_xy=fc.rollout_of(e)) for e in encs]
    truth = [e["ped_xy"] for e in encs]
    want = {"real": fc.evaluate(encs), "vel": fc.evaluate(encs, with_vel=True),
            "sim": fc.evaluate(sims, truth=truth, interaction_distance=3.0)}
    for v in want.values():
        for a in v:
            a.setflags(write=False)
    return encs, sims, truth, want


def test_fuzz_matches_the_restatement(engine, fuzz_set):
    encs, sims, truth, want = fuzz_set
    compare(good(engine, encs), want["real"], "recorded")
    compare(good(engine, encs, with_vel=True), want["vel"], "recorded, ped_vel")
    compare(good(engine, sims, truth=truth, interaction_distance=3.0), want["sim"], "simulated")
    assert np.sum(want["real"][3] >= 0) >= 300 and not want["real"][4].any()
    assert np.any(want["sim"][0]["err_count"] == 0) and np.any(want["sim"][0]["err_count"] > 0)
    # ped_vel given against ped_vel differenced: each follows its own rule
    assert not np.array_equal(want["real"][3], want["vel"][3])


def test_an_encounters_outputs_do_not_depend_on_the_call(engine, fuzz_set):
    encs, sims, truth, _ = fuzz_set
    n = len(encs)
    so = np.concatenate([[0], np.cumsum([len(e["ego_xy"]) for e in encs])])
    pb = np.concatenate([[0], np.cumsum([e["ped_xy"].shape[1] for e in encs])])
    rec, series, dist, step = good(engine, sims, truth=truth, interaction_distance=3.0)

    def pieces(order, got):
        g_so = np.concatenate([[0], np.cumsum([so[i + 1] - so[i] for i in order])])
        g_pb = np.concatenate([[0], np.cumsum([pb[i + 1] - pb[i] for i in order])])
        for k, i in enumerate(order):
            assert got[0][k:k + 1].tobytes() == rec[i:i + 1].tobytes(), f"record of encounter {i}"
            assert got[1][g_so[k]:g_so[k + 1]].tobytes() == series[so[i]:so[i + 1]].tobytes(), f"series of encounter {i}"
            assert got[2][g_pb[k]:g_pb[k + 1]].tobytes() == dist[pb[i]:pb[i + 1]].tobytes(), f"onset distances of encounter {i}"
            assert got[3][g_pb[k]:g_pb[k + 1]].tobytes() == step[pb[i]:pb[i + 1]].tobytes(), f"onset steps of encounter {i}"

    for order in (list(range(n))[::-1], list(range(0, n, 2)) + list(range(1, n, 2))):
        pieces(order, good(engine, [sims[i] for i in order], truth=[truth[i] for i in order], interaction_distance=3.0))
    for i in range(n):                                              # one per call
        pieces([i], good(engine, [sims[i]], truth=[truth[i]], interaction_distance=3.0))


def test_edges(engine):
    edges = fc.edge_encounters()
    encs = [e for _, e, _, _ in edges]
    base = np.concatenate([[0], np.cumsum([e["ped_xy"].shape[1] for e in encs])])
    for with_vel, col in ((False, 2), (True, 3)):
        got = good(engine, encs, with_vel=with_vel)
        compare(got, fc.evaluate(encs, with_vel=with_vel), f"edges, ped_vel {with_vel}")
        for i, edge in enumerate(edges):
            if edge[col] is not None:
                step = got[3][base[i]:base[i + 1]]
                assert {j: int(s) for j, s in enumerate(step) if s >= 0} == edge[col], edge[0]
    # the 257-pedestrian encounter first in its call: its evaders are the last lane of a wave and the first of the next
    i = [name for name, _, _, _ in edges].index("onset_lanes_63_64")
    rec, _, dist, step = good(engine, [encs[i], encs[0]])
    assert np.nonzero(step[:257] >= 0)[0].tolist() == [63, 64] and int(rec["n_onset"][0]) == 2
    # twice in range: the first occurrence wins
    k = [name for name, _, _, _ in edges].index("onset_twice")
    rec, series, dist, step = good(engine, [encs[k]])
    assert step[0] == 4 and dist[0] == fc.distances(encs[k]["ego_xy"], encs[k]["ped_xy"])[4, 0]
    # the onset distance is the bits of the separation of that (step, pedestrian) pair
    assert dist[0] == series[4]


def test_interaction_distance_keeps_all_some_or_none(engine):
    rng = np.random.default_rng(9)
    encs = [fc.with_drift(rng, fc.random_encounter(rng, 30, 9, 0.4)) for _ in range(4)]
    sims, truth = [dict(e, ped_xy=fc.rollout_of(e)) for e in encs], [e["ped_xy"] for e in encs]
    nearest = np.concatenate([np.min(fc.distances(e["ego_xy"], e["ped_xy"]), axis=0) for e in encs])
    some = float(np.median(nearest))
    kept = {}
    for label, inter in (("all", None), ("all_far", 1e6), ("some", some), ("none", 1e-6)):
        got = good(engine, sims, truth=truth, interaction_distance=inter)
        compare(got, fc.evaluate(sims, truth=truth, interaction_distance=inter), label)
        kept[label] = int(got[0]["err_count"].sum()) // 29
    assert kept["all"] == kept["all_far"] == 36 and 0 < kept["some"] < 36 and kept["none"] == 0
    assert fidelity.rollout_ade(engine, encs, [s["ped_xy"] for s in sims], 1e-6) == float("inf")
    # without truth: no error
    rec = good(engine, encs)[0]
    assert not rec["err_sum"].any() and not rec["err_count"].any()


def test_exact_thresholds_on_dyadic_inputs(engine):
    """dt = 0.5, coordinates on multiples of 1/8, the ego at the origin, the pedestrian on an axis: `away` is exact whatever
    is fused, and these hold bit for bit."""
    e = fc.axis_encounter([3, 3, 3, 3, 3.25])                     # away = 0, 0, 0.25, 0.5, 0.5
    for thr, want in ((0.25, 3), (float(np.nextafter(0.25, 0)), 2), (0.5, -1), (float(np.nextafter(0.5, 0)), 3)):
        rec, series, dist, step = good(engine, [e], accel_threshold=thr)
        assert step.tolist() == [want], thr                      # away == threshold: no onset; one binade step above: onset
        w = fc.evaluate([e], accel_threshold=thr)
        assert rec.tobytes() == w[0].tobytes() and series.tobytes() == w[1].tobytes() and np.array_equal(dist, w[2], equal_nan=True)
    e = fc.axis_encounter([5, 5, 5, 5, 6])                        # away[2] = 1 at dist 5
    for max_d, want in ((5.0, 2), (float(np.nextafter(5.0, 0)), -1), (float(np.nextafter(5.0, 9)), 2)):
        rec, series, dist, step = good(engine, [e], max_distance=max_d)
        assert step.tolist() == [want] and (want < 0 or dist.tolist() == [5.0]), max_d           # dist == max_distance is kept
    e = fc.axis_encounter(None, py=[0, 0, 0, 0, 1])               # on the ego until the last step: skipped before any division
    rec, series, dist, step = good(engine, [e])
    assert step.tolist() == [4] and dist.tolist() == [1.0] and series.tolist() == [0, 0, 0, 0, 1]
    assert float(rec["closest"][0]) == 0.0 and int(rec["closest_step"][0]) == 0 and int(rec["n_onset"][0]) == 1


def test_a_nan_coordinate_stays_where_it_is(engine):
    rng = np.random.default_rng(11)
    clean = [fc.random_encounter(rng, 12, 3, 0.4), fc.designed(12, 3, [0, 1, 2], range(3, 12)), fc.random_encounter(rng, 9, 2, 0.1)]
    dirty = [dict(e, ped_xy=e["ped_xy"].copy()) for e in clean]
    dirty[1]["ped_xy"][5, 1, 0] = np.nan
    a, b = good(engine, clean), good(engine, dirty)
    w = fc.evaluate(dirty)
    assert np.array_equal(b[1], w[1], equal_nan=True) and np.array_equal(b[3], w[3]) and np.array_equal(b[2], w[2], equal_nan=True)
    series = b[1][12:24]
    assert np.isnan(series[5]) and not np.isnan(np.delete(series, 5)).any()
    assert np.isnan(b[0]["closest"][1]) and b[0]["closest_step"][1] == -1
    assert a[0][[0, 2]].tobytes() == b[0][[0, 2]].tobytes()        # the encounters beside it
    assert a[3][3:6].tolist() == [3, 3, 3]
    assert b[3][3:6].tolist() == [3, 4, 3]                          # steps 3, 5 and 7 carry a NaN acceleration; step 4 does not
    assert b[2][3] == a[2][3] and b[2][5] == a[2][5]                # the pedestrians beside it


def test_series_equals_the_legacy_series_of_the_footprint_recheck(engine):
    """fixed-population trajectories: the same distances, the same minimum -- bit for bit"""
    rng = np.random.default_rng(17)
    encs = [fc.random_encounter(rng, T, N, 0.4) for T, N in ((40, 7), (3, 1), (65, 64), (2, 65))]
    _, series, _, _ = good(engine, encs)
    steps = [len(e["ego_xy"]) for e in encs]
    step_off = np.concatenate([[0], np.cumsum(steps)]).astype(np.int32)
    counts = np.concatenate([[e["ped_xy"].shape[1]] * len(e["ego_xy"]) for e in encs])
    ped_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    xy = np.concatenate([e["ego_xy"] for e in encs])
    ped = np.concatenate([e["ped_xy"].reshape(-1, 2) for e in encs])
    _, fp_series, _ = engine.footprint_recheck(safety.footprint_geometry(None), step_off, xy, np.zeros(len(xy)), ped_off, ped,
                                               want_series=True)
    assert series.tobytes() == np.ascontiguousarray(fp_series["legacy"]).tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
REFUSALS = [("p_null", dict(null=("p",))), ("step_off_null", dict(null=("step_off",))), ("n_ped_null", dict(null=("n_ped",))),
            ("dt_null", dict(null=("dt",))), ("ego_null", dict(null=("ego_xy",))), ("ped_null", dict(null=("ped_xy",))),
            ("out_null", dict(null=("out",))), ("n_enc_negative", dict(n_enc=-1)), ("step_off_from_1", dict(step_off=[1, 4, 6])),
            ("step_off_decreasing", dict(step_off=[0, 4, 3])), ("no_step", dict(step_off=[0, 4, 4])),
            ("n_ped_negative", dict(n_ped=[2, -1])), ("dt_zero", dict(dt=[0.4, 0.0])), ("dt_negative", dict(dt=[-0.1, 0.4])),
            ("dt_nan", dict(dt=[np.nan, 0.4])), ("dt_inf", dict(dt=[0.4, np.inf])),
            ("threshold_nan", dict(accel_threshold=np.nan)), ("max_distance_nan", dict(max_distance=np.nan))]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_change_nothing(engine, name, change):
    rng = np.random.default_rng(3)
    encs = [fc.random_encounter(rng, 4, 2, 0.4), fc.random_encounter(rng, 2, 2, 0.4)]
    rc, _, _, _, _, untouched = call(engine, encs, **change)
    assert rc == _abi.ERR_INVALID and untouched
    assert _abi.lib().fot_last_error(engine._h)
    assert call(engine, encs)[0] == _abi.OK                         # the handle is as good as before


def test_no_encounter_succeeds_and_writes_nothing(engine):
    rc, _, _, _, _, untouched = call(engine, [])
    assert rc == _abi.OK and untouched
    out = fidelity.fidelity_batch(engine, [])
    assert len(out["records"]) == 0 and out["series"] == []
