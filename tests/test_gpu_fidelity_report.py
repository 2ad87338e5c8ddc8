"""The Python layer of the encounter-fidelity statistics on the GPU (integrated_path_planning_amd/fidelity.py):
fidelity_report against the reference's own dictionary (tests/golden/fidelity/cases.npz), rollout_ade, the single-encounter
functions, calculate_min_separation on a trajectory.npz the suite writes, and the KS statistic against scipy's.

Bounds (tests/fidelity_common.py): closest approaches and the KS statistics are exact; onset distances within 4 * 2^-52
relative (the reference's np.dot and 1-D norm may fuse one multiply-add); error means within count * 2^-52 * mean."""
import os

import numpy as np
import pytest

import fidelity_common as fc
from integrated_path_planning_amd import fidelity, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return fc.load_cases()


@pytest.fixture(scope="module")
def engine():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        yield bp


@pytest.mark.parametrize("group", ("ref", "rand"))
def test_report_equals_the_references_dictionary(fix, engine, group):
    encs = fc.golden_encounters(fix, group)
    sims = [fc.rollout_of(e) for e in encs]
    want = fix["meta"]["report"][group]
    got = fidelity.fidelity_report(engine, encs, sims)
    assert list(got) == list(want)                                  # key for key, in the reference's order
    for k in ("n_encounters", "n_onset_sim", "n_onset_real", "ks_closest", "ks_onset", "closest_sim_raw", "closest_real_raw"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    for k in ("onset_sim_raw", "onset_real_raw", "onset_per_enc_sim_raw", "onset_per_enc_real_raw", "mean_closest_sim",
              "mean_closest_real"):
        assert np.shape(got[k]) == np.shape(want[k]), k
        assert np.allclose(got[k], want[k], rtol=fc.REL_FUSED, atol=0.0, equal_nan=True), k
    count = sum((len(e["ego_xy"]) - 1) * e["ped_xy"].shape[1] for e in encs)
    assert abs(got["rollout_ade"] - want["rollout_ade"]) <= fc.sum_tol(count, want["rollout_ade"])
    assert isinstance(got["onset_sim_raw"], list) and isinstance(got["n_onset_sim"], int)


@pytest.mark.parametrize("group", ("ref", "rand"))
def test_report_p_values_equal_the_references(fix, engine, group):
    pytest.importorskip("scipy")
    encs = fc.golden_encounters(fix, group)
    got = fidelity.fidelity_report(engine, encs, [fc.rollout_of(e) for e in encs])
    for k in ("p_closest", "p_onset"):
        want = fix["meta"]["report"][group][k]
        assert abs(got[k] - want) <= 1e-9 * abs(want), k          # scipy's own p of the same statistic and sizes


def test_rollout_ade(fix, engine):
    meta = fix["meta"]
    for g in ("ref", "rand"):
        encs = fc.golden_encounters(fix, g)
        sims = [fc.rollout_of(e) for e in encs]
        count = sum((len(e["ego_xy"]) - 1) * e["ped_xy"].shape[1] for e in encs)
        for inter, want in ((None, meta["rollout_ade"][g]), (meta["interaction_distance"], meta["rollout_ade_interaction"][g])):
            got = fidelity.rollout_ade(engine, encs, sims, interaction_distance=inter)
            assert abs(got - want) <= fc.sum_tol(count, want) + fc.EPS * want, (g, inter)
        assert fidelity.rollout_ade(engine, encs, sims, interaction_distance=1e-6) == float("inf")
    assert fidelity.rollout_ade(engine, [], []) == float("inf")


def test_single_encounter_functions(fix, engine):
    ref = fc.golden_encounters(fix, "ref")
    assert fidelity.min_separation_series(engine, ref[0]["ego_xy"], ref[0]["ped_xy"]).tolist() == [3.0, 1.0]
    assert np.all(np.isinf(fidelity.min_separation_series(engine, ref[1]["ego_xy"], ref[1]["ped_xy"])))
    with pytest.raises(ValueError, match=r"ego_xy T=2 != ped_xy T=3"):
        fidelity.min_separation_series(engine, np.zeros((2, 2)), np.zeros((3, 1, 2)))
    e = ref[2]
    assert fidelity.avoidance_onset_distance(engine, e["ego_xy"], e["ped_xy"]).tolist() == [3.0]
    assert fidelity.avoidance_onset_distance(engine, e["ego_xy"], e["ped_xy"], ped_vel=e["ped_vel"]).tolist() == [3.0]
    assert fidelity.avoidance_onset_distance(engine, ref[3]["ego_xy"], ref[3]["ped_xy"]).size == 0
    assert fidelity.avoidance_onset_distance(engine, ref[4]["ego_xy"], ref[4]["ped_xy"], max_distance=5.0).size == 0
    assert fidelity.avoidance_onset_distance(engine, ref[4]["ego_xy"], ref[4]["ped_xy"], max_distance=9.5).size == 1
    for i, e in enumerate(fc.golden_encounters(fix, "rand")[:8]):
        for branch, vel in (("fd", None), ("vel", e["ped_vel"])):
            got = fidelity.avoidance_onset_distance(engine, e["ego_xy"], e["ped_xy"], ped_vel=vel, dt=e["dt"])
            want = fix[f"rand_{i}_onset_real_{branch}"]
            assert got.shape == want.shape and np.allclose(got, want, rtol=fc.REL_FUSED, atol=0.0), (i, branch)
        assert fidelity.min_separation_series(engine, e["ego_xy"], e["ped_xy"]).tobytes() == fix[f"rand_{i}_sep_real"].tobytes()


def test_calculate_min_separation_on_a_trajectory_file(fix, engine, tmp_path):
    e = fc.golden_encounters(fix, "rand")[2]
    obj = np.empty(len(e["ego_xy"]), dtype=object)
    for t in range(len(obj)):
        obj[t] = e["ped_xy"][t]
    arrays = dict(ego_x=e["ego_xy"][:, 0], ego_y=e["ego_xy"][:, 1], ped_positions=obj)
    path = os.path.join(tmp_path, "trajectory.npz")
    np.savez(path, **arrays)
    series, overall = fidelity.calculate_min_separation(engine, path)
    assert series.tobytes() == fix["rand_2_sep_real"].tobytes() and overall == float(np.min(fix["rand_2_sep_real"]))
    # a history of results, the reference's attribute names and this package's
    from types import SimpleNamespace as NS
    theirs = [NS(ego_state=NS(x=x, y=y), ped_state=NS(positions=p)) for (x, y), p in zip(e["ego_xy"], e["ped_xy"])]
    ours = [NS(ego=NS(x=x, y=y), ped_positions=p) for (x, y), p in zip(e["ego_xy"], e["ped_xy"])]
    for hist in (theirs, ours):
        s, o = fidelity.calculate_min_separation(engine, hist)
        assert s.tobytes() == series.tobytes() and o == overall
    # what BatchedClosedLoop.save_results writes: the same keys through the same function
    saved = BatchedClosedLoop.trajectory_arrays([])
    assert {"ego_x", "ego_y", "ped_positions"} <= set(saved)
    theirs[3].ped_state.positions = theirs[3].ped_state.positions[:-1]
    with pytest.raises(ValueError, match="fixed pedestrian population"):
        fidelity.calculate_min_separation(engine, theirs)
    obj[3] = obj[3][:-1]
    np.savez(path, **arrays)
    with pytest.raises(ValueError, match="fixed pedestrian population"):
        fidelity.calculate_min_separation(engine, path)


def test_ks_statistic_against_scipy_on_tied_and_untied_samples():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(4)
    for n_a, n_b, tied in ((1, 1, False), (7, 7, False), (40, 23, False), (500, 500, False), (60, 45, True), (9, 300, True)):
        a, b = rng.normal(0.0, 1.0, n_a), rng.normal(0.3, 1.2, n_b)
        if tied:
            a, b = np.round(a * 2) / 2, np.round(b * 2) / 2
        stat, p = fidelity.compare_distributions_ks(a, b)
        ref = stats.ks_2samp(a, b)
        assert stat == float(ref.statistic) and p == float(ref.pvalue), (n_a, n_b, tied)
