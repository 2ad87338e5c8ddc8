"""The NumPy restatement of the encounter-fidelity statistics (tests/fidelity_common.py) pinned to the reference's own answers
(tests/golden/fidelity/cases.npz, made by tests/golden/make_fidelity.py).  No GPU.

Separation, closest approach and per-element errors: equal bits (the same NumPy operations).  Onset steps: equal.  Onset
distances and `away`: within 4 * 2^-52 relative -- the reference's np.dot and 1-D norm may fuse one multiply-add,
everything in front of them is the same roundings.  Error sums: within count * 2^-52 * sum (two orders of one sum)."""
import os

import numpy as np
import pytest

import fidelity_common as fc


@pytest.fixture(scope="module")
def fix():
    return fc.load_cases()


def groups(fix):
    return {g: fc.golden_encounters(fix, g) for g in fix["meta"]["groups"]}


def test_fixture_holds_what_the_tests_need(fix):
    meta = fix["meta"]
    assert os.path.getsize(fc.GOLDEN) < 512 * 1024
    assert meta["groups"] == {"ref": 5, "rand": 40}
    rand = fc.golden_encounters(fix, "rand")
    T = [len(e["ego_xy"]) for e in rand]
    N = [e["ped_xy"].shape[1] for e in rand]
    assert min(T) == 2 and max(T) == 70 and min(N) == 0 and max(N) == 12
    assert {e["dt"] for e in rand} == set(fc.DTS)
    counts = meta["counts"]["rand"]
    assert counts["pedestrians"] >= 150 and counts["onsets_real_fd"] >= 40 and counts["closest_margin"] >= fc.BAND
    assert list(meta["report"]["rand"]) == ["n_encounters", "rollout_ade", "mean_closest_sim", "mean_closest_real", "ks_closest",
                                            "p_closest", "n_onset_sim", "n_onset_real", "ks_onset", "p_onset", "closest_sim_raw",
                                            "closest_real_raw", "onset_sim_raw", "onset_real_raw", "onset_per_enc_sim_raw",
                                            "onset_per_enc_real_raw"]


def test_separation_and_closest_equal_the_references_bits(fix):
    for g, encs in groups(fix).items():
        for i, e in enumerate(encs):
            for side, pos in (("real", e["ped_xy"]), ("sim", fc.rollout_of(e))):
                got = fc.separation(e["ego_xy"], pos)
                assert got.tobytes() == fix[f"{g}_{i}_sep_{side}"].tobytes(), f"{g} {i} {side}"
        rep = fix["meta"]["report"][g]
        real = [float(fc.record(e["ego_xy"], e["ped_xy"], dt=e["dt"])[0]["closest"]) for e in encs]
        sim = [float(fc.record(e["ego_xy"], fc.rollout_of(e), dt=e["dt"])[0]["closest"]) for e in encs]
        assert real == rep["closest_real_raw"] and sim == rep["closest_sim_raw"]


def test_the_references_own_cases(fix):
    """what the reference's tests assert of their inputs, of the restatement"""
    ref = fc.golden_encounters(fix, "ref")
    assert fc.separation(ref[0]["ego_xy"], ref[0]["ped_xy"]).tolist() == [3.0, 1.0]
    assert np.all(np.isinf(fc.separation(ref[1]["ego_xy"], ref[1]["ped_xy"]))) and len(ref[1]["ego_xy"]) == 3
    for vel in (None, ref[2]["ped_vel"]):
        step, where, _, _ = fc.onset(ref[2]["ego_xy"], ref[2]["ped_xy"], vel, dt=0.4)
        assert step.tolist() == [1] and where[0] == 3.0
    assert fc.onset(ref[3]["ego_xy"], ref[3]["ped_xy"], dt=0.4)[0].tolist() == [-1]          # a steady approach
    assert fc.onset(ref[4]["ego_xy"], ref[4]["ped_xy"], dt=0.4)[0].tolist() == [-1]          # an evasion out of range
    with pytest.raises(ValueError, match=r"ego_xy T=2 != ped_xy T=3"):
        fc.separation(np.zeros((2, 2)), np.zeros((3, 1, 2)))


def test_onsets_equal_the_references(fix):
    worst, n_onsets = 0.0, 0
    for g, encs in groups(fix).items():
        for i, e in enumerate(encs):
            for side, pos in (("real", e["ped_xy"]), ("sim", fc.rollout_of(e))):
                for branch, vel in (("fd", None), ("vel", e["ped_vel"])):
                    k = f"{g}_{i}_"
                    if k + f"step_{side}_{branch}" not in fix:
                        continue
                    step, where, away, band = fc.onset(e["ego_xy"], pos, vel, dt=e["dt"])
                    assert g == "ref" or not band.any()          # (the reference's own cases sit ON max_distance)
                    assert np.array_equal(step, fix[k + f"step_{side}_{branch}"]), f"{k}{side} {branch}: steps"
                    hit = step >= 0
                    want_d, want_a = fix[k + f"onset_{side}_{branch}"], fix[k + f"away_{side}_{branch}"][hit]
                    assert want_d.shape == where[hit].shape
                    for got, want in ((where[hit], want_d), (away[hit], want_a)):
                        if got.size:
                            rel = float(np.max(np.abs(got - want) / np.abs(want)))
                            assert rel <= fc.REL_FUSED, f"{k}{side} {branch}: {rel:.3e}"
                            worst = max(worst, rel)
                    # the onset distance is the separation's own distance of that (step, pedestrian) pair
                    d = fc.distances(e["ego_xy"], pos)
                    assert np.array_equal(where[hit], d[step[hit], np.nonzero(hit)[0]])
                    assert np.array_equal(fc.onset_loop(e["ego_xy"], pos, vel, dt=e["dt"]), where[hit])
                    n_onsets += int(hit.sum())
    assert n_onsets >= 150
    print(f"{n_onsets} onsets, largest relative difference to the reference {worst:.3e}")


def test_rollout_error_within_the_bound_of_a_reordered_sum(fix):
    meta = fix["meta"]
    for g, encs in groups(fix).items():
        sims = [fc.rollout_of(e) for e in encs]
        for wants, inter in (((meta["rollout_ade"][g], meta["report"][g]["rollout_ade"]), None),
                             ((meta["rollout_ade_interaction"][g],), meta["interaction_distance"])):
            total, count = 0.0, 0
            for e, s in zip(encs, sims):
                r = fc.record(e["ego_xy"], s, truth_xy=e["ped_xy"], dt=e["dt"], interaction_distance=inter)[0]
                total += float(r["err_sum"])
                count += int(r["err_count"])
            assert count > 0
            for want in wants:                                      # (the mean's own division: one more rounding)
                assert abs(total / count - want) <= fc.sum_tol(count, want) + fc.EPS * want, (g, inter)
    # per-element errors: the same bits as the norm over the last axis
    e = groups(fix)["rand"][2]
    _, _, err = fc.ped_error(e["ego_xy"], fc.rollout_of(e), e["ped_xy"])
    assert err.tobytes() == np.linalg.norm(fc.rollout_of(e) - e["ped_xy"], axis=2).tobytes()
    # none kept: the count is 0
    r = fc.record(e["ego_xy"], fc.rollout_of(e), truth_xy=e["ped_xy"], dt=e["dt"], interaction_distance=1e-6)[0]
    assert int(r["err_count"]) == 0 and float(r["err_sum"]) == 0.0 and meta["rollout_ade_none"] == float("inf")


def test_ks_statistic_equals_the_references(fix):
    ks = fix["meta"]["ks"]
    assert fc.ks_statistic(fix["ks_a"], fix["ks_b"]) == ks["same"][0]
    assert fc.ks_statistic(fix["ks_a"], fix["ks_c"]) == ks["different"][0]
    assert fc.ks_statistic(fix["ks_tied_a"], fix["ks_tied_b"]) == ks["tied"][0]
    finite = fix["ks_nonfinite"][np.isfinite(fix["ks_nonfinite"])]
    assert fc.ks_statistic(finite, fix["ks_b"]) == ks["nonfinite"][0]
