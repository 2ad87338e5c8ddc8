"""The NumPy restatement of the external-path checks (tests/check_paths_common.py) against the reference's own answers
(tests/golden/check_paths/cases.npz, no GPU): categories and free / hit answers exactly; the CPU oracle's unused entry
orc_path_collision_free against the same answers; and the fuzz generator alone, over the seeds the GPU test uses, with
the share of cases inside the 1e-9 band under its cap."""
import collections
import os

import numpy as np
import pytest

import check_paths_common as pc
from conftest import GOLDEN_DIR


@pytest.fixture(scope="module")
def fixture():
    return pc.load_calls(os.path.join(GOLDEN_DIR, "check_paths", "cases.npz"))


def test_fixture_is_the_shared_cases(fixture):
    """The stored inputs are what class_calls() / fuzz_call() build today (the GPU test runs both)."""
    calls, _ = fixture
    built = pc.class_calls()
    built += [pc.fuzz_call(s) for s in range(len(calls) - len(built))]
    assert [c["name"] for c in calls] == [c["name"] for c in built]
    for a, b in zip(calls, built):
        assert a["cfg"] == b["cfg"] and a["overrides"] == b["overrides"] and a["max_stop"] == b["max_stop"], a["name"]
        assert len(a["paths"]) == len(b["paths"])
        for p, q in zip(a["paths"], b["paths"]):
            for f in pc.FIELDS:
                np.testing.assert_array_equal(p[f], q[f], err_msg=f"{a['name']} {f}")
        for key in ("static", "dyn", "dist"):
            assert (a[key] is None) == (b[key] is None), a["name"]
            if a[key] is not None:
                np.testing.assert_array_equal(a[key], b[key], err_msg=a["name"])


def test_restatement_reproduces_the_reference(fixture):
    calls, expected = fixture
    seen = collections.Counter()
    for cl, ex in zip(calls, expected):
        cat, free, _ = pc.evaluate(cl)
        assert cat.tolist() == ex["cat"].tolist(), cl["name"]
        assert free.tolist() == ex["free"].tolist(), cl["name"]
        seen.update(pc.CATEGORIES[k] for k in cat)
    assert set(seen) == set(pc.CATEGORIES), seen
    assert sum(seen.values()) >= 300


def test_fixture_holds_the_ragged_answers_the_issue_names(fixture):
    """What the reference says where the arrays differ in length: the rules reach as far as the arrays they read."""
    calls, expected = fixture
    by_name = {c["name"]: e["cat"][0] for c, e in zip(calls, expected)}
    assert by_name["ragged_geo_s_len8_bad6"] == pc.CURV              # a slip inside the short s: still a curvature error
    assert by_name["ragged_geo_s_len4_bad6"] == pc.OK                # behind it: no low-speed rule
    assert by_name["ragged_d_len8_bad6"] == pc.ROAD                  # d shorter than x still bounds the road
    assert by_name["ragged_d_len16_bad14"] == pc.ROAD                # ... and longer than x
    assert by_name["ragged_v_len8_bad6"] == pc.SPEED
    assert by_name["ragged_v_len16_bad14"] == pc.SPEED
    assert by_name["ragged_short_v_no_lowspeed_behind_it"] == pc.OK  # no zero speed is made up behind a short v
    assert by_name["ragged_nonfinite_behind_x"] == pc.DROPPED
    assert by_name["ragged_stop_v_len0"] == pc.STOP


def test_oracle_path_collision_free_reproduces_the_reference(fixture):
    from oracle import oracle as orc
    calls, expected = fixture
    n = 0
    for cl, ex in zip(calls, expected):
        c = dict(cl["cfg"])
        fp = c.pop("footprint")
        if fp is not None:
            c.update(footprint_offsets=fp[0], footprint_radius=fp[1])
        params = orc.make_params(**c)
        for p, want in zip(cl["paths"], ex["free"]):
            if len(p["x"]) == 0:
                continue
            got = orc.path_collision_free(params, p["x"], p["y"], p["yaw"], p["t"], cl["static"], cl["dyn"], cl["dist"])
            assert got == bool(want), cl["name"]
            n += 1
    assert n >= 300


def test_fuzz_generator_stays_out_of_the_band():
    """The generator alone over the GPU test's seeds: at most BAND_CAP of the cases may lie within BAND of a threshold
    (continuous random inputs: expected none), and every category is a fair share of the draw."""
    n = inside = 0
    seen = collections.Counter()
    for seed in pc.FUZZ_SEEDS:
        cl = pc.fuzz_call(seed)
        assert 1 <= len(cl["paths"]) <= 8 and all(len(p["x"]) <= 64 for p in cl["paths"])
        cat, _, margin = pc.evaluate(cl)
        n += len(cat)
        inside += int((margin < pc.BAND).sum())
        seen.update(pc.CATEGORIES[k] for k in cat)
    print(f"fuzz: {n} paths, {inside} inside the band, categories {dict(seen)}")
    assert len(pc.FUZZ_SEEDS) == 300 and n > 1000
    assert inside <= pc.BAND_CAP * n, (inside, n)
    for name in pc.CATEGORIES:
        assert seen[name] >= 0.05 * n, (name, seen)


def test_eps_pairs_straddle_an_integer():
    (e_lo, s_lo), (e_hi, s_hi) = pc.eps_pairs()[:2]
    assert e_lo * s_lo < round(e_lo * s_lo) and np.floor(e_lo * s_lo) == round(e_lo * s_lo) - 1
    assert e_hi * s_hi > round(e_hi * s_hi) and np.floor(e_hi * s_hi) == round(e_hi * s_hi)
    assert abs(e_lo * s_lo - round(e_lo * s_lo)) < 1e-12 and abs(e_hi * s_hi - round(e_hi * s_hi)) < 1e-12
