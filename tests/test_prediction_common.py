"""The NumPy restatements of tests/prediction_common.py against the reference's own vectors (no GPU): before they check
a kernel they reproduce every stored result of process_prediction, predict_cv, the closest-to-mean pick and
compute_safety_metrics_static at the 1e-12 the oracle is held to."""
import json
import os

import numpy as np
import pytest

import prediction_common as pc
from conftest import GOLDEN_DIR

TOL = dict(rtol=1e-12, atol=1e-12)


def _load(*path):
    z = np.load(os.path.join(GOLDEN_DIR, *path), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def test_process_prediction_and_predict_cv_reproduce_the_reference():
    cases = _load("prediction", "cases.npz")
    assert len(cases["meta"]["resample"]) == 30
    for m in cases["meta"]["resample"]:
        c = m["case"]
        kw = dict(sgan_dt=m["sgan_dt"], sim_dt=m["sim_dt"], plan_horizon=m["plan_horizon"])
        anchor = cases[f"c{c}_anchor"] if m["with_anchor"] else None
        got = pc.process_prediction(cases[f"c{c}_pred"], anchor, m["staleness"], **kw)
        want = cases[f"c{c}_dense"]
        assert got.shape == want.shape, m
        assert got.shape[1] == pc.n_dense(m["sgan_dt"], m["sim_dt"], m["plan_horizon"], m["pred_len"])
        np.testing.assert_allclose(got, want, err_msg=str(m), **TOL)
        last = cases[f"c{c}_cv1"][:, 0, :]                         # zero velocity: every row is the last observation
        cv = pc.predict_cv(last, cases[f"c{c}_prev"], m["staleness"], pred_len=m["pred_len"], **kw)
        np.testing.assert_allclose(cv, cases[f"c{c}_cv"], err_msg=str(m), **TOL)
        cv1 = pc.predict_cv(last, None, m["staleness"], pred_len=m["pred_len"], **kw)
        np.testing.assert_allclose(cv1, cases[f"c{c}_cv1"], err_msg=str(m), **TOL)


def test_closest_to_mean_reproduces_the_reference():
    cases = _load("prediction", "cases.npz")
    assert cases["meta"]["select"]
    for m in cases["meta"]["select"]:
        d = pc.sample_distances(cases[f"s{m['case']}_samples"])
        assert int(np.argmin(d)) == m["best"], m


def test_safety_metrics_reproduce_the_reference():
    cases = _load("safety", "cases.npz")
    assert len(cases["meta"]) == 70
    for i, m in enumerate(cases["meta"]):
        fp = m["footprint"]
        kw = {} if fp is None else dict(offsets=fp["offsets"], footprint_radius=fp["radius"])
        got = pc.safety_metrics(cases[f"c{i}_ego"], cases[f"c{i}_pos"], cases[f"c{i}_vel"], m["ego_radius"],
                                m["ped_radius"], **kw)
        want = cases[f"c{i}_want"]
        assert got["collision"] == bool(want[1]), i
        for k, j in (("min_distance", 0), ("ttc", 2), ("clearance", 3), ("clearance_ahead", 4)):
            np.testing.assert_allclose(got[k], want[j], err_msg=f"case {i} {k}", **TOL)


def test_predict_cv_follows_the_observation_dtype():
    """float32 observations: float32 velocity, float64 extrapolation -- not the float64 result of the same numbers."""
    rng = np.random.default_rng(4)
    last, prev = rng.normal(0, 20, (9, 2)), rng.normal(0, 20, (9, 2))
    a = pc.predict_cv(last.astype(np.float32), prev.astype(np.float32), 0.2)
    b = pc.predict_cv(last.astype(np.float32).astype(np.float64), prev.astype(np.float32).astype(np.float64), 0.2)
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape == (9, 50, 2)
    assert 1e-7 < np.abs(a - b).max() < 1e-3
    with pytest.raises(AssertionError):
        pc.predict_cv(last.astype(np.float32), prev, 0.2)


def test_pairwise_selection_covers_every_value_and_is_seeded():
    cases = pc.resample_cases()
    assert cases == pc.resample_cases()
    for name, values in pc.RESAMPLE_AXES.items():
        for v in values:
            assert any(c[name] == v for c in cases), (name, v)
    assert all(pc.resample_case_valid(c) for c in cases)
    assert len(cases) < 80
