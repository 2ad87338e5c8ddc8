"""BatchedClosedLoop(prediction_scores=True) on the GPU: the reference's distribution episodes scored step by step while the
loop runs -- through the host hand-over (fot_prediction_scores) and with the samples resident in HBM
(fot_loop_prediction_scores) -- against the reference's own calculate_aggregate_metrics dictionaries."""
import numpy as np
import pytest

from closed_loop_common import scripted_sample_source
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from pred_scores_common import METRIC_KEYS, assert_metrics_match_reference, load_cases
from test_pred_scores_cpu import EPISODES

pytestmark = pytest.mark.gpu
AWARE = tuple(n for n in EPISODES if n != "s5_best_only")           # device_samples needs distribution-aware planning


@pytest.fixture(scope="module")
def fix():
    return load_cases()


def _sources(ep):
    import torch
    host = scripted_sample_source(ep["n_samples"], ep["config"]["pred_len"])
    dev = torch.device("cuda", 0)
    return host, lambda last, prev: torch.from_numpy(np.ascontiguousarray(host(last, prev), dtype=np.float64)).to(dev)


def _steps(hists):
    return [[(r.ego.x, r.ego.y, r.ego.yaw, r.ego.v, r.ego.a, r.ego.jerk, r.ego.state, tuple(sorted(r.metrics.items())),
              None if r.planned_path is None else (r.planned_path.cost, tuple(r.planned_path.x))) for r in h] for h in hists]


@pytest.fixture(scope="module")
def host_runs(fix):
    """Every episode once through the host hand-over with scores on: (metrics, per-step records)."""
    out = {}
    for name in EPISODES:
        ep = fix["meta"]["episodes"][name]
        host, _ = _sources(ep)
        with BatchedClosedLoop(dict(ep["config"]), [fix[name + "_ped_traj"]], sample_source=host, prediction_scores=True) as sim:
            hists = sim.run()
            assert len(hists[0]) == ep["steps"] and sim.episodes[0].termination_reason == ep["termination"]
            out[name] = (sim.prediction_metrics()[0], _steps(hists))
    return out


@pytest.mark.parametrize("name", EPISODES)
def test_host_hand_over_matches_the_reference(fix, host_runs, name):
    got = host_runs[name][0]
    assert tuple(got) == METRIC_KEYS
    print(name, got)
    assert_metrics_match_reference(got, fix["meta"]["episodes"][name]["reference"], fix["meta"]["nll_atol"], name)


@pytest.mark.parametrize("name", AWARE)
def test_samples_resident_in_hbm_match_the_reference_and_the_host_hand_over(fix, host_runs, name):
    ep = fix["meta"]["episodes"][name]
    _, dev = _sources(ep)
    with BatchedClosedLoop(dict(ep["config"]), [fix[name + "_ped_traj"]], sample_source=dev, device_samples=True,
                           prediction_scores=True) as sim:
        assert sim._native and sim._device_samples
        sim.run()
        got = sim.prediction_metrics()[0]
    print(name, got)
    assert_metrics_match_reference(got, ep["reference"], fix["meta"]["nll_atol"], name)
    # the same kernels on the same numbers: the library's resampler wrote both tensors
    assert got == host_runs[name][0] or all(
        (np.isnan(got[k]) and np.isnan(host_runs[name][0][k])) or got[k] == host_runs[name][0][k] for k in METRIC_KEYS)


def test_a_batch_of_three_equals_the_episodes_alone(fix, host_runs):
    """One sample source has one sample count: the two four-sample episodes (same configuration, different tracks and
    lengths), one of them twice, in one lock step with the samples in HBM -- each equal to its run alone."""
    names = [n for n in AWARE if fix["meta"]["episodes"][n]["n_samples"] == 4]
    assert len(names) == 2
    names = names + names[:1]
    ep = fix["meta"]["episodes"][names[0]]
    _, dev = _sources(ep)
    cfg = dict(ep["config"])
    assert all(fix["meta"]["episodes"][n]["config"] == ep["config"] for n in names)
    with BatchedClosedLoop(cfg, [fix[n + "_ped_traj"] for n in names], sample_source=dev, device_samples=True,
                           prediction_scores=True) as sim:
        sim.run()
        got = sim.prediction_metrics()
    for g, n in zip(got, names):
        w = host_runs[n][0]
        assert all((np.isnan(g[k]) and np.isnan(w[k])) or g[k] == w[k] for k in METRIC_KEYS), (n, g, w)


def test_scoring_does_not_disturb_the_step(fix, host_runs):
    """The per-step records of the loop are identical with and without prediction_scores."""
    name = "weave_s4"
    ep = fix["meta"]["episodes"][name]
    host, dev = _sources(ep)
    with BatchedClosedLoop(dict(ep["config"]), [fix[name + "_ped_traj"]], sample_source=host) as sim:
        assert _steps(sim.run()) == host_runs[name][1]
        with pytest.raises(ValueError, match="prediction_scores=True"):
            sim.prediction_metrics()
    runs = []
    for on in (False, True):
        with BatchedClosedLoop(dict(ep["config"]), [fix[name + "_ped_traj"]], sample_source=dev, device_samples=True,
                               prediction_scores=on) as sim:
            runs.append(_steps(sim.run()))
    assert runs[0] == runs[1]
