"""Sample distributions of more than 64 samples in the closed loop, the samplers and the scores (a handle whose sample
capacity was raised), the part that needs no GPU: the Python loop and the oracle against reference episodes of 100 and 130
samples (tests/golden/closed_loop/reference_wide_episodes.npz); the constructors' capacity keyword; and the sum order of
the wide score and selection kernels, restated from the shared headers by tests/emu/fot_wide_loop_emu.cpp, against
NumPy."""
import os
import subprocess

import numpy as np
import pytest

from closed_loop_common import OracleEngine, OracleResampler, assert_episode_matches
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.prediction import RecordedSamples, SganSampler, SganWeights
from pred_scores_common import RECORD_DT, assert_records_close, layouts, origin_terms, random_origin, write_emu_cases
from summary_common import SUM_RTOL
from wide_loop_common import FIXTURE, load_wide_episodes, predict_single_best, tie_block, wide_sample_source

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_EXE = os.path.join(EMU_DIR, "_build", "fot_wide_loop_emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
VARIANTS = ("s100_eps01", "s130_eps0")


# ---- the reference episodes ---------------------------------------------------------------------------------------------------
def test_fixture_holds_what_the_tests_need():
    ep = load_wide_episodes()
    meta = ep["meta"]["variants"]
    assert tuple(meta) == VARIANTS
    assert meta["s100_eps01"]["n_samples"] == 100 and meta["s100_eps01"]["chance_epsilon"] == 0.01
    assert int(0.01 * 100) == 1                                       # the budget: exactly one sample
    assert meta["s130_eps0"]["n_samples"] == 130 and meta["s130_eps0"]["chance_epsilon"] == 0.0
    for name in VARIANTS:
        assert meta[name]["n_samples"] > _abi.MAX_SAMPLES
        assert (ep[name + "_metrics"][:, 5] > 0).any(), f"{name}: no step with n_collision_rejected > 0"
        assert (np.diff(ep[name + "_state"]) > 0).any(), f"{name}: no state escalation"
    assert meta["s100_eps01"]["budget_decided_calls"] > 0             # the one sample changed a selected path
    assert os.path.getsize(FIXTURE) < 850_000


@pytest.mark.parametrize("name", VARIANTS)
def test_wide_distribution_episodes_free_running(name):
    """The five-call loop on the oracle-backed stand-ins, every plan() call checked against all 100 / 130 samples under
    the chance constraint: the Python loop and the oracle at S > 64, before any GPU is involved."""
    ep = load_wide_episodes()
    var = ep["meta"]["variants"][name]
    cfg = dict(var["config"])
    src = wide_sample_source(var["n_samples"], cfg["pred_len"])
    sim = BatchedClosedLoop(cfg, [ep[name + "_ped_traj"]], engine=OracleEngine(cfg), resampler=OracleResampler(cfg),
                            sample_source=src)
    hist = sim.run()[0]
    assert_episode_matches(hist, sim.episodes[0].termination_reason, ep, name)


# ---- the constructors -----------------------------------------------------------------------------------------------------------
def _weights():
    return SganWeights.__new__(SganWeights)                           # (the sample-count check comes before the weights are read)


@pytest.mark.parametrize("S", [65, 254])
def test_constructors_accept_more_samples_with_the_keyword(S):
    rec = RecordedSamples(np.zeros((2, S, 3, 4, 2), np.float32), sample_capacity=S)
    assert rec.num_samples == S and rec.sample_capacity == S
    rec = RecordedSamples(np.zeros((1, S, 3, 4, 2)), sample_capacity=_abi.MAX_PLAN_SAMPLES)
    assert rec.num_samples == S
    w = _weights()
    w.noise_type = "gaussian"
    smp = SganSampler(None, w, S, counter_seed=3, sample_capacity=S)
    assert smp.num_samples == S and smp.sample_capacity == S


def test_constructors_refuse_what_lies_above_the_capacity():
    w = _weights()
    w.noise_type = "gaussian"
    with pytest.raises(ValueError, match="S <= 64"):                    # the default, word for word
        RecordedSamples(np.zeros((1, 65, 3, 4, 2), np.float32))
    with pytest.raises(ValueError, match="num_samples <= 64"):
        SganSampler(None, w, 65, counter_seed=3)
    with pytest.raises(ValueError, match="S <= 254"):
        RecordedSamples(np.zeros((1, 255, 3, 4, 2), np.float32), sample_capacity=254)
    with pytest.raises(ValueError, match="num_samples <= 254"):
        SganSampler(None, w, 255, counter_seed=3, sample_capacity=254)
    with pytest.raises(ValueError, match="S <= 128"):                   # the keyword's own value, not the library's maximum
        RecordedSamples(np.zeros((1, 129, 3, 4, 2), np.float32), sample_capacity=128)
    for bad in (63, 255):
        with pytest.raises(ValueError, match="sample_capacity"):
            RecordedSamples(np.zeros((1, 4, 3, 4, 2), np.float32), sample_capacity=bad)
        with pytest.raises(ValueError, match="sample_capacity"):
            SganSampler(None, w, 4, counter_seed=3, sample_capacity=bad)


def test_loop_refuses_a_source_wider_than_its_capacity_at_construction():
    ep = load_wide_episodes()
    cfg = dict(ep["meta"]["variants"]["s100_eps01"]["config"])
    tracks = ep["s100_eps01_ped_traj"]
    rec = RecordedSamples(np.zeros((3, 100, cfg["pred_len"], tracks.shape[1], 2), np.float32), sample_capacity=100)
    kw = dict(engine=OracleEngine(cfg), resampler=OracleResampler(cfg))
    with pytest.raises(ValueError, match="sample_capacity"):            # the loop's default capacity: 64
        BatchedClosedLoop(cfg, [tracks], sample_source=rec, **kw)
    with pytest.raises(ValueError, match="sample_capacity"):
        BatchedClosedLoop(cfg, [tracks], sample_source=rec, sample_capacity=99, **kw)
    with pytest.raises(ValueError, match="sample_capacity"):            # not a capacity at all
        BatchedClosedLoop(cfg, [tracks], sample_source=rec, sample_capacity=255, **kw)
    sim = BatchedClosedLoop(cfg, [tracks], sample_source=rec, sample_capacity=100, **kw)
    assert sim.sample_source is rec
    # a caller's engine: its own capacity counts, whatever the keyword says
    eng = OracleEngine(cfg)
    eng.sample_capacity = 64
    with pytest.raises(ValueError, match="sample_capacity"):
        BatchedClosedLoop(cfg, [tracks], sample_source=rec, sample_capacity=254, engine=eng, resampler=OracleResampler(cfg))
    eng.sample_capacity = 128
    BatchedClosedLoop(cfg, [tracks], sample_source=rec, engine=eng, resampler=OracleResampler(cfg))


# ---- the kernels' sum order ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    srcs = [os.path.join(EMU_DIR, "fot_wide_loop_emu.cpp"), os.path.join(CSRC, "fot_loopscore.hpp"),
            os.path.join(CSRC, "fot_predscore.hpp")]
    if not os.path.exists(EMU_EXE) or os.path.getmtime(EMU_EXE) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(EMU_EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EMU_EXE, srcs[0]], check=True)

    def run(cases, tmp_path):
        """cases: (dense [S, P, T, 2], truth [P, E, 2], stride) -> (records, [(best, dev [S])]) in the kernels' layout: the
        current position in front of the dense entries, skipped."""
        src, rec, best = (str(tmp_path / n) for n in ("cases.bin", "records.bin", "best.bin"))
        write_emu_cases(src, [(layouts(d, False, 1, np.float64), t, stride, False, 1) for d, t, stride in cases])
        subprocess.run([EMU_EXE, src, rec, best], check=True, timeout=120)
        records = np.fromfile(rec, dtype=RECORD_DT)
        assert len(records) == len(cases)
        raw = np.fromfile(best, dtype=np.uint8)
        chosen, at = [], 0
        for d, _, _ in cases:
            b, S = (int(v) for v in raw[at:at + 8].view(np.int32))
            assert S == d.shape[0]
            chosen.append((b, raw[at + 8:at + 8 + 8 * S].view(np.float64).copy()))
            at += 8 + 8 * S
        assert at == len(raw)
        return records, chosen
    return run


def test_wide_sum_orders_equal_the_numpy_restatements(emu, tmp_path):
    """S on both sides of two and of three mask words and at the top, P of one lane, a few and past a wave: the records
    within SUM_RTOL of origin_terms (the project's rule for another summation order), the chosen sample equal to
    predict_single_best's."""
    rng = np.random.default_rng(34)
    cases = []
    for S in (65, 128, 129, 254):
        for P in (1, 5, 65):
            cases.append(random_origin(rng, S=S, P=P, E=int(rng.integers(1, 13)), stride=int(rng.integers(1, 5))))
    cases.append(random_origin(rng, S=254, P=270, E=1, stride=1))     # more pedestrians than lanes: a second pass
    cases.append(random_origin(rng, S=200, P=90, E=12, stride=1))     # more (p, j) pairs than a tile holds
    records, chosen = emu(cases, tmp_path)
    compared = len(cases)
    for (dense, truth, stride), rec, (best, dev) in zip(cases, records, chosen):
        label = f"S {dense.shape[0]} P {dense.shape[1]} E {truth.shape[1]}"
        assert_records_close(rec, origin_terms(dense, truth, stride), label)
        want_best, want_dev = predict_single_best(dense, skip=0)
        np.testing.assert_allclose(dev, want_dev, rtol=SUM_RTOL, err_msg=label)
        if np.ptp(dense, axis=0).max() == 0.0:                        # (random_origin's identical samples: every sum is the
            compared -= 1                                             #  rounding of the mean, the choice among them open)
            continue
        two = np.sort(want_dev)[:2]
        assert two[1] - two[0] > 1e-9 * two[1], f"{label}: two minima within 1e-9 (another seed)"
        assert best == want_best, label
    assert compared >= 10                                             # every S among them still (the seed decides)


def test_wide_selection_exact_tie_across_the_first_mask_word(emu, tmp_path):
    """Samples 63 and 64 are the same numbers: their sums are the same operations on the same values, an exact tie at the
    minimum; the first wins.  Once more with the tie at 64 / 253 and the pair of sample 0 and the last."""
    rng = np.random.default_rng(35)
    truth = np.zeros((5, 2, 2))
    cases = [(tie_block(rng, 130, 5, 9, 63, 64), truth, 1), (tie_block(rng, 254, 5, 9, 64, 253), truth, 1),
             (tie_block(rng, 254, 5, 9, 0, 253), truth, 1)]
    _, chosen = emu(cases, tmp_path)
    for (blk, _, _), (best, dev), (a, b) in zip(cases, chosen, ((63, 64), (64, 253), (0, 253))):
        want_best, want_dev = predict_single_best(blk, skip=0)
        assert dev[a] == dev[b] and want_dev[a] == want_dev[b]
        assert dev[a] < np.delete(dev, [a, b]).min()
        assert best == a == want_best
