"""Prediction scores and episode summaries of a resident sampler loop (fot_loop_scores_enable, fot_loop_score_summaries,
fot_loop_last_best_sample), the part that needs no GPU: the C ABI's symbols; the per-slot ring fold and the
representative-sample rule of csrc/fot_loopscore.hpp -- the code the host and k_loop_best_sample run -- against direct
evaluations of the reference's rules; and the messages of the Python refusals that stay."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from closed_loop_common import OracleEngine, OracleResampler, load_episodes, scenario_config
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SHIM_SO = os.path.join(EMU_DIR, "_build", "libfot_loopscore_emu.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
ENTRIES = ("fot_loop_scores_enable", "fot_loop_score_summaries", "fot_loop_last_best_sample")
REC_DT = np.dtype(_abi.PredScore)


def test_library_exports_the_score_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for sym in ENTRIES:
        assert hasattr(lib, sym), f"{sym} not exported by libfot.so"
        assert sym in _abi.SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} not declared in include/fot.h"
    assert _abi.ABI_VERSION == 8                                    # additions only: the version and the words stay


@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(EMU_DIR, "fot_loopscore_emu.cpp"), os.path.join(CSRC, "fot_loopscore.hpp"),
            os.path.join(CSRC, "fot_predscore.hpp")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        # (no contraction of a * b + c: the fold rounds its products as NumPy does)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", SHIM_SO, srcs[0]], check=True)
    L = C.CDLL(SHIM_SO)
    vp = C.c_void_p
    L.best_sample_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.first_min_of.argtypes = [C.c_int, vp]
    L.score_ring_run.argtypes = [C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]
    return L


# ---- the fold ----------------------------------------------------------------------------------------------------------------
def _direct(recs, l, H):
    """BatchedClosedLoop.prediction_metrics over the first l records of one slot: the reference's rule i + H < l."""
    tot = [0.0] * 5
    count = nll_count = samples = 0
    for i in range(l):
        r = recs[i]
        if r["n_peds"] <= 0 or i + H >= l:
            continue
        tot[0] += float(r["ade_scene"]) * int(r["n_peds"])
        tot[1] += float(r["fde_scene"]) * int(r["n_peds"])
        tot[2] += float(r["ade_agent_sum"])
        tot[3] += float(r["fde_agent_sum"])
        count += int(r["n_peds"])
        samples = max(samples, int(r["n_samples"]))
        if r["flags"] & _abi.PRED_NLL:
            tot[4] += float(r["log_lik_sum"])
            nll_count += int(r["nll_count"])
    nan = float("nan")
    m = [v / count for v in tot[:4]] if count else [nan] * 4
    return m + [-tot[4] / nll_count if nll_count else nan, float(count), float(nll_count), float(samples if count else 0)]


def _records(rng, n, S):
    r = np.zeros(n, REC_DT)
    r["n_peds"] = rng.integers(1, 40, n)
    r["n_peds"][rng.random(n) < 0.2] = 0                            # steps without a prediction / slots without pedestrians
    for k in ("ade_scene", "fde_scene", "ade_agent_sum", "fde_agent_sum"):
        r[k] = rng.uniform(0.0, 7.0, n)
    r["log_lik_sum"] = rng.uniform(-400.0, 30.0, n)
    r["n_samples"] = S
    nll = (rng.random(n) < 0.7) & (r["n_peds"] > 0) & (S >= 2)      # records without FOT_PRED_NLL among them
    r["flags"] = np.where(nll, _abi.PRED_NLL, 0) | np.where(rng.random(n) < 0.1, _abi.PRED_NONFINITE, 0)
    r["nll_count"] = np.where(nll, r["n_peds"] * 3, 0)
    zero = r["n_peds"] == 0
    for k in ("ade_scene", "fde_scene", "ade_agent_sum", "fde_agent_sum", "log_lik_sum"):
        r[k][zero] = 0.0
    return r


def test_ring_fold_equals_the_reference_rule(shim):
    """Slots of different lengths in lock step (a slot stops, the others go on), summaries taken mid-run and the run
    continued, runs that end before H steps, records without pedestrians and without the KDE: the ring's totals equal the
    direct evaluation exactly -- both add the same rounded terms in the same order."""
    rng = np.random.default_rng(77)
    cases = [(48, (274, 9, 48, 49, 120), 20), (1, (5, 0, 1), 1), (4, (3, 4, 5, 30), 4), (12, (11, 12, 13, 64), 64)]
    for _ in range(30):
        H = int(rng.integers(1, 20))
        cases.append((H, tuple(int(v) for v in rng.integers(0, 4 * H + 3, int(rng.integers(1, 6)))), int(rng.integers(1, 9))))
    counted = early = stopped = no_nll = 0
    for H, lengths, S in cases:
        n, L_max = len(lengths), max(max(lengths), 1)
        recs = np.stack([_records(rng, L_max, S) for _ in range(n)])
        L = np.array(lengths, np.int32)
        at = np.unique(np.concatenate([[0, L_max], rng.integers(0, L_max + 1, 6)])).astype(np.int32)
        out = np.zeros((len(at), n, 8))
        assert shim.score_ring_run(H, n, L.ctypes.data, L_max, recs.ctypes.data, len(at), at.ctypes.data, out.ctypes.data) == len(at)
        for j, a in enumerate(at):
            for e in range(n):
                l = min(int(a), int(L[e]))
                want = _direct(recs[e], l, H)
                np.testing.assert_array_equal(out[j, e], want, err_msg=f"H {H} lengths {lengths} slot {e} after {a} lock steps")
                counted += want[5] > 0
                early += 0 < l <= H and want[5] == 0 and np.isnan(want[0]) and want[7] == 0
                stopped += int(L[e]) < a and want[5] > 0
                no_nll += want[5] > 0 and want[6] < want[5] * 3
    assert counted > 50 and early > 20 and stopped > 10 and no_nll > 10


def test_fold_rounds_the_product_before_it_adds(shim):
    """ade_scene * n_peds is a float64 of its own (NumPy's product), not the inner term of a fused multiply-add: values
    whose product needs more than 53 bits."""
    H, n = 1, 40
    rng = np.random.default_rng(5)
    recs = np.zeros((1, n), REC_DT)
    recs["n_peds"] = rng.integers(3, 255, n) | 1
    recs["ade_scene"] = rng.uniform(0.1, 1.0, n)
    recs["fde_scene"] = rng.uniform(0.1, 1.0, n)
    recs["n_samples"] = 2
    L, at = np.array([n], np.int32), np.array([n], np.int32)
    out = np.zeros((1, 1, 8))
    assert shim.score_ring_run(H, 1, L.ctypes.data, n, recs.ctypes.data, 1, at.ctypes.data, out.ctypes.data) == 1
    np.testing.assert_array_equal(out[0, 0], _direct(recs[0], n, H))


# ---- the representative sample --------------------------------------------------------------------------------------------------
def _reference_dev(blk, skip):
    """predict_single_best (trajectory_predictor.py:346-351) on [S, P, T, 2], the prepended entries left out."""
    q = blk[:, :, skip:]
    return np.linalg.norm(q - q.mean(axis=0)[None], axis=-1).sum(axis=(1, 2))


def _choose(shim, blk, skip):
    S, P, T, _ = blk.shape
    blk = np.ascontiguousarray(blk)
    dev = np.zeros(S)
    return shim.best_sample_run(S, P, T, skip, blk.ctypes.data, dev.ctypes.data), dev


def test_best_sample_is_the_first_minimum_of_the_reference_s_formula(shim):
    # (S >= 3: two samples lie symmetrically about their mean, so their sums are equal but for rounding)
    rng = np.random.default_rng(31)
    left_out = n = 0
    for S, P, T, skip in [(3, 1, 2, 1), (4, 3, 51, 1), (20, 30, 51, 1), (64, 7, 13, 0), (5, 65, 9, 1), (3, 256, 6, 1)] + \
            [(int(rng.integers(3, 33)), int(rng.integers(1, 40)), int(rng.integers(2, 30)), int(rng.integers(0, 2))) for _ in range(40)]:
        blk = rng.normal(0.0, 1.0, (S, P, T, 2)) * rng.uniform(0.01, 3.0) + rng.uniform(-40.0, 40.0, (1, P, 1, 2))
        best, dev = _choose(shim, blk, skip)
        want = _reference_dev(blk, skip)
        np.testing.assert_allclose(dev, want, rtol=1e-12)           # (another order of at most 256 x 50 non-negative terms)
        two = np.sort(want)[:2]
        n += 1
        if two[1] - two[0] < 1e-9 * two[1]:
            left_out += 1
            continue
        assert best == int(np.argmin(want)), (S, P, T, skip)
    assert left_out == 0, f"{left_out} of {n} blocks had two minima within 1e-9"


def test_best_sample_exact_tie_and_single_sample(shim):
    rng = np.random.default_rng(32)
    # samples 1 and 3 are the same numbers (their sums are the same operations on the same values: an exact tie), samples 0
    # and 2 lie symmetrically far off: the tie is the minimum and the FIRST of the two is chosen
    base = rng.normal(0.0, 1.0, (7, 12, 2)) + 20.0
    off = rng.uniform(1.0, 2.0, (7, 12, 2))
    blk = np.stack([base + off, base, base - off, base])
    best, dev = _choose(shim, blk, 1)
    want = _reference_dev(blk, 1)
    assert dev[1] == dev[3] and want[1] == want[3] and dev[1] < min(dev[0], dev[2])
    assert best == 1 == int(np.argmin(want))
    best, dev = _choose(shim, np.stack([base + off, base - off, base, base]), 1)
    assert best == 2 and dev[2] == dev[3]
    # S = 1: sample 0, whatever it holds
    best, dev = _choose(shim, base[None], 1)
    assert best == 0 and dev[0] == 0.0
    # the rule on the sums alone: np.argmin, ties and NaN included
    for v in ([3.0, 1.0, 1.0, 2.0], [1.0], [2.0, float("nan"), 1.0, float("nan")], [float("nan"), 0.0], [5.0, 4.0, 3.0, 3.0],
              [float("inf"), float("inf")]):
        a = np.array(v)
        assert shim.first_min_of(len(a), a.ctypes.data) == int(np.argmin(a)), v


# ---- the Python refusals that stay ------------------------------------------------------------------------------------------------
def _counter_source():
    """What BatchedClosedLoop takes for a resident loop's own sampler, as far as its argument checks look."""
    return types.SimpleNamespace(counter_seed=1, bind=lambda engine: None, engine=None, num_samples=4)


def test_python_refusals_keep_their_messages():
    with pytest.raises(ValueError, match="resident=False"):         # resident, but no resident sampler
        BatchedClosedLoop({}, [], prediction_scores=True, resident=True)
    with pytest.raises(ValueError, match="resident=False"):         # ... a sample source that is not counter-seeded
        BatchedClosedLoop({}, [], prediction_scores=True, resident=True, sample_source=lambda a, b: None, device_samples=True)
    with pytest.raises(ValueError, match="resident=False"):         # ... not through device memory
        BatchedClosedLoop({}, [], prediction_scores=True, resident=True, sample_source=_counter_source())
    with pytest.raises(ValueError, match="summaries=True with a sampler"):
        BatchedClosedLoop({}, [], sample_source=_counter_source(), device_samples=True, resident=True, summaries=True)
    with pytest.raises(ValueError, match="summaries=True with a sampler"):      # scores do not lift it
        BatchedClosedLoop({}, [], sample_source=_counter_source(), device_samples=True, resident=True, summaries=True,
                          prediction_scores=True)
    with pytest.raises(ValueError, match="resident=True"):
        BatchedClosedLoop({}, [], summaries=True)
    episodes = load_episodes()
    cfg = scenario_config(episodes["meta"], "base")
    sim = BatchedClosedLoop(cfg, [episodes["base_ped_traj"]], engine=OracleEngine(cfg), resampler=OracleResampler(cfg))
    with pytest.raises(ValueError, match="prediction_scores=True"):
        sim.prediction_metrics()
    with pytest.raises(ValueError, match="summaries=True"):
        sim.aggregate_metrics()
