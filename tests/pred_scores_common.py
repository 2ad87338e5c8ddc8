"""Prediction scores restated in NumPy for the tests (CPU and GPU): what one prediction origin contributes to the
reference's ``_standard_ade_fde_details`` / ``_kde_nll_details`` (src/core/metrics.py:31-176), written from the definition
in include/fot.h (fot_pred_score), and the deferred fold of an episode's records -- plus fixture access, a writer of the
emulation program's case files and the comparisons with their tolerances.

The tolerances (none invented here):
* float64 tensors against the reference fixture: ``summary_common``'s rule -- rtol = SUM_RTOL (1e-10, the order of
  summation) plus atol = PRED_ATOL (sqrt(2) 1e-12, the predictions' own distance from the reference's: every
  displacement term is 1-Lipschitz in each point); for ``nll`` the absolute term is PRED_ATOL times the largest
  |d log p / d q| present in the fixture, max |q - g| / b^2 over the un-floored entries, which the generator computes
  and stores (meta["nll_atol"]);
* the kernel against this restatement on identical inputs, and against the emulation program: rtol = SUM_RTOL alone
  (exp / log / sqrt of the device against libm: a few ulp on terms of magnitude <= 20);
* counts and flags: equal.
"""
import json
import os
import struct

import numpy as np

from conftest import GOLDEN_DIR
from summary_common import PRED_ATOL, SUM_RTOL

BANDWIDTH_FLOOR = 0.05
LOG_P_FLOOR = -20.0
FLAG_NLL, FLAG_NONFINITE = 1, 2
F64_FIELDS = ("ade_scene", "fde_scene", "ade_agent_sum", "fde_agent_sum", "log_lik_sum")
I32_FIELDS = ("n_peds", "n_samples", "nll_count", "flags")
RECORD_DT = np.dtype([(n, "f8") for n in F64_FIELDS] + [(n, "i4") for n in I32_FIELDS])
METRIC_KEYS = ("ade", "fde", "ade_per_agent", "fde_per_agent", "pred_samples", "ade_eval_count", "nll", "nll_eval_count")
FIXTURE = os.path.join(GOLDEN_DIR, "prediction_scores", "cases.npz")


def load_cases():
    """tests/golden/make_prediction_scores.py: meta["units"] / meta["episodes"] and their arrays."""
    z = np.load(FIXTURE, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def log_p_terms(samples, truth):
    """Per (p, j): the un-floored log p and the bandwidths.  samples [S, P, E, 2] at the evaluation indices."""
    S = samples.shape[0]
    scott = S ** (-1.0 / 6.0)
    mean = samples.mean(axis=0)
    std = np.sqrt(((samples - mean[None]) ** 2).sum(axis=0) / (S - 1))           # two passes, ddof = 1
    bw = np.maximum(std * scott, BANDWIDTH_FLOOR)
    u = (samples - truth[None]) / bw[None]
    l = -0.5 * (u ** 2).sum(axis=3) - np.log(2.0 * np.pi * bw[..., 0] * bw[..., 1])[None]
    peak = l.max(axis=0)
    return peak + np.log(np.exp(l - peak[None]).mean(axis=0)), bw


def origin_terms(dense, truth, stride):
    """One origin's record.  dense [S, P, n_dense, 2] (no prepended entry), truth [P, E, 2]."""
    dense, truth = np.asarray(dense, np.float64), np.asarray(truth, np.float64)
    S, P = dense.shape[0], dense.shape[1]
    E = truth.shape[1]
    r = np.zeros((), RECORD_DT)
    r["n_samples"] = S
    if P == 0:
        return r
    idx = stride * np.arange(1, E + 1) - 1
    q = dense[:, :, idx, :]
    d = np.sqrt(((q - truth[None]) ** 2).sum(axis=3))                             # [S, P, E]
    with np.errstate(invalid="ignore"):
        r["ade_scene"] = np.min(d.sum(axis=2).sum(axis=1) / (P * E))
        r["fde_scene"] = np.min(d[:, :, -1].sum(axis=1) / P)
        r["ade_agent_sum"] = np.sum(np.min(d.sum(axis=2) / E, axis=0))
        r["fde_agent_sum"] = np.sum(np.min(d[:, :, -1], axis=0))
    r["n_peds"] = P
    flags = 0 if np.isfinite(q).all() and np.isfinite(truth).all() else FLAG_NONFINITE
    if S >= 2 and np.any(np.ptp(q, axis=0) > 0):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            lp, _ = log_p_terms(q, truth)
            r["log_lik_sum"] = np.maximum(lp, LOG_P_FLOOR).sum()
        r["nll_count"] = P * E
        flags |= FLAG_NLL
    r["flags"] = flags
    return r


def fold(records, L, stride, E):
    """``records``: (step index i, record) of one episode in step order; L: the episode's steps.  The reference's fold
    (metrics.py:96-113, 171-176): an origin counts if i + stride E < L."""
    tot = [0.0] * 5
    count = nll_count = samples = 0
    for i, r in records:
        if r["n_peds"] <= 0 or i + stride * E >= L:
            continue
        P = int(r["n_peds"])
        tot[0] += float(r["ade_scene"]) * P
        tot[1] += float(r["fde_scene"]) * P
        tot[2] += float(r["ade_agent_sum"])
        tot[3] += float(r["fde_agent_sum"])
        count += P
        samples = max(samples, int(r["n_samples"]))
        if r["flags"] & FLAG_NLL:
            tot[4] += float(r["log_lik_sum"])
            nll_count += int(r["nll_count"])
    nan = float("nan")
    m = [t / count for t in tot[:4]] if count else [nan] * 4
    return dict(ade=m[0], fde=m[1], ade_per_agent=m[2], fde_per_agent=m[3], pred_samples=samples if count else 0,
                ade_eval_count=count, nll=-tot[4] / nll_count if nll_count else nan, nll_eval_count=nll_count)


def unit_case(fix, name):
    """(dense [S, P, T, 2], truth [P, E, 2], stride, the reference's answers) of a unit origin."""
    u = fix["meta"]["units"][name]
    return fix[f"u_{name}_dense"], fix[f"u_{name}_truth"], int(u["stride"]), u["reference"]


def unit_metrics(rec, name=""):
    """The reference's per-history answers from ONE eligible origin's record."""
    return fold([(0, rec)], 10 ** 9, 0, 0)


def _close(got, want, rtol, atol, what):
    if np.isnan(want) or np.isinf(want):
        assert (np.isnan(got) and np.isnan(want)) or got == want, f"{what}: {got!r}, expected {want!r}"
    else:
        assert abs(got - want) <= atol + rtol * abs(want), f"{what}: {got!r}, expected {want!r} (diff {got - want:.3e})"


def assert_metrics_match_reference(got, want, nll_atol, label):
    for k in ("pred_samples", "ade_eval_count", "nll_eval_count"):
        assert int(got[k]) == int(want[k]), f"{label} {k}: {got[k]!r}, reference {want[k]!r}"
    for k in ("ade", "fde", "ade_per_agent", "fde_per_agent"):
        _close(float(got[k]), float(want[k]), SUM_RTOL, PRED_ATOL, f"{label} {k}")
    _close(float(got["nll"]), float(want["nll"]), SUM_RTOL, nll_atol, f"{label} nll")


def assert_records_close(got, want, label, rtol=SUM_RTOL):
    """Two records of the same inputs: counts and flags equal, the float64 terms within rtol."""
    for k in I32_FIELDS:
        assert int(got[k]) == int(want[k]), f"{label} {k}: {int(got[k])}, expected {int(want[k])}"
    for k in F64_FIELDS:
        _close(float(got[k]), float(want[k]), rtol, 0.0, f"{label} {k}")


def layouts(dense, t_major, skip, dtype, rng=None):
    """The origin's block as the library reads it: [S, P, T + skip, 2] or [T + skip, S, P, 2], the skipped entry poisoned."""
    S, P, T, _ = dense.shape
    blk = np.empty((S, P, T + skip, 2), dtype)
    blk[:, :, skip:] = dense
    if skip:
        blk[:, :, 0] = np.nan
    return np.ascontiguousarray(blk.transpose(2, 0, 1, 3)) if t_major else blk


def write_emu_cases(path, cases):
    """cases: (block, truth, stride, t_major, skip) with block as ``layouts`` returns it."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for blk, truth, stride, t_major, skip in cases:
            S, P, T = (blk.shape[1], blk.shape[2], blk.shape[0]) if t_major else blk.shape[:3]
            f.write(struct.pack("<8i", S, P, T, stride, truth.shape[1], int(t_major), int(skip),
                                0 if blk.dtype == np.float32 else 1))
            f.write(np.ascontiguousarray(blk).tobytes())
            f.write(np.ascontiguousarray(truth, np.float64).tobytes())


def random_origin(rng, S=None, P=None, E=None, stride=None):
    S = int(rng.integers(1, 65)) if S is None else S
    P = int(rng.integers(1, 40)) if P is None else P
    E = int(rng.integers(1, 13)) if E is None else E
    stride = int(rng.integers(1, 5)) if stride is None else stride
    T = stride * E + int(rng.integers(0, 4))
    centre = rng.uniform(-60.0, 60.0, (1, P, 1, 2)) + np.cumsum(rng.normal(0, 0.2, (1, P, T, 2)), axis=2)
    spread = 10.0 ** rng.uniform(-3.0, 0.0)
    dense = centre + rng.normal(0.0, spread, (S, P, T, 2))
    if rng.random() < 0.15:
        dense[:] = dense[:1]                                              # identical samples
    truth = centre[0][:, stride * np.arange(1, E + 1) - 1] + rng.normal(0.0, 10.0 ** rng.uniform(-2.0, 0.7), (P, E, 2))
    return dense, truth, stride
