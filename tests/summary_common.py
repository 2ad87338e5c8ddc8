"""Episode summary metrics, restated in NumPy for the tests (CPU and GPU): what the reference's
``calculate_aggregate_metrics`` (src/core/metrics.py:272-320) makes of an episode's history, written from the definition
in include/fot.h (fot_loop_summary) over the loop's own ``StepRecord`` objects -- plus fixture access and the comparison
with its tolerances.

The tolerances (none invented here):
* counts, ``steps``, termination: equal;
* ego- and safety-derived keys against the reference fixture: the tolerance ``closed_loop_common.assert_episode_matches``
  applies to the per-step ego state and metrics of these very episodes (rtol = atol = 1e-6, atol x 100 for jerk): a
  minimum, maximum or mean of values that each lie within a tolerance lies within it;
* prediction-error keys against the fixture: a mean of Euclidean distances is 1-Lipschitz in every point, and the
  existing tests hold these episodes' predictions to the reference at atol 1e-12 per coordinate, so atol = sqrt(2) 1e-12;
  plus rtol = 1e-10 for the order of summation (at most ~2e5 non-negative float64 terms: n 2^-53 = 2e-11);
* against this restatement applied to the same loop's own history: only that rtol (sums of the same non-negative terms in
  another order), for the prediction-error keys and for the means; extrema equal.
"""
import json
import math
import os

import numpy as np

from conftest import GOLDEN_DIR

EGO_TOL = 1e-6                                   # assert_episode_matches' tol
PRED_ATOL = math.sqrt(2.0) * 1e-12
SUM_RTOL = 1e-10

INT_KEYS = ("collision_count", "pred_samples", "ade_eval_count", "planning_eval_count", "nll_eval_count")
EXTREMA = ("min_dist", "min_ttc", "max_jerk", "max_accel")
MEANS = ("mean_jerk", "rms_jerk", "mean_accel")
JERK_KEYS = ("max_jerk", "mean_jerk", "rms_jerk")
PRED_KEYS = ("ade", "fde", "ade_per_agent", "fde_per_agent", "planning_ade", "planning_fde", "nll")


def load_summaries():
    """tests/golden/make_closed_loop_summary.py: per variant ``<name>_summary`` (values in meta["keys"] order), for base
    also ``base_summary_60`` / ``_100``; for the weave variants their tracks and configurations."""
    z = np.load(os.path.join(GOLDEN_DIR, "closed_loop", "reference_summary_episodes.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def reference_summary(fix, name, prefix=None):
    """The reference's dictionary for a variant (or for the first ``prefix`` steps of it), counts as ints."""
    v = fix[f"{name}_summary" if prefix is None else f"{name}_summary_{prefix}"]
    keys = fix["meta"]["keys"]
    return {k: (int(x) if k in fix["meta"]["int_keys"] else float(x)) for k, x in zip(keys, v)}


def summary_of_history(hist, dt, sgan_dt, pred_len, num_samples=1):
    """The summary of one episode from its step records (``StepRecord``: ego, metrics, ped_positions,
    predicted_trajectories [P, n_dense, 2] or None)."""
    hist = list(hist)
    L = len(hist)
    absjerk = np.array([abs(r.ego.jerk) for r in hist])
    absacc = np.array([abs(r.ego.a) for r in hist])
    ttc = np.array([r.metrics["ttc"] for r in hist])
    ttc = ttc[(ttc > 0) & np.isfinite(ttc)]
    out = dict(
        min_dist=min(r.metrics["min_distance"] for r in hist) if L else 0.0,
        collision_count=int(sum(bool(r.metrics["collision"]) for r in hist)),
        min_ttc=float(ttc.min()) if len(ttc) else float("inf"),
        max_jerk=float(absjerk.max()) if L else 0.0, mean_jerk=float(absjerk.mean()) if L else 0.0,
        rms_jerk=float(np.sqrt((absjerk ** 2).mean())) if L else 0.0,
        max_accel=float(absacc.max()) if L else 0.0, mean_accel=float(absacc.mean()) if L else 0.0)
    ratio = sgan_dt / dt
    stride = int(round(ratio))
    if stride < 1 or not np.isclose(ratio, stride):
        raise ValueError("sgan_dt must be a multiple of dt")
    horizon = stride * pred_len                                  # steps a standard origin must have ahead of it
    rolling = np.zeros(2)
    standard = np.zeros(2)
    n_rolling = n_standard = 0
    for i, r in enumerate(hist):
        pred = r.predicted_trajectories
        if pred is None or pred.size == 0:
            continue
        P, n_dense, _ = pred.shape
        ahead = L - 1 - i                                        # steps recorded after origin i
        if ahead > 0:
            E = min(n_dense, ahead)
            truth = np.stack([hist[i + 1 + k].ped_positions for k in range(E)], axis=1)      # [P, E, 2]
            diff = pred[:, :E] - truth
            d = np.sqrt(diff[..., 0] ** 2 + diff[..., 1] ** 2)
            rolling += (d.mean(axis=1).sum(), d[:, -1].sum())
            n_rolling += P
        if n_dense >= horizon and ahead >= horizon:
            at = stride * np.arange(1, pred_len + 1)
            truth = np.stack([hist[i + k].ped_positions for k in at], axis=1)                  # [P, pred_len, 2]
            diff = pred[:, at - 1] - truth
            d = np.sqrt(diff[..., 0] ** 2 + diff[..., 1] ** 2)
            standard += (d.mean() * P, d[:, -1].mean() * P)
            n_standard += P
    nan = float("nan")
    ade, fde = (standard / n_standard) if n_standard else (nan, nan)
    p_ade, p_fde = (rolling / n_rolling) if n_rolling else (nan, nan)
    out.update(ade=float(ade), fde=float(fde), ade_per_agent=float(ade), fde_per_agent=float(fde),
               pred_samples=int(num_samples) if n_standard else 0, ade_eval_count=int(n_standard),
               planning_ade=float(p_ade), planning_fde=float(p_fde), planning_eval_count=int(n_rolling),
               nll=nan, nll_eval_count=0)
    return out


def _close(got, want, rtol, atol, what):
    if math.isnan(want) or math.isinf(want):
        assert (math.isnan(got) and math.isnan(want)) or got == want, f"{what}: {got!r}, expected {want!r}"
    else:
        assert abs(got - want) <= atol + rtol * abs(want), f"{what}: {got!r}, expected {want!r} (diff {got - want:.3e})"


def assert_summary_matches_reference(got, want, label):
    """``got``: a dictionary of aggregate_metrics() / summary_of_history(); ``want``: reference_summary()."""
    for k in INT_KEYS:
        assert isinstance(got[k], int) and got[k] == want[k], f"{label} {k}: {got[k]!r}, reference {want[k]!r}"
    for k in EXTREMA + MEANS:
        _close(got[k], want[k], EGO_TOL, EGO_TOL * (100 if k in JERK_KEYS else 1), f"{label} {k}")
    for k in PRED_KEYS:
        _close(got[k], want[k], SUM_RTOL, PRED_ATOL, f"{label} {k}")


def assert_summary_matches_own_history(got, own, label):
    """``got``: the device's summary; ``own``: summary_of_history() of the same loop's records."""
    for k in INT_KEYS:
        assert isinstance(got[k], int) and got[k] == own[k], f"{label} {k}: {got[k]!r}, own history {own[k]!r}"
    for k in EXTREMA:
        assert got[k] == own[k], f"{label} {k}: {got[k]!r}, own history {own[k]!r}"
    for k in MEANS + PRED_KEYS:
        _close(got[k], own[k], SUM_RTOL, 0.0, f"{label} {k}")
