#!/usr/bin/env python3
"""Encounter-fidelity answers of the REFERENCE (build container only) -- data only.

Encounters -- the inputs of the reference's own tests/test_fidelity_metrics.py, written out here, and seeded random ones
(tests/fidelity_common.py: T from 2 to 70, N from 0 to 12, dt in {0.4, 0.1, 1 / 23.98}) -- go through the reference's own
functions:
  * ``min_separation_series`` and ``avoidance_onset_distance`` (src/core/metrics.py), the latter with the velocity
    differenced from the positions and with the stored velocity;
  * ``compare_distributions_ks`` on the samples of the reference's tests, on tied samples and on samples emptied by the
    filter; ``calculate_min_separation`` on a two-step history;
  * ``_per_encounter_onset``, ``objective_rollout_ade`` (with and without ``interaction_distance``) and ``fidelity_report``
    (src/simulation/calibration_harness.py) with ``simulate_encounter`` patched to hand back the supplied roll-out: the
    Social-Force roll-out itself is not part of what is measured.
``loguru`` and ``pysocialforce`` are stubbed.  No reference code is stored.

``avoidance_onset_distance`` returns the distances of the pedestrians that evade and nothing else.  The step and the
``away`` value of every onset are formed here with the reference's own NumPy calls (np.gradient, the 1-D np.linalg.norm,
np.dot) and its rule, one pedestrian at a time, and the generator asserts that the distances so found are, bit for bit
and in order, what the reference's function returned.

The generator also asserts (a condition, not a measurement) that no pedestrian of a random encounter comes within the
band 1e-9 (relative) of ``accel_threshold`` or ``max_distance`` at any step up to its onset.
"""
import argparse
import json
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root
sys.path.insert(0, HERE)
import fidelity_common as fc  # noqa: E402
from make_prediction_scores import save_npz  # noqa: E402

N_RANDOM = 40
INTERACTION = 3.0


def load_reference(ref):
    lg = types.ModuleType("loguru")

    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None

    lg.logger = _Logger()
    sys.modules["loguru"] = lg
    sys.modules.setdefault("pysocialforce", types.ModuleType("pysocialforce"))
    sys.path.insert(0, ref)
    os.chdir(ref)
    from src.core import metrics
    from src.simulation import calibration_harness as harness
    return metrics, harness


def onsets_by_the_rule(ego, ped, vel, dt, thr, max_d):
    """(step [N], distance [N], away [N], closest approach to a threshold): per pedestrian, every step's distance and
    `away` at once -- through the NumPy calls the reference makes per (step, pedestrian) pair, the 1-D norm and np.dot of
    two-vectors, so that the bits are its bits -- then a first-hit search among the steps in range."""
    T, N, _ = ped.shape
    step, where, away_at, margin = np.full(N, -1, np.int32), np.full(N, np.nan), np.full(N, np.nan), np.inf
    if min(T - 1, N) < 1:
        return step, where, away_at, margin
    acc = np.gradient(np.gradient(ped, dt, axis=0) if vel is None else vel, dt, axis=0)
    for j in range(N):
        offset = ped[:, j] - ego                                                      # [T, 2]
        dist = np.array([float(np.linalg.norm(row)) for row in offset])
        usable = ~((dist < 1e-9) | (dist > max_d))
        away = np.full(T, np.nan)
        away[usable] = [float(np.dot(acc[t, j], offset[t] / dist[t])) for t in np.flatnonzero(usable)]
        hits = np.flatnonzero(usable & (away > thr))
        last = hits[0] if hits.size else T - 1                                      # (the reference looks no further)
        seen = np.arange(T) <= last
        margin = min(margin, float(np.min(np.abs(dist[seen] - max_d) / max_d)),
                     float(np.min(np.abs(away[seen & usable] - thr) / thr, initial=np.inf)))
        if hits.size:
            step[j], where[j], away_at[j] = last, dist[last], away[last]
    return step, where, away_at, margin


def reference_encounters():
    """the encounters of the reference's tests, written out: separation of two pedestrians, no pedestrians, an evasion at
    3 m, a steady approach, an evasion out of range"""
    line = lambda px: np.array([[[x, 0.0]] for x in px])
    cases = [(np.zeros((2, 2)), np.array([[[3.0, 0.0], [0.0, 4.0]], [[1.0, 0.0], [0.0, 2.0]]])),
             (np.zeros((3, 2)), np.zeros((3, 0, 2))),
             (np.zeros((5, 2)), line([4.0, 3.0, 2.0, 2.5, 3.5])),
             (np.zeros((5, 2)), line([5.0, 4.0, 3.0, 2.0, 1.0])),
             (np.zeros((4, 2)), line([10.0, 9.0, 9.5, 10.5]))]
    return [dict(ego_xy=e, ped_xy=p, dt=0.4, ped_vel=np.gradient(p, 0.4, axis=0) if p.shape[1] else np.zeros_like(p))
            for e, p in cases]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    out_path = fc.GOLDEN
    metrics, harness = load_reference(args.ref)
    rng = np.random.default_rng(20251020)
    groups = {"ref": reference_encounters(), "rand": fc.fuzz(7, N_RANDOM)}
    # one encounter each at the ends of the ranges, whatever the seed drew
    groups["rand"][0] = fc.random_encounter(rng, 2, 12, 0.4)
    groups["rand"][1] = fc.random_encounter(rng, 70, 0, 0.1)
    groups["rand"][2] = fc.random_encounter(rng, 70, 12, 1 / 23.98)
    out, meta = {}, {"groups": {g: len(v) for g, v in groups.items()}, "interaction_distance": INTERACTION, "report": {},
                     "rollout_ade": {}, "rollout_ade_interaction": {}, "counts": {}}
    thr, max_d = fc.DEFAULTS["accel_threshold"], fc.DEFAULTS["max_distance"]
    for g, encs in groups.items():
        objs, sims, n_ped, n_onset, worst = [], {}, 0, 0, np.inf
        for i, e in enumerate(encs):
            k = f"{g}_{i}_"
            N = e["ped_xy"].shape[1]
            e["drift"] = rng.normal(0.0, 0.25, (2, N, 2))                                 # the roll-out's two coefficients
            sim = fc.rollout_of(e)
            out[k + "ego_xy"], out[k + "ped_xy"], out[k + "dt"] = e["ego_xy"], e["ped_xy"], np.float64(e["dt"])
            out[k + "ped_vel"], out[k + "drift"] = e["ped_vel"], e["drift"]
            for side, pos in (("real", e["ped_xy"]), ("sim", sim)):
                out[k + f"sep_{side}"] = metrics.min_separation_series(e["ego_xy"], pos)
                for branch, vel in (("fd", None), ("vel", e["ped_vel"])):
                    if side == "sim" and branch == "vel":
                        continue
                    got = metrics.avoidance_onset_distance(e["ego_xy"], pos, ped_vel=vel, dt=e["dt"])
                    step, where, away, margin = onsets_by_the_rule(e["ego_xy"], pos, vel, e["dt"], thr, max_d)
                    assert got.tobytes() == where[step >= 0].tobytes(), (k, side, branch)
                    out[k + f"onset_{side}_{branch}"] = got
                    out[k + f"step_{side}_{branch}"], out[k + f"away_{side}_{branch}"] = step, away
                    if g == "rand":
                        worst = min(worst, margin)
                    if side == "real" and branch == "fd":
                        n_ped += N
                        n_onset += int(np.sum(step >= 0))
            obj = SimpleNamespace(ego_xy=e["ego_xy"], ped_xy=e["ped_xy"], ped_vel=e["ped_vel"], dt=e["dt"])
            objs.append(obj)
            sims[id(obj)] = sim
        assert g != "rand" or worst >= fc.BAND, worst
        harness.simulate_encounter = lambda enc, *a, **kw: sims[id(enc)]
        report = harness.fidelity_report(objs, 0.5, 2.0)
        meta["report"][g] = report
        meta["rollout_ade"][g] = harness.objective_rollout_ade(objs, 0.5, 2.0)
        meta["rollout_ade_interaction"][g] = harness.objective_rollout_ade(objs, 0.5, 2.0, interaction_distance=INTERACTION)
        meta["counts"][g] = {"pedestrians": n_ped, "onsets_real_fd": n_onset, "closest_margin": float(worst)}
        real_fd = [out[f"{g}_{i}_onset_real_fd"] for i in range(len(encs))]
        assert harness._per_encounter_onset(real_fd) == report["onset_per_enc_real_raw"] or \
            np.array_equal(harness._per_encounter_onset(real_fd), report["onset_per_enc_real_raw"], equal_nan=True)
    assert meta["counts"]["rand"]["onsets_real_fd"] >= 40 and meta["counts"]["rand"]["pedestrians"] >= 150, meta["counts"]
    # ---- none kept: an interaction distance below every approach
    meta["rollout_ade_none"] = harness.objective_rollout_ade(objs, 0.5, 2.0, interaction_distance=1e-6)
    assert meta["rollout_ade_none"] == float("inf")
    # ---- _per_encounter_onset on the arrays of the reference's test
    arrays = [np.array([2.0, 4.0]), np.array([3.0]), np.array([]), np.array([2.0, np.nan, 4.0])]
    meta["per_encounter_onset"] = {"arrays": [a.tolist() for a in arrays], "medians": harness._per_encounter_onset(arrays)}
    # ---- compare_distributions_ks: the samples of the reference's test, tied samples, a side emptied by the filter
    r0 = np.random.default_rng(0)
    a, b, c = r0.normal(0.0, 1.0, 500), r0.normal(0.0, 1.0, 500), r0.normal(3.0, 1.0, 500)
    tied_a, tied_b = np.round(r0.normal(0.0, 1.0, 60) * 2) / 2, np.round(r0.normal(0.4, 1.0, 45) * 2) / 2
    out["ks_a"], out["ks_b"], out["ks_c"], out["ks_tied_a"], out["ks_tied_b"] = a, b, c, tied_a, tied_b
    with_nonfinite = np.concatenate([a[:50], [np.inf, np.nan, -np.inf]])
    out["ks_nonfinite"] = with_nonfinite
    meta["ks"] = {"same": metrics.compare_distributions_ks(a, b), "different": metrics.compare_distributions_ks(a, c),
                  "tied": metrics.compare_distributions_ks(tied_a, tied_b),
                  "nonfinite": metrics.compare_distributions_ks(with_nonfinite, b),
                  "empty": metrics.compare_distributions_ks([np.inf, np.nan], [1.0, 2.0])}
    assert meta["ks"]["same"][1] > 0.05 and meta["ks"]["different"][1] < 0.01 and np.isnan(meta["ks"]["empty"][0])
    meta["ks_imbalance"] = [[a_, b_, metrics.ks_sample_imbalance(a_, b_)] for a_, b_ in ((0, 5), (5, 0), (10, 10), (10, 21), (30, 14), (2, 4))]
    # ---- calculate_min_separation on the history of the reference's test
    hist = [SimpleNamespace(ego_state=SimpleNamespace(x=0.0, y=0.0), ped_state=SimpleNamespace(positions=np.array([[px, 0.0]])))
            for px in (2.0, 1.0)]
    series, overall = metrics.calculate_min_separation(hist)
    meta["history"] = {"ped_x": [2.0, 1.0], "series": series.tolist(), "overall": overall}
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    save_npz(out_path, out)
    print(out_path, os.path.getsize(out_path), "bytes;", meta["counts"])


if __name__ == "__main__":
    main()
