"""Safety metrics behind the reference's call surface.

``compute_safety_metrics_static`` has the signature and result dictionary of
src/core/data_structures.py:301-388; the arithmetic runs in ``k_safety``
(csrc/fot_loop_kernels.hip), one wavefront per ego, through ``fot_safety_metrics_batch``.
``SafetyMonitor.metrics_batch`` is the many-ego form the reference lacks.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence

import numpy as np

from .footprint import EgoFootprint
from .planner import BatchPlanner

_STRAIGHT = (np.array([0.0, 1.0]), np.array([0.0, 0.0]))      # a handle needs a reference path; k_safety never reads it


class SafetyMonitor:
    """One libfot handle per footprint (the footprint is a handle constant, include/fot.h fot_params)."""

    def __init__(self, footprint: Optional[EgoFootprint] = None, engine: Optional[BatchPlanner] = None, device: int = -1):
        self.footprint = footprint
        if engine is None:
            kw = {"footprint": footprint} if footprint is not None else {}
            engine = BatchPlanner(waypoints=_STRAIGHT, device=device, **kw)
        self.engine = engine

    def metrics_batch(self, egos, ped_positions: Sequence, ped_velocities: Sequence, ego_radius: float,
                      ped_radius: float) -> np.ndarray:
        return self.engine.safety_metrics(egos, ped_positions, ped_velocities, ego_radius, ped_radius,
                                          use_footprint=self.footprint is not None)

    def metrics(self, ego_state, ped_state, ego_radius: float, ped_radius: float) -> Dict[str, Any]:
        r = self.metrics_batch([[ego_state.x, ego_state.y, ego_state.yaw, ego_state.v]], [ped_state.positions],
                               [ped_state.velocities], ego_radius, ped_radius)[0]
        return {"min_distance": float(r["min_distance"]), "collision": bool(r["collision"]), "ttc": float(r["ttc"]),
                "clearance": float(r["clearance"]), "clearance_ahead": float(r["clearance_ahead"])}


_monitors: Dict[Any, SafetyMonitor] = {}


def compute_safety_metrics_static(ego_state, ped_state, ego_radius: float, ped_radius: float,
                                  footprint: Optional[EgoFootprint] = None) -> Dict[str, Any]:
    """Drop-in for data_structures.py:301 (same arguments, same keys)."""
    key = None if footprint is None else (float(footprint.radius), tuple(float(o) for o in footprint.offsets))
    mon = _monitors.get(key)
    if mon is None:
        mon = _monitors[key] = SafetyMonitor(footprint)
    return mon.metrics(ego_state, ped_state, ego_radius, ped_radius)


# ---- footprint re-verification (A-4): centre, circle cover and exact rectangle, fixed across planner conditions -----------
FOOTPRINT_OBS_DEFAULTS = dict(vehicle_length=4.5, vehicle_width=2.0, n_circles=3, ped_radius=0.2, ego_radius=1.0)
RECHECK_KEYS = ("steps", "yaw_source", "legacy_min_dist", "legacy_collision_steps", "multi_min_dist", "multi_clearance",
                "multi_collision_steps", "rect_min_surface_dist", "rect_clearance", "rect_collision_steps")
FOOTPRINT_METRIC_KEYS = ("legacy_min_dist", "multi_clearance", "multi_violation_steps", "rect_clearance",
                         "rect_violation_steps")


def footprint_geometry(geometry=None):
    """``_abi.FootprintGeom`` of a geometry dictionary (keys of ``FOOTPRINT_OBS_DEFAULTS``; missing ones take the reference's
    fixed 4.5 m x 2.0 m, 3 circles, pedestrian radius 0.2 m, ego radius 1.0 m).  The legacy threshold is ``ego_radius +
    ped_radius``, added here as the reference adds it; ``legacy_radius`` overrides the sum."""
    from . import _abi
    g = dict(FOOTPRINT_OBS_DEFAULTS)
    if geometry not in (None, True):
        unknown = set(geometry) - set(g) - {"legacy_radius"}
        if unknown:
            raise ValueError(f"footprint geometry: unknown keys {sorted(unknown)}")
        g.update(geometry)
    legacy = float(g["legacy_radius"]) if "legacy_radius" in g else float(g["ego_radius"]) + float(g["ped_radius"])
    return _abi.FootprintGeom(float(g["vehicle_length"]), float(g["vehicle_width"]), float(g["ped_radius"]), legacy,
                              int(g["n_circles"]), 0)


def _recheck_call(engine, geom, items, reconstruct):
    """One ``fot_footprint_recheck`` call over ``items`` = [(ego_x, ego_y, ego_yaw | None, ped_positions)]."""
    steps = [len(it[0]) for it in items]
    step_off = np.concatenate([[0], np.cumsum(steps)]).astype(np.int32)
    xy = np.empty((int(step_off[-1]), 2))
    yaw = None if reconstruct else np.empty(int(step_off[-1]))
    counts, rows = [], []
    for (x, y, a, peds), lo, hi in zip(items, step_off[:-1], step_off[1:]):
        xy[lo:hi, 0], xy[lo:hi, 1] = x, y
        if yaw is not None:
            yaw[lo:hi] = a
        if len(peds) != hi - lo:
            raise ValueError("footprint_recheck: one pedestrian array per step")
        for p in peds:
            p = np.asarray(p, dtype=float).reshape(-1, 2)
            counts.append(p.shape[0])
            rows.append(p)
    ped_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ped_xy = np.concatenate(rows) if rows else np.zeros((0, 2))
    return engine.footprint_recheck(geom, step_off, xy, yaw, ped_off, ped_xy, want_series=True)


def footprint_recheck(engine, trajectories, geometry=None, yaw: str = "stored", with_series: bool = False):
    """The reference's post-hoc ``recheck`` (examples/recheck_footprint.py) of saved trajectories on the device.

    trajectories: dictionaries with ``ego_x``, ``ego_y`` [n], optionally ``ego_yaw`` [n], and ``ped_positions``, one [P_i, 2]
    array per step.  yaw: "stored" uses ``ego_yaw`` where a trajectory has it and reconstructs the others' headings;
    "reconstruct" reconstructs all of them (finite differences, held through standstill -- on the device).  All
    trajectories go through ONE ``fot_footprint_recheck`` call (two when "stored" meets both kinds: the entry takes the
    headings of a whole call or of none).  Returns one dictionary per trajectory with ``RECHECK_KEYS``; with
    ``with_series`` also ``series``, the per-step (legacy, multi, rect) minima.  Non-finite coordinates: unspecified."""
    if yaw not in ("stored", "reconstruct"):
        raise ValueError('yaw: "stored" or "reconstruct"')
    geom = footprint_geometry(geometry)
    items = [(np.asarray(t["ego_x"], float), np.asarray(t["ego_y"], float),
              None if yaw == "reconstruct" or t.get("ego_yaw") is None else np.asarray(t["ego_yaw"], float),
              t["ped_positions"]) for t in trajectories]
    out = [None] * len(items)
    for reconstruct in (False, True):
        idx = [i for i, it in enumerate(items) if (it[2] is None) == reconstruct]
        if not idx:
            continue
        rec, series, _ = _recheck_call(engine, geom, [items[i] for i in idx], reconstruct)
        lo = 0
        for i, r in zip(idx, rec):
            row = dict(steps=int(r["steps"]), yaw_source="reconstructed" if reconstruct else "stored",
                       legacy_min_dist=float(r["legacy_min_dist"]), legacy_collision_steps=int(r["legacy_collision_steps"]),
                       multi_min_dist=float(r["multi_min_dist"]), multi_clearance=float(r["multi_clearance"]),
                       multi_collision_steps=int(r["multi_violation_steps"]),
                       rect_min_surface_dist=float(r["rect_min_surface_dist"]), rect_clearance=float(r["rect_clearance"]),
                       rect_collision_steps=int(r["rect_violation_steps"]))
            if with_series:
                row["series"] = series[lo:lo + row["steps"]].copy()
            lo += row["steps"]
            out[i] = row
    return out


def recheck_npz(engine, paths, geometry=None, yaw: str = "stored"):
    """``footprint_recheck`` of ``trajectory.npz`` files (``ego_x``, ``ego_y``, optional ``ego_yaw``, the object array
    ``ped_positions``; ``BatchedClosedLoop.save_results`` writes them), all files in one library call.  Each row also
    carries ``run`` (the file's directory) and ``stored_vs_recomputed_maxdiff``: the largest difference of the per-step
    centre distance to the file's ``min_distances`` (NaN without them, or when they are not all finite)."""
    import os
    trajs, stored = [], []
    for p in paths:
        with np.load(p, allow_pickle=True) as d:
            trajs.append(dict(ego_x=d["ego_x"], ego_y=d["ego_y"], ego_yaw=d["ego_yaw"] if "ego_yaw" in d else None,
                              ped_positions=list(d["ped_positions"])))
            stored.append(np.asarray(d["min_distances"], float) if "min_distances" in d else None)
    rows = footprint_recheck(engine, trajs, geometry=geometry, yaw=yaw, with_series=True)
    out = []
    for p, row, ref in zip(paths, rows, stored):
        legacy = row.pop("series")["legacy"]
        diff = float("nan")
        if ref is not None and np.isfinite(ref).all() and len(ref) == len(legacy):
            diff = float(np.nanmax(np.abs(legacy - ref)))
        out.append(dict(run=os.path.basename(os.path.dirname(os.path.abspath(str(p)))), **row,
                        stored_vs_recomputed_maxdiff=diff))
    return out
