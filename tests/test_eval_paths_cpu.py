"""helpers.EVAL_PATHS without a GPU: what set_eval_path sets for each name, and the premise the "-noflat" names stand on.

The flat form of the lean evaluation kernels takes over every lean-eligible launch on an exactly straight path, so the
names "auto", "group" and "split-wave" mean the flat kernels there and "group-noflat" / "split-noflat" the lean kernels
every bent road runs.  That only guards anything while the suite's fixtures keep straight paths among them: the counts
below pin how many goldens and reference episodes do, and that the goldens of the walk's rare branches are among them.
"""
import numpy as np
import pytest

import helpers
from closed_loop_common import load_episodes
from conftest import Golden, golden_names
from helpers import EVAL_PATH_KNOBS, EVAL_PATHS, NOFLAT_PATHS, set_eval_path, waypoints_are_flat

OLD_NAMES = {"auto": (0, 0), "group": (2, 1), "wave": (1, 1), "split-wave": (1, 4)}
RARE_BRANCH_GOLDENS = ("trunc_end", "trunc_end60", "nan_ped_dist", "nan_ped_single", "creep", "standstill", "emergency_stop")
FLAT_EPISODES = {"base", "fast", "shift", "walls", "footprint", "inflate", "rnd0", "rnd1", "rnd3", "rnd5"}


class Recorder:
    """stands in for a BatchPlanner: keeps what the three debug hooks were last given, and every call in order"""

    def __init__(self):
        self.cut = self.seg = self.flat = "unset"
        self.calls = []

    def set_tile_cut(self, cut):
        self.cut = cut
        self.calls.append(("cut", cut))

    def set_eval_segments(self, seg):
        self.seg = seg
        self.calls.append(("seg", seg))

    def set_flat(self, on):
        assert on in (0, 1), "set_eval_path sets the knob: -1 only queries"
        self.flat = on
        self.calls.append(("flat", on))
        return False


def knobs(path, bp=None):
    bp = bp or Recorder()
    set_eval_path(bp, path)
    return bp.cut, bp.seg, bp.flat


@pytest.mark.parametrize("path", EVAL_PATHS)
def test_every_name_sets_all_three_knobs(path):
    bp = Recorder()
    got = knobs(path, bp)
    assert "unset" not in got, f"[{path}] leaves a knob as the name before it set it: {got}"
    assert sorted(k for k, _ in bp.calls) == ["cut", "flat", "seg"]
    assert got == EVAL_PATH_KNOBS[path]


def test_a_loop_over_the_names_leaks_no_state():
    """whatever name came before: the same triple, and "auto" last restores a handle's defaults (0, 0, 1)"""
    for before in EVAL_PATHS:
        for path in EVAL_PATHS:
            bp = Recorder()
            set_eval_path(bp, before)
            assert knobs(path, bp) == knobs(path), (before, path)
    assert knobs("auto") == (0, 0, 1)


def test_the_triples_are_pairwise_distinct():
    triples = [knobs(p) for p in EVAL_PATHS]
    assert len(set(triples)) == len(EVAL_PATHS) == len(set(EVAL_PATHS)), triples


def test_the_four_old_names_keep_their_shape_and_allow_the_flat_form():
    for path, shape in OLD_NAMES.items():
        assert path in EVAL_PATHS
        assert knobs(path) == shape + (1,), path


def test_the_new_names_are_the_grouped_and_the_split_shape_with_the_flat_form_off():
    new = [p for p in EVAL_PATHS if p not in OLD_NAMES]
    assert tuple(new) == NOFLAT_PATHS and len(new) == 2
    shapes = {knobs(p)[:2] for p in new}
    assert shapes == {OLD_NAMES["group"], OLD_NAMES["split-wave"]}, "the two families that have a flat kernel"
    assert all(knobs(p)[2] == 0 for p in new)
    assert set(helpers.FLAT_KERNEL_PATHS) == {"group", "split-wave"}


def test_waypoints_are_flat():
    x = np.arange(0.0, 50.0, 10.0)
    assert waypoints_are_flat(x, np.zeros(5)) and waypoints_are_flat(np.full(5, -2.25), x) and waypoints_are_flat(x[::-1], np.full(5, 3.5))
    assert not waypoints_are_flat(x, 1e-300 * x) and not waypoints_are_flat(np.cos(0.37) * x, np.sin(0.37) * x)
    assert not waypoints_are_flat(x[:1], np.zeros(1))


# ---- the premise, as data ----------------------------------------------------------------------------------------------

def flat_goldens():
    out = []
    for n in golden_names():
        g = Golden(n)
        if waypoints_are_flat(g["wx"], g["wy"]):
            out.append(n)
    return out


def test_forty_one_of_ninety_six_goldens_are_on_exactly_straight_paths():
    names, flat = golden_names(), flat_goldens()
    assert (len(flat), len(names)) == (41, 96), f"{len(flat)} of {len(names)} goldens are on straight paths"
    missing = [n for n in RARE_BRANCH_GOLDENS if n not in flat]
    assert not missing, f"rare-branch goldens no longer on a straight path (the -noflat legs lose them): {missing}"


def test_the_straight_goldens_keep_their_spline_flat():
    """the stored coefficients of the still coordinate are exactly zero beyond the constant term, as spline_is_flat asks"""
    for n in flat_goldens():
        g = Golden(n)
        still = "y" if (g["wy"] == g["wy"][0]).all() else "x"
        for c in "bcd":
            assert not g[f"sp_{c}{still}"].any(), f"{n}: sp_{c}{still} is not all zero"


def test_ten_of_thirteen_reference_episodes_are_on_straight_paths():
    meta = load_episodes()["meta"]["variants"]
    flat = {n for n, v in meta.items()
            if waypoints_are_flat(v["config"]["reference_waypoints_x"], v["config"]["reference_waypoints_y"])}
    assert (len(flat), len(meta)) == (10, 13), sorted(flat)
    assert flat == FLAT_EPISODES and set(meta) - flat == {"turn", "rnd2", "rnd4"}
    # the closed-loop leg of test_gpu_loop_run.py: three short lean-eligible ones
    for n, steps in (("fast", 41), ("rnd5", 37), ("inflate", 57)):
        cfg = meta[n]["config"]
        assert n in flat and meta[n]["steps"] == steps
        assert cfg.get("ego_footprint", "circle") == "circle" and cfg.get("chance_epsilon", 0.0) == 0.0
