"""Limits placed at value (1 + delta) of a candidate's own extreme, through the header emulation: the CPU leg.

The scenes, targets and instances of tests/limit_boundaries_common.py (see there for how each threshold is steered and
what is left out on purpose) run through tests/emu/fot_emu.cpp -- csrc/fot_math.hpp and csrc/fot_setup.hpp with loops in
place of the launch grid, every candidate walked in one piece AND in 2, 3 and 4 time segments -- one emulated plan call
per instance, against the oracle's tables and record under the same inputs; the instances of the pairwise rules (step
length, yaw cap) a second time with the tables of the 4-segment walk itself, whose every segment rebuilds its
predecessor sample.  This keeps check_sample / check_status /
final_status and the per-instance limits of build_batch_layout under a directed test on every machine.

Conditions (asserted): every target's floor 10 dev is <= 1e-9; measured here, every target keeps every delta down to
1e-11 (the emulation's quantities differ from the oracle's by 9e-14 at most: the yaw cap), so the share retained at 1e-11
is asserted to be 1; in every scene at least a fifth of the instances change a status against the obstacle-free table;
the deciding samples cover k = 1, the last kept sample, a held sample of a brake-ladder entry, a step across a cut of
the 4-segment walk for both pairwise rules and (76-sample scenes) k >= 64 (COVERAGE in limit_boundaries_common.py:
every reachable (rule, case)); sample 0 and precedence instances exist and the oracle says what
they are meant to show.  The GPU leg is tests/test_gpu_limit_boundaries.py.
"""
import numpy as np
import pytest

import limit_boundaries_common as lb
from helpers import assert_record_matches_oracle
from integrated_path_planning_amd import _abi


@pytest.fixture(scope="module")
def emu():
    return lb.Emu()


def run_instances(emu, sc, insts):
    applied = [0, 0]
    for i, inst in enumerate(insts):
        lab = f"{sc.name} inst {i} {inst.label()}"
        lb.check_kind(sc, inst)
        rec, status, keep, nt, margins = emu.plan(dict(sc.kw, **inst.kw), sc.waypoints, inst.req)
        lb.check_tables(lab, (rec.n_cand, status, keep, nt), inst.want)
        assert_record_matches_oracle(rec, inst.want, label=lab)
        lb.check_margins(sc, inst, margins, lab, applied)       # candidate_margins, the diagnostic of the fuzz sweeps
        if any(t.rule in lb.PAIRWISE for t, _ in inst.targets):  # the 4-segment walk on its own: prev rebuilt at each cut
            rec, status, keep, nt, _ = emu.plan(dict(sc.kw, **inst.kw), sc.waypoints, inst.req, segments=4)
            lb.check_tables(lab + " [4 segments]", (rec.n_cand, status, keep, nt), inst.want)
            assert_record_matches_oracle(rec, inst.want, label=lab + " [4 segments]")
        for (t, d), (m, _) in zip(inst.targets, inst.expect):    # the test's own construction: the threshold IS |delta| away
            assert abs(m - abs(d)) <= 0.01 * abs(d), f"{lab}: the oracle's own margin is {m:.3e}"
    assert applied[0] >= 0.8 * applied[1], f"{sc.name}: the target's own comparison decides {applied[0]} of {applied[1]} margins only"


@pytest.mark.parametrize("name", list(lb.SCENES))
def test_limits_at_the_boundary_match_the_oracle(emu, name):
    sc = lb.Scene(name, emu)
    _, paths = emu.paths(sc.kw, sc.waypoints, sc.request())
    insts, picked, avail = lb.build(sc, lambda c: paths[c])
    lists = list(picked.values())
    if "v_last" in sc.rules:
        def at(target_speed):
            _, p = emu.paths(sc.kw, sc.waypoints, sc.request(target_speed=target_speed))
            return lambda c: p[c]
        more, ts = lb.v_last_scene_targets(sc, at)
        insts, lists = insts + more, lists + [ts]
    share, worst = lb.retained(lists)
    assert share["1e-11"] == 1.0, f"{name}: share of the targets retained per |delta| {share}, worst dev {worst}"
    assert lb.changed_share(sc, insts) >= 0.2, f"{name}: {lb.changed_share(sc, insts):.0%} of the instances change a status"
    lb.assert_coverage(sc, insts, picked)
    run_instances(emu, sc, insts)


def test_brake_ladder_gate(emu):
    """Ego speeds at which the oracle's s_d is 0.1 (1 + delta): the ladder is there exactly above the gate."""
    sc = lb.Scene("fast", emu)
    insts = lb.gate_instances(sc)
    assert len(insts) >= 10
    for inst in insts:
        assert (inst.want.n_cand > min(i.want.n_cand for i in insts)) == (inst.delta > 0), inst.label()
        rec, status, keep, nt, _ = emu.plan(sc.kw, sc.waypoints, inst.req)
        dev = abs(rec.frenet0[1] - inst.want.frenet0[1]) / 0.1
        assert 10.0 * dev <= lb.FLOOR_MAX, inst.label()
        if abs(inst.delta) >= 10.0 * dev:
            lb.check_tables(f"gate {inst.label()}", (rec.n_cand, status, keep, nt), inst.want)
            assert_record_matches_oracle(rec, inst.want, label=inst.label())


def test_pairwise_cut_positions_come_from_the_tile_tables(emu):
    """The cuts a cross-segment target straddles: ceil(n_loop / 4) of its tile under either cut of the lattice, n_loop
    between the candidate's own length and the longest candidate's."""
    sc = lb.Scene("step", emu)
    for seg in sc.seg_len:
        assert len(seg) == sc.free.n_cand
        lo, hi = -(-sc.free.cand_nt // 4), -(-sc.n_total // 4)
        assert np.all((seg >= lo) & (seg <= hi)), (seg, lo, hi)
    assert _abi.ST_DROPPED == 8
