"""The step bookkeeping of the evaluation walk on the CPU: the host emulation against the oracle, and the two forms of
the bookkeeping (with and without scalar registers, csrc/fot_math.hpp evaluate_segment<LEAN, SREG>) against each other.

tests/step_bookkeeping_common.py says what the cases are and how the oracle's arrays prove that each reaches its branch;
those counts are asserted here first.  Then, per case: tests/emu/fot_step_emu.cpp plans the instance (the walk in one piece
and cut into 2 and 3 time segments), its candidate table and record are the oracle's, and every candidate walked in the
form without scalar registers equals the form with them under ne_min = 0, n_eval / 2 and n_eval, bit for bit.
"""
import numpy as np
import pytest

import limit_boundaries_common as lb
import step_bookkeeping_common as sb
from helpers import assert_record_matches_oracle

CK_NANSTEP = 2


@pytest.fixture(scope="module")
def emu():
    return sb.StepEmu()


def judge(emu, case):
    """The emulation's table and record of a case are the oracle's, in one piece and in 2 and 3 segments; -> the tally."""
    emu.reset()
    for seg in (1, 2, 3):
        rec, status, keep, nt, _ = emu.plan(case.kw, case.waypoints, case.req, segments=seg)
        label = f"{case.name} [{seg} segment(s)]"
        lb.check_tables(label, (rec.n_cand, status, keep, nt), case.want)
        assert_record_matches_oracle(rec, case.want, label=label)
    t = emu.tally()
    assert t["differences"] == 0, f"{case.name}: the two forms of the bookkeeping differ: {t}"
    assert t["walked"] == 3 * case.want.n_cand, f"{case.name}: {t}"
    return t


def test_hold_split(emu):
    cases = {c.name: c for c in sb.hold_cases()}
    facts = {(n, g): sb.tile_facts(emu, c, g) for n, c in cases.items() for g in (0, 1)}
    print("\n(lanes, ne_min, n_loop, holding lanes) per tile:", facts)
    assert cases["standing"].want.n_cand == cases["standing"].info["n_grid"], "the standing ego has a ladder"
    for g in (0, 1):
        moving = facts["ladder", g] + facts["all_hold", g] + facts["partial", g]
        # polynomial and holding lanes in one tile: the scalar branch is taken for ne_min steps and not for the rest
        assert any(0 < hold < lanes and ne < loop for lanes, ne, loop, hold in moving), (g, moving)
        # every lane of a tile holds from some step on
        assert any(hold == lanes and ne < loop for lanes, ne, loop, hold in moving), (g, moving)
        # lanes that walk the empty path
        assert any(lanes < sb.WAVE for lanes, _, _, _ in facts["partial", g]), facts["partial", g]
        # no lane holds: ne_min is the shortest horizon, the branch is taken in every step a lane evaluates
        assert all(hold == 0 and ne <= loop for _, ne, loop, hold in facts["standing", g]), facts["standing", g]
    for name, case in cases.items():
        t = judge(emu, case)
        held = int((case.info["n_t"] - np.minimum(case.info["n_eval"], case.info["n_t"])).sum())
        assert t["steps_held"] == 3 * held and t["steps_direct"] == 3 * int(np.minimum(case.info["n_eval"], case.info["n_t"]).sum()), \
            f"{name}: {t}, the oracle's arrays hold {held} step(s)"
        assert (held > 0) == (name != "standing"), (name, held)


def test_first_nan(emu):
    cases = sb.nan_cases()
    h = sb.nan_positions(cases)
    print("\ncandidates by the position of their first NaN sample:", h)
    for pos in sb.NAN_REQUIRED:
        assert h[pos] > 0, f"no candidate with {pos}: {h}"
    for case in cases:
        t = judge(emu, case)
        seen = int((case.info["first_nan"] >= 0).sum())
        # (a singular candidate keeps nothing whatever its NaN; the walk still notes the NaN)
        assert t["seen_nan"] == 3 * seen, f"{case.name}: {t}, the oracle's arrays have {seen} candidate(s) with a NaN sample"
        fn, keep = case.info["first_nan"], case.want.cand_keep
        sing = case.info["singular_before"]
        some = (fn >= 0) & ~sing
        np.testing.assert_array_equal(keep[some], np.where(fn[some] >= 2, fn[some], 0), err_msg=case.name)


def test_step_length(emu):
    cases = sb.step_cases(emu)
    where = {(("first" if case.info["k_max_step"][t.c] == 1 else "last"), d > 0) for case, t, d in cases
             if case.info["k_max_step"][t.c] in (1, case.info["n_t"][t.c] - 1)}
    assert where == {("first", False), ("first", True), ("last", False), ("last", True)}, where
    status = {}
    for case, t, d in cases:
        judge(emu, case)
        status.setdefault(t.c, {})[d > 0] = int(case.want.cand_status[t.c])
    for c, s in status.items():               # the limit just below the largest step drops the candidate, just above does not
        assert s[False] != s[True], (c, s)


def test_nan_step_leaves_the_largest_step_alone(emu):
    """check_sample over (0, 0), (1, 0), (inf, inf), (inf, inf), (2, 0): the third step has NaN length."""
    flags, largest = emu.nan_step()
    assert flags == CK_NANSTEP, flags
    assert largest == [-np.inf, 1.0, np.inf, np.inf, np.inf], largest
