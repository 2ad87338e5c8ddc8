"""The step bookkeeping of the evaluation kernels on the device: the cases of tests/step_bookkeeping_common.py (which says
how the oracle's arrays prove that each reaches its branch; tests/test_step_bookkeeping_cpu.py asserts the same counts on the
host emulation) under every evaluation kernel.

Per case, one to four instances in a launch, under the grouped cut, the per-wave cut and the split walk in 2 and 3 time
segments, each in the lean form ("auto": all cases have 21 samples per candidate) and with the general form forced: the
record and the candidate table (status, keep, n_t; cost to 1e-9 relative) are the oracle's, and records and tables are
byte-identical across all eight.  The lean grouped and lean split kernels keep the bookkeeping in scalar registers
(evaluate_segment<LEAN, SREG>), the other four do not: equality across the eight is equality of the two forms.
"""
import numpy as np
import pytest

import limit_boundaries_common as lb
import step_bookkeeping_common as sb
from helpers import assert_record_matches_oracle
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu

# (tile cut, time segments): grouped, per-wave, split in 2 and 3 (fot_debug_set_tile_cut / _eval_segments)
PATHS = {"group": (2, 1), "wave": (1, 1), "split-2": (1, 2), "split-3": (1, 3)}
FORMS = ("auto", "general")
CAP = 1024


@pytest.fixture(scope="module")
def emu():
    return sb.StepEmu()                  # (host code only: the tile tables and the step scene's targets)


def run_case(case, counts=(1, 2, 3, 4)):
    want = case.want
    with BatchPlanner(waypoints=case.waypoints, **case.kw) as bp:
        first = None
        for (path, (cut, seg)) in PATHS.items():
            bp.set_tile_cut(cut)
            bp.set_eval_segments(seg)
            for form in FORMS:
                bp.set_eval_form(form)
                for n_inst in counts:
                    res = bp.plan_batch([case.req] * n_inst)
                    took = bp.last_eval_form()
                    if want.n_cand > 0 and np.isfinite(want.frenet0).all():
                        assert took == ("lean" if form == "auto" else "general"), f"{case.name} [{path}, {form}]: {took}"
                    for i in range(n_inst):
                        label = f"{case.name} [{path}, {form}] inst {i} of {n_inst}"
                        rec = res.records[i]
                        cost, status, keep, nt = bp.candidates(i, cap=CAP)
                        got = (bytes(memoryview(rec).cast("B")), status.tobytes(), keep.tobytes(), cost.tobytes())
                        if first is None:
                            assert_record_matches_oracle(rec, want, label=label)
                            lb.check_tables(label, (rec.n_cand, status, keep, nt), want)
                            np.testing.assert_allclose(cost, want.cand_cost, rtol=1e-9, atol=0.0, err_msg=label)
                            first = got
                        else:
                            for what, a, b in zip(("record", "status", "keep", "cost"), got, first):
                                assert a == b, f"{label}: {what} differs from the first launch's"


def test_hold_split(emu):
    cases = {c.name: c for c in sb.hold_cases()}
    for g in (0, 1):
        moving = sum((sb.tile_facts(emu, cases[n], g) for n in ("ladder", "all_hold", "partial")), [])
        assert any(0 < hold < lanes and ne < loop for lanes, ne, loop, hold in moving), (g, moving)
        assert any(hold == lanes and ne < loop for lanes, ne, loop, hold in moving), (g, moving)
        assert any(lanes < sb.WAVE for lanes, _, _, _ in sb.tile_facts(emu, cases["partial"], g))
        assert all(hold == 0 for _, _, _, hold in sb.tile_facts(emu, cases["standing"], g))
    for case in cases.values():
        run_case(case)


def test_first_nan():
    cases = sb.nan_cases()
    h = sb.nan_positions(cases)
    for pos in sb.NAN_REQUIRED:
        assert h[pos] > 0, f"no candidate with {pos}: {h}"
    for case in cases:
        run_case(case, counts=(1, 3))


def test_step_length(emu):
    cases = sb.step_cases(emu)
    where = {(("first" if case.info["k_max_step"][t.c] == 1 else "last"), d > 0) for case, t, d in cases
             if case.info["k_max_step"][t.c] in (1, case.info["n_t"][t.c] - 1)}
    assert where == {("first", False), ("first", True), ("last", False), ("last", True)}, where
    for case, t, d in cases:
        run_case(case, counts=(1, 4))
