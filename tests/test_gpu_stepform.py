"""The limits kept as running maxima and the heading composed in the low-speed branch, on the device: the cases of
tests/stepform_common.py (which says how the oracle's arrays prove that each reaches its branch;
tests/test_stepform_cpu.py asserts the same counts next to the host emulation) under every evaluation kernel.

Per case, one to four instances in a launch, under the grouped cut, the per-wave cut and the split walk in 2 and 3 time
segments, each in the lean form ("auto": every case has 21 samples per candidate) and with the general form forced: the
record and the candidate table (status, keep, n_t; cost to 1e-9 relative) are the oracle's, and records and tables are
byte-identical across all eight.  The case with a chance budget is not eligible for the lean form: its "auto" launches
take the general kernels too.
"""
import numpy as np
import pytest

import limit_boundaries_common as lb
import stepform_common as sf
from helpers import assert_record_matches_oracle
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu

# (tile cut, time segments): grouped, per-wave, split in 2 and 3 (fot_debug_set_tile_cut / _eval_segments)
PATHS = {"group": (2, 1), "wave": (1, 1), "split-2": (1, 2), "split-3": (1, 3)}
FORMS = ("auto", "general")
CAP = 1024


@pytest.fixture(scope="module")
def emu():
    return lb.Emu()                      # (host code only: the scenes' segment cuts and targets)


def run_case(case, counts=(1, 2, 3, 4), lean=True):
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
                    assert took == ("lean" if form == "auto" and lean else "general"), f"{case.name} [{path}, {form}]: {took}"
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


def test_low_speed_yaw_step_behind_a_hold_row_and_behind_a_cut(emu):
    for case, facts in sf.yaw_cases(emu):
        if facts is not None:
            assert facts["hold_prev"] > 0 and facts["cut_2"] > 0 and facts["cut_3"] > 0, (case.name, facts)
            run_case(case)
        else:
            run_case(case, counts=(1, 3))


def test_one_sample_over_each_limit(emu):
    cases = sf.one_sample_cases(emu)
    reached = {(rule, where) for _, rule, where, _ in cases}
    assert reached >= sf.REACHED, sf.REACHED - reached
    for case, rule, where, c in cases:
        # (by the oracle: the limit's status where a sample k > 0 exceeds it, "ok" where only sample 0 does)
        assert case.want.cand_status[c] == (_abi.ST_OK if where == "k0" else sf.ST_OF[rule]), case.name
        run_case(case, counts=(1, 4))


def test_late_limit_on_a_candidate_inside_an_obstacle(emu):
    (static, c0), (chance, c1) = sf.late_cases(emu)
    assert static.want.cand_status[c0] == _abi.ST_SPEED and chance.want.cand_status[c1] == _abi.ST_SPEED
    run_case(static, counts=(1, 4))
    run_case(chance, counts=(1, 4), lean=False)


def test_partial_tile_and_standing_ego():
    for case in sf.partial_cases():
        run_case(case, counts=(1, 4))
