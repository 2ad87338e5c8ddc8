"""k_frenet_state with one wave behind the nearest-point search (the default) against all four waves to the end
(FOT_FRENET_WAVES=all), and both against the oracle.

An instance that heads no chain retires waves 1 - 3 behind the last block-wide scan of its search; wave 0 alone refines,
converts, writes the state and composes the group headers.  The switch is read once per process, so every case runs in
two child processes (tests/frenet_waves_common.py; one per setting, each with a time limit), and

  * BatchPlanner.frenet_states and the plan_batch records are byte-identical between the two;
  * the records match the oracle as the other suites require: the arc length of the nearest point bit for bit
    (assert_record_matches_oracle), and frenet_states' arc length bit for bit against the oracle's converter.

Cases (frenet_waves_common): on the road of 2, 11, 65 and 513 knots (513: the lone wave reads the spline from HBM) an
ego without prev_s (global scan only), with prev_s and the winner inside the window (one scan), with a stale prev_s on
either side (winner on the window's upper / lower edge: window, then global), given as a Frenet state (no scan: waves
1 - 3 leave at once), behind the start and beyond the end of the path (refinement clamped at 0 and at s_end), a
standing ego whose window ties; on 11 knots in calls of 1, 3 and 5 instances (a block first, last, interior).  A
chain of three behind its head between two solo instances (the four-wave path and the retired one in one launch).
Group headers from the one-wave tail, grouped against per-wave cut byte for byte and against the oracle: the bench
lattice (144 header items per instance: three passes of the one wave) and the largest lattice of the stored goldens.

The NaN fallback (the conversion fails AND the curve is NaN at the refined arc length, then a re-scan, on wave 0 alone
here) cannot be reached from finite inputs: the handle's spline is fitted from finite, distinct waypoints, so every
coefficient is finite and spline_xy is finite at every arc length the search returns; a non-finite ego reaches the
re-scan with NaN distances throughout and fails the conversion either way.  What the one-wave re-scan rests on -- the
arg-min is the same entry however the samples are shared out -- is held on the CPU (tests/test_frenet_waves_cpu.py).
"""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import frenet_waves_common as fw
from helpers import assert_record_matches_oracle, oracle_plan_for_request
from integrated_path_planning_amd import _abi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CASES = fw.cases()
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frenet_waves_common.py")


def child(tmp, tag, env_value):
    env = dict(os.environ)
    env.pop("FOT_FRENET_WAVES", None)
    if env_value:
        env["FOT_FRENET_WAVES"] = env_value
    out = os.path.join(tmp, tag + ".pkl")
    r = subprocess.run([sys.executable, CHILD, out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (tag, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("frenet_waves"))
    return child(tmp, "one_wave", None), child(tmp, "all_waves", "all")


def record(raw):
    return _abi.Result.from_buffer_copy(raw)


@pytest.mark.parametrize("name", list(CASES))
def test_one_wave_equals_four_waves(runs, name):
    one, four = runs
    assert len(one[name]) == len(four[name]) == len(CASES[name][2])
    for b, (r1, r4) in enumerate(zip(one[name], four[name])):
        assert r1.keys() == r4.keys()
        assert r1["frenet_states"] == r4["frenet_states"], f"{name} batch {b}: frenet_states differ"
        for path in CASES[name][3]:
            for i, (a, c) in enumerate(zip(r1[path], r4[path])):
                assert a == c, f"{name} batch {b} inst {i} ({path}): the one-wave record differs from the four-wave one"


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("heads_")])
def test_headers_of_the_one_wave_tail_grouped_equals_per_wave(runs, name):
    for which in runs:
        for b, run in enumerate(which[name]):
            assert run["group"] == run["wave"], f"{name} batch {b}: grouped records differ from the per-wave ones"


def oracle_wants(params, sp, reqs):
    """the oracle's plan of every request: a chain member as the call behind the one before it"""
    wants, prev_s = [], None
    for rq in reqs:
        one = copy.copy(rq)
        if rq.chain_prev_s:
            one.chain_prev_s, one.prev_s = False, prev_s
        want = oracle_plan_for_request(orc, params, sp, one)
        prev_s = float(want.new_prev_s)
        wants.append(want)
    return wants


# the oracle's plans that long_paths_common has computed already (the same request objects: both are computed once)
STORED = {id(rq): want for n in fw.KNOTS for rq, want in fw.road_requests(n) if want is not None}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_oracle(runs, name):
    kw, wp, batches, paths = CASES[name]
    params, sp = orc.make_params(**kw), orc.Spline(*wp)
    for which, tag in zip(runs, ("one wave", "four waves")):
        for b, reqs in enumerate(batches):
            run = which[name][b]
            if name.startswith("road_"):
                wants = [STORED.get(id(rq)) or oracle_plan_for_request(orc, params, sp, rq) for rq in reqs]
            else:
                wants = oracle_wants(params, sp, reqs)
            for i, want in enumerate(wants):
                assert_record_matches_oracle(record(run[paths[0]][i]), want, label=f"{name} {tag} batch {b} inst {i}")
            # frenet_states: the arc length of the nearest point, bit for bit
            cart = [r for r in reqs if not r.is_frenet and not r.chain_prev_s]
            nps = np.frombuffer(run["frenet_states"][2], np.float64)
            ok = np.frombuffer(run["frenet_states"][3], np.int32)
            assert len(nps) == len(cart) and ok.any()
            for i, r in enumerate(cart):
                s = orc.cartesian_to_frenet_state(sp, orc.make_ego(r.x, r.y, r.yaw, r.v, r.a, prev_s=r.prev_s))[3]
                if ok[i]:
                    assert nps[i] == s, f"{name} {tag} batch {b} ego {i}: s0 {nps[i]!r} != oracle's {s!r}"
