"""The inputs of the chance-budget tests are what they claim: checked on the oracle and the host emulation alone.

tests/chance_budget_common.py builds instances that count: max_viol = floor(eps S) distinct samples hit a target candidate
(pattern A), one more (B), the same number repeated over steps, pedestrians and circles (C), and the static / NaN /
inflation twins (D, E, F).  Here, without a GPU:

  1. the oracle's status of the target candidate is the one each pattern names, and A and B differ in it for every
     (scene, pair, target);
  2. the sample ids of every pattern are distinct and include 0, 31, 32 and S - 1 where they exist;
  3. every instance keeps every (candidate, step, circle) point of the lattice at |d^2 / R^2 - 1| >= CLEARANCE from every
     obstacle row that step reads -- a condition on the inputs, not a tolerance: no instance is dropped;
  4. the host emulation (tests/emu/fot_emu.cpp: csrc/fot_math.hpp + fot_setup.hpp run by loops, with its internal
     EntryCollider-against-collide_candidate and 2..4-segment comparisons) returns the oracle's status table exactly.

The device forms of the same logic are held to the same oracle runs by tests/test_gpu_chance_budget.py.
"""
import ctypes as C

import numpy as np
import pytest

import chance_budget_common as cb
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest
from integrated_path_planning_amd.params import make_params
from limit_boundaries_common import Emu


def test_the_pairs_round_as_intended():
    cb.pair_facts()
    ms = {(e, S): cb.max_viol(e, S) for e, S in cb.pairs()}
    assert len(ms) == 16
    assert ms[(0.0, 1)] == 0 and ms[(1.0, 1)] == 1 and ms[(0.5, 2)] == 1 and ms[(0.1, 20)] == 2
    assert (ms[(0.1, 31)], ms[(0.1, 32)], ms[(0.1, 33)]) == (3, 3, 3)
    assert (ms[(0.05, 63)], ms[(0.05, 64)], ms[(0.5, 64)]) == (3, 3, 32)


@pytest.mark.parametrize("S", sorted({S for _, S in cb.pairs()}))
def test_sample_ids_are_distinct_and_start_at_the_edges_of_the_mask(S):
    ids = cb.sample_ids(S)
    assert sorted(ids) == list(range(S))
    want = [s for s in (S - 1, 0, 32, 31, 33, 63) if s < S]
    assert ids[:len(dict.fromkeys(want))] == list(dict.fromkeys(want)), (S, ids)


@pytest.mark.parametrize("name", cb.SCENE_NAMES)
def test_scene_and_targets(name):
    sc = cb.scene(name)
    n_total = {"straight": 21, "long": 76, "arc30": 21}[name]
    assert sc.n_total == n_total and len(sc.offsets) == (3 if name == "arc30" else 1)
    assert len(sc.cands) == 2, f"{name}: no brake-ladder entry reaches the collision check"
    grid, brake = sc.cands
    assert sc.free.cand_status[grid] == _abi.ST_OK and sc.free.cand_status[brake] == _abi.ST_OK
    assert sc.free.cand_nt[grid] == sc.free.cand_keep[grid] == n_total
    # the brake-ladder entry stands still well before the end: its profile is shorter than the tile's longest
    p = sc.points[brake, :, 0]
    held = np.flatnonzero((np.diff(p, axis=0) == 0.0).all(1))
    assert len(held) and held[0] + 1 < (2 * n_total) // 3 and (np.diff(p[held[0]:], axis=0) == 0.0).all()
    if name == "long":
        assert {63, 64} <= set(sc.steps(grid)) and {63, 64} <= set(sc.steps(brake))


@pytest.mark.parametrize("name", cb.SCENE_NAMES)
def test_the_oracle_alone_separates_the_patterns(name):
    sc, insts = cb.scene(name), cb.instances(name)
    by = {}
    for inst in insts:
        got = int(inst.want.cand_status[inst.cand])
        want = _abi.ST_COLLISION if inst.collides else _abi.ST_OK
        assert got == want, f"{inst.label()}: oracle status {got}, the pattern says {want}"
        assert inst.want.n_cand == sc.free.n_cand
        np.testing.assert_array_equal(inst.want.cand_nt, sc.free.cand_nt, err_msg=inst.label())
        # only a pending candidate may change, and only to a collision
        ch = np.flatnonzero(inst.want.cand_status != sc.free.cand_status)
        assert (sc.free.cand_status[ch] == _abi.ST_OK).all() and (inst.want.cand_status[ch] == _abi.ST_COLLISION).all()
        by[(inst.pattern, inst.eps, inst.S, inst.cand)] = inst
    n_b = 0
    for eps, S in cb.pairs():
        m = cb.max_viol(eps, S)
        for c in sc.cands:
            a, b, cc = (by.get((p, eps, S, c)) for p in "ABC")
            assert a is not None and cc is not None, (name, eps, S, c)
            assert (b is None) == (m + 1 > S), (name, eps, S, c)
            assert len(a.hit_ids) == len(cc.hit_ids) == m and len(set(a.hit_ids)) == m
            ids = cb.sample_ids(S)
            for need in (S - 1, 0, 31, 32):          # ... are among the hitting samples as soon as the budget reaches them
                if need < S and ids.index(need) < m:
                    assert need in a.hit_ids
            if b is not None:
                n_b += 1
                assert len(set(b.hit_ids)) == m + 1 and b.hit_ids[:m] == a.hit_ids
                assert a.want.cand_status[c] != b.want.cand_status[c], f"{a.label()}: A and B agree on the target"
            # C hits at every target step through both pedestrians, in the samples of A only
            d = np.asarray(cc.req.dist)
            near = np.abs(d - np.array(sc.ego[:2])).max(-1) < 1000.0             # [S, P, T]
            assert sorted(np.flatnonzero(near.any((1, 2)))) == sorted(cc.hit_ids)
            if m:
                assert (near[cc.hit_ids][:, :, sc.steps(c)]).all() and near.sum() == m * cb.P * len(sc.steps(c))
    assert n_b >= 2 * (len(cb.pairs()) - 2)
    # the extras: one of each, the twins on the same tensor but for the one thing that differs
    ex = {i.pattern: i for i in insts if i.group == "extra"}
    assert sorted(ex) == ["D", "D+static", "E", "E-twin", "F", "F-single"]
    assert ex["D"].req.dist is ex["D+static"].req.dist and len(ex["D"].hit_ids) == ex["D"].S
    e, t = np.asarray(ex["E"].req.dist), np.asarray(ex["E-twin"].req.dist)
    assert np.isnan(e).sum() == 1 and np.isnan(t).sum() == 1
    (s, p, _, _), (s2, p2, _, _) = np.argwhere(np.isnan(e))[0], np.argwhere(np.isnan(t))[0]
    assert s == s2 and p != p2 and s in ex["E"].hit_ids
    assert np.isfinite(e[s, p2]).all() and (np.abs(e[s, p2] - np.array(sc.ego[:2])).max(-1) > 1000.0).all()
    assert ex["F"].req.dyn is None and ex["F-single"].req.dist is None
    np.testing.assert_array_equal(ex["F-single"].req.dyn, np.asarray(ex["F"].req.dist)[0])


@pytest.mark.parametrize("name", cb.SCENE_NAMES)
def test_every_instance_keeps_its_clearance(name):
    sc, insts = cb.scene(name), cb.instances(name)
    assert len(insts) >= 90
    for inst in insts:
        for a in (inst.req.static, inst.req.dyn, inst.req.dist):
            if a is not None:                        # float32-exact: one oracle run serves both tensor dtypes
                a = np.asarray(a)
                np.testing.assert_array_equal(a, a.astype(np.float32).astype(np.float64), err_msg=inst.label())
        got = cb.instance_clearance(sc, inst)
        assert got >= cb.CLEARANCE, f"{inst.label()}: clearance {got:.3e}"


@pytest.fixture(scope="module")
def emu():
    return Emu().L


@pytest.mark.parametrize("name", cb.SCENE_NAMES)
def test_the_emulation_agrees_with_the_oracle(emu, name):
    sc, insts = cb.scene(name), cb.instances(name)
    wx, wy = (np.ascontiguousarray(w) for w in sc.waypoints)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    cap = 4096
    for inst in insts:
        params = make_params(**sc.params_kw(inst.eps, inst.inflation))
        pb = PackedBatch([PlanRequest(**{**inst.req.__dict__, "scenario": 0})])
        out = (_abi.Result * 1)()
        cost, status, keep = np.zeros(cap), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        err = C.create_string_buffer(256)
        rc = emu.emu_plan_batch(C.byref(params), len(wx), wx.ctypes.data_as(dp), wy.ctypes.data_as(dp), C.byref(pb.c), out, cap,
                                cost.ctypes.data_as(dp), status.ctypes.data_as(ip), keep.ctypes.data_as(ip), err)
        assert rc == 0, f"{inst.label()}: emulation rc {rc} {err.value}"
        n = out[0].n_cand
        assert n == inst.want.n_cand, inst.label()
        np.testing.assert_array_equal(status[:n], inst.want.cand_status, err_msg=inst.label())
        np.testing.assert_array_equal(keep[:n], inst.want.cand_keep, err_msg=inst.label())
