"""The premises of tests/test_gpu_wide_crowds.py, on the oracle and the host emulation alone.

  1. the selection of tests/wide_crowds_common.py: 12 instances on 4 handles from fewer than 2000 draws, every one decisive
     in the oracle's table (both verdicts; the budget decides where there is one; sample ids >= 64 decide), every listed
     S, P and track length among them, statics, NaN tracks, footprints and lean-eligible instances as often as the GPU
     tests need, a static obstacle that decides a verdict; eps = 1 can never pass the third condition;
  2. the oracle counts DISTINCT samples: its tables and its plan do not change under a permutation of the sample axis;
  3. the four-word forms of csrc/fot_math.hpp on the host (tests/emu/fot_wide_emu.cpp: collide_candidate_wide,
     EntryColliderT<false, 4> in one piece and in 2 .. 4 segments, EntryColliderT<true, 4> where eligible) return the
     oracle's table on every instance of parts 1 and 3 with S P <= 2000 -- static entries (SID_STATIC) and NaN tracks under
     a SampleMask4, without a GPU;
  4. the wide NaN-cache tensors are what their labels say, and the lane is free exactly where the NaN tracks are forgiven;
  5. at most 5 % of the (instance, path) pairs of the external-path checkers' test decide within 1e-7 of a threshold.
"""
import types

import numpy as np
import pytest

import wide_crowds_common as wc
from integrated_path_planning_amd import _abi
from oracle import oracle as orc
from test_wide_samples_cpu import WideEmu, hold_to_oracle

EMU_LIMIT = 2000                  # S P of the instances the emulation walks (it has no broad phase)


@pytest.fixture(scope="module")
def emu():
    return WideEmu()


# ---- 1 ----------------------------------------------------------------------------------------------------------------

def test_the_selection_keeps_twelve_decisive_instances():
    insts, draws = wc.selection()
    assert draws < wc.MAX_DRAWS and len(insts) == 12
    hs = wc.handles()
    assert len(hs) == 4 and all(len(group) == 3 for _, group in hs) and len({id(h) for h, _ in hs}) == 4
    assert len({i.seed for i in insts}) == 12
    for i in insts:
        lab, st = i.label(), i.want.cand_status
        d = np.asarray(i.req.dist)
        assert d.shape == (i.S, i.P, wc.n_rows(i.t_kind, i.handle.n_total), 2) and i.S > _abi.MAX_SAMPLES, lab
        assert (st == _abi.ST_OK).any() and (st == _abi.ST_COLLISION).any(), lab                          # (a)
        if i.eps > 0.0:                                                                                   # (b)
            assert wc.max_viol(i.eps, i.S) > 0 and (i.want_hard.cand_status != st).any(), lab
            ch = np.flatnonzero(i.want_hard.cand_status != st)
            assert (i.want_hard.cand_status[ch] == _abi.ST_COLLISION).all() and (st[ch] != _abi.ST_COLLISION).all(), lab
        assert i.want64.n_cand == i.want.n_cand and (i.want64.cand_status != st).any(), lab               # (c)
        assert int(np.isnan(d).any((2, 3)).sum()) == i.n_nan, lab
        assert (0 if i.req.static is None else len(i.req.static)) == i.n_static, lab
        assert i.eps in wc.EPS_LIST and i.eps < 1.0 and i.S in wc.S_LIST and i.P in wc.P_LIST, lab
        assert i.n_static in wc.N_STATIC and i.n_nan in tuple(min(n, i.S * i.P) for n in wc.N_NAN), lab


def test_the_selection_covers_what_the_gpu_tests_need():
    insts = wc.crowd_instances()
    assert {i.S for i in insts} == set(wc.S_LIST)
    assert {i.P for i in insts} == set(wc.P_LIST)
    assert {i.t_kind for i in insts} == set(wc.T_KINDS)
    assert {i.T for i in insts if i.t_kind == "one"} == {1}
    assert all(i.T == i.handle.n_total // 2 for i in insts if i.t_kind == "half")
    assert all(i.T == i.handle.n_total + 3 for i in insts if i.t_kind == "over")
    assert sum(i.n_static > 0 for i in insts) >= 4 and sum(i.n_nan > 0 for i in insts) >= 4
    assert {i.n_static for i in insts} == set(wc.N_STATIC) and {i.n_nan for i in insts} >= {0, 3, 40}
    assert sum(i.handle.footprint is not None for i in insts) >= 3
    lean = [i for i in insts if i.lean_eligible]
    assert len(lean) >= 2 and all(i.eps == 0.0 and i.handle.footprint is None and i.handle.n_total <= 64 for i in lean)
    assert sum(i.lean_eligible for i in wc.handles()[0][1]) >= 2          # ... two of one handle: they go out in one launch
    assert sum(wc.max_viol(i.eps, i.S) > 0 for i in insts) >= 3
    # a NaN track at a sample id of the second to fourth mask word
    assert any(np.isnan(np.asarray(i.req.dist)[64:]).any() for i in insts)
    # a static obstacle decides a verdict: the oracle's table changes when the statics are taken away
    moved = [int((i.want_no_static.cand_status != i.want.cand_status).sum()) for i in insts if i.n_static]
    assert len(moved) >= 4 and max(moved) >= 1, moved


def test_a_budget_of_the_whole_distribution_cannot_show_that_high_ids_decide():
    """why eps = 1 is never kept: every sample is forgiven, of the whole tensor and of its first 64 alike"""
    i = next(i for i in wc.crowd_instances() if i.n_static == 0)
    whole = i.handle.oracle(i.req, 1.0)
    cut = i.handle.oracle(wc.with_tensors(i.req, None, np.asarray(i.req.dist)[:64]), 1.0)
    np.testing.assert_array_equal(whole.cand_status, cut.cand_status)
    assert not (whole.cand_status == _abi.ST_COLLISION).any()


# ---- 2 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(12))
def test_the_oracle_does_not_care_about_the_sample_order(k):
    inst = wc.crowd_instances()[k]
    want = inst.want
    for name, perm in wc.permutations(inst.S).items():
        assert sorted(perm) == list(range(inst.S)) and (name == "reversed" or perm[0] != 0)
        got = inst.handle.oracle(wc.permuted(inst, perm), inst.eps)
        lab = f"{inst.label()} [{name}]"
        np.testing.assert_array_equal(got.cand_status, want.cand_status, err_msg=lab)
        np.testing.assert_array_equal(got.cand_keep, want.cand_keep, err_msg=lab)
        np.testing.assert_array_equal(got.cand_nt, want.cand_nt, err_msg=lab)
        np.testing.assert_array_equal(got.cand_cost, want.cand_cost, err_msg=lab)
        assert (got.status, got.best_index, got.stats) == (want.status, want.best_index, want.stats), lab
        if want.status == orc.PLAN_OK:
            for f in orc.PATH_FIELDS:
                np.testing.assert_array_equal(got.path[f], want.path[f], err_msg=f"{lab} {f}")
    # the rolls carry hits across every word edge: sample 63 <-> 64, 127 <-> 128, 191 <-> 192 where the tensor has them
    assert wc.permutations(inst.S)["roll 1"][64] == 63 and wc.permutations(inst.S)["roll 64"][64] == 0


# ---- 3 ----------------------------------------------------------------------------------------------------------------

def test_the_four_word_forms_return_the_oracles_tables_on_crowds(emu):
    walked = [i for i in wc.crowd_instances() if i.S * i.P <= EMU_LIMIT]
    assert len(walked) >= 6 and any(i.n_static for i in walked) and any(i.n_nan for i in walked)
    assert any(np.isnan(np.asarray(i.req.dist)[64:]).any() for i in walked)
    n_lean = 0
    for inst in walked:
        lean = hold_to_oracle(emu, 4, inst.handle, inst)
        assert lean == inst.lean_eligible, inst.label()
        n_lean += lean
    assert n_lean >= 2                                # the lean-wide re-check beside static entries and NaN tracks


def _limits_scene(kw, eps=0.0, footprint=None):
    """the straight road of tests/test_gpu_limits.py as the emulation wrapper's scene"""
    def params_kw(eps_, inflation):
        out = dict(kw, chance_epsilon=eps_, collision_margin_inflation=inflation)
        if footprint is not None:
            out.update(footprint_offsets=[float(o) for o in footprint.offsets], footprint_radius=float(footprint.radius))
        return out
    return types.SimpleNamespace(waypoints=(wc.LIMITS_WX, wc.LIMITS_WY), params_kw=params_kw, footprint=footprint,
                                 n_total=int(round(kw.get("max_t", 5.0) / kw["dt"])) + 1)


@pytest.mark.parametrize("S,P,n_block,n_extra,high_only,label", wc.NAN_CASES, ids=[f"S{c[0]}-P{c[1]}" for c in wc.NAN_CASES])
def test_the_wide_nan_cache_tensors(emu, S, P, n_block, n_extra, high_only, label):
    reqs, n_bad = wc.nan_cache_case(S, P, n_block, n_extra, high_only)
    d, clean = np.asarray(reqs[0].dist), np.asarray(reqs[2].dist)
    assert d.shape == (S, P, 23, 2) and S > _abi.MAX_SAMPLES and not np.isnan(clean).any()
    nan_track = np.isnan(d).any((2, 3))                                  # [S, P]
    assert int(nan_track.sum()) == n_bad == (S - 64 if high_only else S) * n_block + n_extra
    assert nan_track[64:, :n_block].all() and nan_track[64:].sum() >= 1   # sample ids of the second mask word and beyond
    if high_only:
        assert not nan_track[:64].any() and not nan_track[:, n_block:].any()
        assert (np.abs(clean[:64, :n_block]) > 4000.0).any(-1).all() and (np.abs(clean[64:, :n_block]) < 100.0).all()
    else:
        assert nan_track[:, :n_block].all()
    # what each case overflows: CULL_VER = 256 tracks per group, CULL_BAD = 32 NaN tracks, CULL_LIST = 256 kept per step
    assert S * P > 256 or n_bad > 32
    if (S, P) == (65, 4):
        assert S * P == 260 > 256
    if (S, P) == (254, 30):
        assert S * P > 256 and n_bad > 32
    wants = wc.limits_oracle(wc.NAN_KW, reqs)
    assert wants[0].stats["collision_error"] < wants[2].stats["collision_error"], label
    if S * P <= EMU_LIMIT:
        sc = _limits_scene(wc.NAN_KW)
        for j, (rq, want) in enumerate(zip(reqs, wants)):
            inst = types.SimpleNamespace(req=rq, eps=0.0, inflation=1.0, S=S, want=want, label=lambda j=j: f"{label} request {j}")
            assert hold_to_oracle(emu, 4, sc, inst)                      # lean-eligible: 23 steps, no footprint, no budget


def test_the_wide_cull_cache_tensors_decide_by_their_budget():
    reqs = wc.cull_cache_case()
    assert np.asarray(reqs[0].dist).shape == (200, 26, 26, 2) and 200 * 26 == 5200
    assert wc.max_viol(wc.CULL_KW["chance_epsilon"], 200) == 20
    wants = wc.limits_oracle(wc.CULL_KW, reqs, wc.CULL_FOOTPRINT)
    hard = wc.limits_oracle(dict(wc.CULL_KW, chance_epsilon=0.0), reqs, wc.CULL_FOOTPRINT)
    for w, h in zip(wants, hard):
        assert (w.cand_status == _abi.ST_OK).any() and (w.cand_status != h.cand_status).any()


# ---- 5 ----------------------------------------------------------------------------------------------------------------

def test_few_checked_paths_decide_near_a_threshold():
    insts = wc.checker_instances()
    assert any(i.n_static for i in insts) and any(i.n_nan for i in insts)
    assert {"one", "half"} <= {i.t_kind for i in insts}
    pairs = skipped = collide = 0
    for inst in insts:
        cands = wc.checker_candidates(inst)
        assert len(cands) >= 4, inst.label()
        for c, (free, cat, margin) in zip(cands, wc.judge_paths(inst, [wc.oracle_path(inst, c) for c in cands])):
            pairs += 1
            if margin <= wc.CHECK_SKIP_MARGIN:
                skipped += 1
                continue
            # the NumPy restatement and the oracle's plan agree on the candidate's own path
            assert free == (inst.want.cand_status[c] != _abi.ST_COLLISION), f"{inst.label()} cand {c}"
            assert cat == int(inst.want.cand_status[c]), f"{inst.label()} cand {c}"
            collide += not free
    assert pairs >= 50 and collide >= pairs // 4
    assert skipped <= wc.CHECK_SKIP_CAP * pairs, f"{skipped} of {pairs} pairs decide within {wc.CHECK_SKIP_MARGIN:g}"
