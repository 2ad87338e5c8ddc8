"""Prediction distributions of more than 64 samples, without a GPU.

The library plans against up to 254 samples on a handle whose sample capacity was raised (fot_set_sample_capacity).  Here:

  1. the oracle reproduces the three reference fixtures of tests/golden/wide_samples/ (100 and 130 samples; written by
     tests/golden/make_golden_wide_samples.py) at the tolerances of tests/test_oracle_golden.py: the oracle, which counts
     violations with a plain loop and has no sample limit, is the reference's above 64 samples as well;
  2. the premises of tests/wide_samples_common.py's budget instances, from the oracle alone: the (eps, S) pairs round as
     listed, the hits take the last sample id and both sides of every word edge, every instance keeps CLEARANCE, the
     oracle's verdict on the target candidate is the pattern's, and no instance is missing;
  3. the portable sample-mask forms of csrc/fot_math.hpp, compiled for the host (tests/emu/fot_wide_emu.cpp) -- the wide
     collide_candidate_wide, EntryColliderT<false, 4> in one piece and in 2 .. 4 merged time segments, and the lean-wide
     EntryColliderT<true, 4> where an instance is eligible -- return the oracle's status table on those instances; the
     one-word forms return the oracle's table on chance_budget_common's instances of up to 64 samples, as before;
  4. the header, the binding and the library agree on FOT_MAX_PLAN_SAMPLES (fot_max_plan_samples), and the words of
     fot_abi_info are the ones they were.

The argument checks of fot_set_sample_capacity / fot_get_sample_capacity need a handle, and creating one needs a GPU:
they are in tests/test_gpu_wide_samples.py, which holds the device forms to the same oracle runs.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chance_budget_common as cb
import wide_samples_common as ws
from conftest import ROOT, Golden, golden_names, wrap_angle
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest
from integrated_path_planning_amd.params import make_params
from oracle import oracle as orc

FIXTURES = ("dist_s100_eps0", "dist_s100_eps005", "footprint3_s130_eps01")
TOL = 1e-9                                            # tests/test_oracle_golden.py


# ---- 1. the reference fixtures ----------------------------------------------------------------------------------------

def test_the_fixtures_are_where_no_default_handle_meets_them():
    assert not set(FIXTURES) & set(golden_names())
    for name in FIXTURES:
        path = os.path.join(ROOT, "tests", "golden", "wide_samples", name + ".npz")
        assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "dist_s64.npz")), name


@pytest.mark.parametrize("name", FIXTURES)
def test_the_oracle_reproduces_the_reference_above_64_samples(name):
    g = Golden("wide_samples/" + name)
    S, P = {"dist_s100_eps0": (100, 5), "dist_s100_eps005": (100, 5), "footprint3_s130_eps01": (130, 4)}[name]
    assert g.dist.shape[:2] == (S, P) and g.dyn is None
    eps = g.meta["planner"]["chance_epsilon"]
    assert int(np.floor(eps * S)) == {"dist_s100_eps0": 0, "dist_s100_eps005": 5, "footprint3_s130_eps01": 13}[name]
    assert bool(g.meta.get("footprint")) == (name == "footprint3_s130_eps01")
    st = g["cand_status"].astype(np.int32)
    assert (st == _abi.ST_OK).any() and (st == _abi.ST_COLLISION).any()
    sp = orc.Spline(g["wx"], g["wy"])
    m = g.meta

    def plan(kw):
        ego = orc.make_ego(*m["ego"], last_kappa=m["last_kappa"], prev_s=m["prev_s"])
        return orc.plan(orc.make_params(**kw), sp, ego, m["target_speed"], m["overrides"], m["max_stop"], static=g.static,
                        dyn=g.dyn, dist=g.dist, table=True)
    out = plan(g.planner_kwargs())
    assert out.n_cand == len(g["cand_cost"])
    np.testing.assert_array_equal(out.cand_nt, g["cand_nt"])
    np.testing.assert_array_equal(out.cand_keep, g["cand_keep"])
    np.testing.assert_allclose(out.cand_cost, g["cand_cost"], rtol=TOL, atol=TOL)
    np.testing.assert_array_equal(out.cand_status, st)
    stats = g["stats"]
    assert out.stats == {orc.STATUS_NAMES[i]: int(stats[i]) for i in range(8) if stats[i] >= 0}
    bi = int(g["best_index"])
    assert out.best_index == bi and bi >= 0 and out.status == orc.PLAN_OK
    np.testing.assert_allclose(out.cost, float(g["best_cost"]), rtol=TOL)
    for f in orc.PATH_FIELDS:
        want, got = g["best_" + f], out.path[f]
        assert len(got) == len(want), f
        if f == "yaw":
            np.testing.assert_allclose(wrap_angle(got - want), 0.0, atol=TOL)
        else:
            np.testing.assert_allclose(got, want, rtol=TOL, atol=TOL, err_msg=f)
    np.testing.assert_allclose(out.new_last_kappa, float(g["last_kappa_after"]), rtol=TOL, atol=TOL)
    if eps > 0.0:                                     # the budget decides something: a verdict differs from eps = 0's
        hard = plan(dict(g.planner_kwargs(), chance_epsilon=0.0)).cand_status
        ch = np.flatnonzero(hard != st)
        assert len(ch) and (hard[ch] == _abi.ST_COLLISION).all() and (st[ch] == _abi.ST_OK).all(), name


# ---- 2. the premises of the budget instances ----------------------------------------------------------------------------

def test_the_pairs_round_as_listed():
    ws.pair_facts()
    assert len(ws.PAIRS) == 15
    got = {p: int(np.floor(np.float64(p[0]) * np.float64(p[1]))) for p in ws.PAIRS}
    assert got == ws.PAIRS


@pytest.mark.parametrize("S", sorted({S for _, S in ws.PAIRS}))
def test_sample_ids_start_at_the_last_id_and_the_word_edges(S):
    ids = ws.sample_ids(S)
    assert sorted(ids) == list(range(S))
    want = [s for s in (S - 1, 0, 63, 64, 65, 127, 128, 129, 191, 192, 193) if s < S]
    want = list(dict.fromkeys(want))
    assert ids[:len(want)] == want, (S, ids)
    assert ids[len(want):] == sorted(ids[len(want):])


@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_the_oracle_alone_separates_the_patterns(name):
    sc, insts = ws.scene(name), ws.instances(name)
    assert len(sc.cands) == 2 and len(insts) == ws.expected_count(sc) == 2 * (3 * 15 - 2)
    by = {}
    for inst in insts:
        assert inst.req.dist.shape == (inst.S, ws.P, sc.n_total, 2) and inst.S > _abi.MAX_SAMPLES
        got = int(inst.want.cand_status[inst.cand])
        want = _abi.ST_COLLISION if inst.collides else _abi.ST_OK
        assert got == want, f"{inst.label()}: oracle status {got}, the pattern says {want}"
        assert inst.want.n_cand == sc.free.n_cand
        ch = np.flatnonzero(inst.want.cand_status != sc.free.cand_status)     # only a pending candidate may change
        assert (sc.free.cand_status[ch] == _abi.ST_OK).all() and (inst.want.cand_status[ch] == _abi.ST_COLLISION).all()
        by[(inst.pattern, inst.eps, inst.S, inst.cand)] = inst
    for (eps, S), m in ws.PAIRS.items():
        ids = ws.sample_ids(S)
        for c in sc.cands:
            a, b, cc = (by.get((p, eps, S, c)) for p in ws.PATTERNS)
            assert a is not None and cc is not None, (name, eps, S, c)
            assert (b is None) == (m + 1 > S) == (eps == 1.0), (name, eps, S, c)
            assert a.hit_ids == cc.hit_ids == ids[:m] and len(set(a.hit_ids)) == m
            if b is not None:
                assert b.hit_ids == ids[:m + 1]
                assert a.want.cand_status[c] != b.want.cand_status[c], f"{a.label()}: A and B agree on the target"
            # the hitting samples, read off the tensors: exactly the pattern's, C through both pedestrians at every step
            for inst in (a, b, cc):
                if inst is None:
                    continue
                near = np.abs(np.asarray(inst.req.dist) - np.array(sc.ego[:2])).max(-1) < 1000.0        # [S, P, T]
                assert sorted(np.flatnonzero(near.any((1, 2)))) == sorted(inst.hit_ids), inst.label()
            if m:
                near = np.abs(np.asarray(cc.req.dist) - np.array(sc.ego[:2])).max(-1) < 1000.0
                assert near[cc.hit_ids][:, :, sc.steps(c)].all() and near.sum() == m * ws.P * len(sc.steps(c))
            # beyond 64 hits the budget reaches into the second word, at 254 into the fourth
            if m >= 11:
                assert {s for s in (S - 1,) + ws.EDGE_IDS if s < S}.issubset(a.hit_ids)
                assert len({s >> 6 for s in a.hit_ids}) == (S + 63) // 64       # every mask word the distribution has


@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_every_instance_keeps_its_clearance(name):
    sc = ws.scene(name)
    for inst in ws.instances(name):
        a = np.asarray(inst.req.dist)                 # float32-exact: one oracle run serves both tensor dtypes
        np.testing.assert_array_equal(a, a.astype(np.float32).astype(np.float64), err_msg=inst.label())
        got = cb.instance_clearance(sc, inst)
        assert got >= ws.CLEARANCE, f"{inst.label()}: clearance {got:.3e}"


# ---- 3. the portable forms on the host ----------------------------------------------------------------------------------

class WideEmu:
    SRC = os.path.join(ROOT, "tests", "emu", "fot_wide_emu.cpp")
    SO = os.path.join(ROOT, "tests", "emu", "_build", "libfot_wide_emu.so")

    def __init__(self):
        csrc = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
        srcs = [self.SRC, os.path.join(ROOT, "tests", "emu", "fot_emu.cpp"), os.path.join(ROOT, "include", "fot.h")]
        srcs += [os.path.join(csrc, f) for f in ("fot_math.hpp", "fot_setup.hpp", "fot_types.h")]
        if not os.path.exists(self.SO) or os.path.getmtime(self.SO) < max(os.path.getmtime(s) for s in srcs):
            os.makedirs(os.path.dirname(self.SO), exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", self.SO, self.SRC],
                           check=True)
        self.L = C.CDLL(self.SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self.L.emu_wide_tables.argtypes = [C.c_int, C.POINTER(_abi.Params), C.c_int, dp, dp, C.POINTER(_abi.Batch), C.c_int,
                                           ip, ip, ip, ip, ip, ip, C.c_char_p]

    def tables(self, words, sc, inst, cap=4096):
        """{form: status table} of one instance under the `words`-word forms, and whether it is lean-eligible"""
        wx, wy = (np.ascontiguousarray(w) for w in sc.waypoints)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        params = make_params(**sc.params_kw(inst.eps, inst.inflation))
        pb = PackedBatch([PlanRequest(**{**inst.req.__dict__, "scenario": 0})])
        t = {k: np.full(cap, -9, np.int32) for k in ("definition", "collider", "lean")}
        seg = np.full((3, cap), -9, np.int32)
        n, lean = C.c_int32(0), C.c_int32(0)
        err = C.create_string_buffer(256)
        rc = self.L.emu_wide_tables(words, C.byref(params), len(wx), wx.ctypes.data_as(dp), wy.ctypes.data_as(dp), C.byref(pb.c),
                                    cap, t["definition"].ctypes.data_as(ip), t["collider"].ctypes.data_as(ip),
                                    seg.ctypes.data_as(ip), t["lean"].ctypes.data_as(ip), C.byref(n), C.byref(lean), err)
        assert rc == 0, f"{inst.label()}: emulation rc {rc} {err.value}"
        out = {k: v[:n.value] for k, v in t.items()}
        for i in range(3):
            out[f"{i + 2} segments"] = seg[i, :n.value]
        if not lean.value:
            assert (out.pop("lean") == -1).all()
        return out, bool(lean.value)


@pytest.fixture(scope="module")
def emu():
    return WideEmu()


def hold_to_oracle(emu, words, sc, inst):
    tabs, lean = emu.tables(words, sc, inst)
    assert lean == ws.lean_eligible(sc, inst), inst.label()
    for form, st in tabs.items():
        assert len(st) == inst.want.n_cand, (inst.label(), form)
        np.testing.assert_array_equal(st, inst.want.cand_status, err_msg=f"{inst.label()} [{words}-word {form}]")
    return lean


@pytest.mark.parametrize("name", ws.SCENE_NAMES)
def test_the_four_word_forms_return_the_oracles_tables(emu, name):
    sc = ws.scene(name)
    n_lean = sum(hold_to_oracle(emu, 4, sc, inst) for inst in ws.instances(name))
    # the lean-wide re-check ran where the issue's rule says so: the two eps = 0 pairs on the straight scene
    assert n_lean == (2 * 2 * 3 if name == "straight" else 0)


@pytest.mark.parametrize("name", cb.SCENE_NAMES)
def test_the_one_word_forms_return_what_they_returned(emu, name):
    """chance_budget_common's instances of up to 64 samples through EntryColliderT<., 1> and collide_candidate, after the
    mask became a parameter: the oracle's tables, which tests/test_chance_budget_cpu.py holds the full emulation to."""
    sc = cb.scene(name)
    insts = [i for i in cb.instances(name) if i.req.dist is not None and i.group in ("A", "B", "C")]
    assert len(insts) >= 80
    for inst in insts:
        hold_to_oracle(emu, 1, sc, inst)


def test_a_one_word_form_refuses_more_than_64_samples(emu):
    sc = ws.scene("straight")
    inst = ws.instances("straight")[0]
    wx, wy = (np.ascontiguousarray(w) for w in sc.waypoints)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    params = make_params(**sc.params_kw(inst.eps, inst.inflation))
    pb = PackedBatch([PlanRequest(**{**inst.req.__dict__, "scenario": 0})])
    z = np.zeros(4 * 4096, np.int32)
    n, lean = C.c_int32(0), C.c_int32(0)
    err = C.create_string_buffer(256)
    rc = emu.L.emu_wide_tables(1, C.byref(params), len(wx), wx.ctypes.data_as(dp), wy.ctypes.data_as(dp), C.byref(pb.c), 4096,
                               z.ctypes.data_as(ip), z.ctypes.data_as(ip), z.ctypes.data_as(ip), z.ctypes.data_as(ip),
                               C.byref(n), C.byref(lean), err)
    assert rc == _abi.ERR_UNSUPPORTED and b"sample" in err.value and b"64" in err.value
    assert b"fot_set_sample_capacity" in err.value


# ---- 4. the ABI word ----------------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_plan_sample_capacity(tmp_path):
    lib = _abi.lib()
    got = (C.c_int32 * 64)()
    n = lib.fot_abi_info(64, got)
    text = open(os.path.join(ROOT, "include", "fot.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (FOT_[A-Z_]+) (\d+)\b", text)}
    lib.fot_max_plan_samples.restype = C.c_int32
    assert lib.fot_max_plan_samples() == defs["FOT_MAX_PLAN_SAMPLES"] == _abi.MAX_PLAN_SAMPLES == 254
    assert defs["FOT_MAX_SAMPLES"] == _abi.MAX_SAMPLES == 64 == got[_abi.ABI_WORD_NAMES.index("FOT_MAX_SAMPLES")]
    assert n == defs["FOT_ABI_INFO_WORDS"] == len(_abi.ABI_WORD_NAMES)        # an addition: no word of fot_abi_info changes
    assert {"fot_set_sample_capacity", "fot_get_sample_capacity", "fot_max_plan_samples"} <= set(_abi.SYMBOLS)
    for sym in ("fot_set_sample_capacity", "fot_get_sample_capacity"):
        assert hasattr(lib, sym)
    # a library built with another FOT_MAX_PLAN_SAMPLES is refused by the loader
    want = _abi.abi_expectation()
    src = tmp_path / "fake.c"
    src.write_text("#include <stdint.h>\nint32_t fot_abi_info(int32_t cap, int32_t *out) { static const int32_t v[] = {"
                   + ",".join(map(str, want)) + "}; for (int i = 0; i < %d && i < cap && out; ++i) out[i] = v[i]; return %d; }\n"
                   % (len(want), len(want)) + "int32_t fot_max_plan_samples(void) { return 200; }\n")
    so = tmp_path / "fake.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    with pytest.raises(ImportError, match="FOT_MAX_PLAN_SAMPLES"):
        _abi._check_abi(C.CDLL(str(so)), str(so))
