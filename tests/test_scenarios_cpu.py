"""Scenarios (several planner configurations + reference paths in one handle) on the CPU: the C ABI's symbols and
constant, the scenario ids PackedBatch packs, and the multi-scenario batch layout of csrc/fot_setup.hpp run through a
g++ build of tests/emu/fot_scen_layout.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.batch import PackedBatch, PlanRequest, request_from_instance
from integrated_path_planning_amd.params import make_params

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SHIM_SO = os.path.join(EMU_DIR, "_build", "libfot_scen_layout.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
NEW_SYMBOLS = ("fot_add_scenario", "fot_set_scenario_path_waypoints", "fot_set_scenario_path_coeffs",
               "fot_plan_batch_scenarios", "fot_plan_batch_scenarios_device")


def test_library_exports_the_scenario_entry_points():
    lib = _abi.lib()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in _abi.SYMBOLS


def test_max_scenarios_matches_the_header():
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        m = re.search(r"#define FOT_MAX_SCENARIOS (\d+)", f.read())
    assert m and int(m.group(1)) == _abi.MAX_SCENARIOS == 64


def test_packed_batch_packs_scenario_ids():
    reqs = [PlanRequest(x=float(i), y=0.0, yaw=0.0, v=3.0, a=0.0, scenario=s) for i, s in enumerate([0, 2, 1, 2, 0])]
    pb = PackedBatch(reqs)
    assert pb.scenario.dtype == np.int32
    np.testing.assert_array_equal(pb.scenario[:5], [0, 2, 1, 2, 0])
    assert pb.mixed
    p = pb.scenario_ptr()
    assert [p[i] for i in range(5)] == [0, 2, 1, 2, 0]
    plain = PackedBatch([PlanRequest(x=0.0, y=0.0, yaw=0.0, v=3.0, a=0.0)])
    assert not plain.mixed and plain.scenario_ptr() is None and plain.scenario[0] == 0


def test_sharded_planner_refuses_other_scenarios():
    from integrated_path_planning_amd.distributed import ShardedPlanner
    sp = ShardedPlanner.__new__(ShardedPlanner)                  # (no device: the check comes before any GPU work)
    sp.torch = None
    with pytest.raises(ValueError, match="scenario"):
        sp.plan([PlanRequest(x=0.0, y=0.0, yaw=0.0, v=3.0, a=0.0, scenario=1)])


@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(EMU_DIR, "fot_scen_layout.cpp")] + [os.path.join(CSRC, f) for f in
                                                             ("fot_math.hpp", "fot_setup.hpp", "fot_types.h")]
    srcs.append(os.path.join(ROOT, "include", "fot.h"))
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SHIM_SO, srcs[0]],
                       check=True)
    L = C.CDLL(SHIM_SO)
    ip = C.POINTER(C.c_int32)
    L.scen_layout.argtypes = [C.c_int, C.POINTER(_abi.Params), C.c_int, C.POINTER(_abi.Batch), ip, ip, ip,
                              C.c_char_p, C.c_int]
    L.single_layout.argtypes = [C.POINTER(_abi.Params), C.c_int, C.POINTER(_abi.Batch), ip]
    return L


def _scenario_params():
    ps = [make_params(**kw) for _, kw in syn.SCENARIO_PLANNERS]
    ps.append(make_params(dt=0.1, min_t=2.0, d_t_s=1.0))          # another lattice: more horizons, finer speeds
    return ps


def _batch(n):
    reqs = []
    for i in range(n):
        r = request_from_instance(syn.config3_instance(i, S=2, P=3))
        r.target_speed = 1.0 + 0.7 * i                            # lattices of several terminal-speed grid sizes
        reqs.append(r)
    return reqs


@pytest.mark.parametrize("cut", [1, 2], ids=["wave", "group"])
def test_multi_scenario_layout_matches_each_scenarios_own(shim, cut):
    """Every instance of a mixed layout carries its scenario, a tile-table offset into that scenario's run, and the
    candidate and tile counts of the single-scenario layout of its own planner."""
    params = _scenario_params()
    n_scen = len(params)
    reqs = _batch(12)
    rng = np.random.default_rng(5)
    scen = rng.integers(0, n_scen, len(reqs)).astype(np.int32)
    pb = PackedBatch(reqs)
    parr = (_abi.Params * n_scen)(*params)
    out = np.zeros((len(reqs), 4), np.int32)
    base = np.zeros(n_scen, np.int32)
    err = C.create_string_buffer(256)
    ip = C.POINTER(C.c_int32)
    rc = shim.scen_layout(n_scen, parr, cut, C.byref(pb.c), scen.ctypes.data_as(ip), out.ctypes.data_as(ip),
                          base.ctypes.data_as(ip), err, 256)
    assert rc == _abi.OK, err.value
    for s in range(n_scen):
        own = np.zeros((len(reqs), 4), np.int32)
        assert shim.single_layout(C.byref(params[s]), cut, C.byref(pb.c), own.ctypes.data_as(ip)) == _abi.OK
        for i in np.flatnonzero(scen == s):
            assert out[i, 0] == s
            assert out[i, 1] == base[s] + own[i, 1], (i, s)
            assert out[i, 2] == own[i, 2] and out[i, 3] == own[i, 3], (i, s)
    assert base[0] == 0 and np.all(np.diff(base) > 0)


def test_multi_scenario_layout_refusals(shim):
    params = _scenario_params()[:2]
    parr = (_abi.Params * 2)(*params)
    reqs = _batch(3)
    reqs[2].chain_prev_s = True
    pb = PackedBatch(reqs)
    ip = C.POINTER(C.c_int32)
    out = np.zeros((3, 4), np.int32)
    base = np.zeros(2, np.int32)
    err = C.create_string_buffer(256)

    def run(scen):
        scen = np.asarray(scen, np.int32)
        return shim.scen_layout(2, parr, 0, C.byref(pb.c), scen.ctypes.data_as(ip), out.ctypes.data_as(ip),
                                base.ctypes.data_as(ip), err, 256)
    assert run([0, 1, 1]) == _abi.OK                               # the chain stays on one scenario
    assert run([0, 0, 1]) == _abi.ERR_INVALID and b"chain" in err.value
    assert run([0, 2, 0]) == _abi.ERR_INVALID                     # unknown id
    assert run([-1, 0, 0]) == _abi.ERR_INVALID
