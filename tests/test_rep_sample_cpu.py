"""Planning on the representative prediction sample (fot_loop_plan_sample), the part that needs no GPU: the prepend rule and
the fixed-shape block of csrc/fot_repsample.hpp -- the code k_loop_rep_block and the host run -- against NumPy; the proof
that the repeated-last-entry block is the same obstacle to the planner as the reference's shorter tensor, on the oracle;
the condition under which the device's summation order and NumPy's choose the same sample, over the episodes the GPU
tests run; the C ABI's symbols and the Python refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import noise_common as nc
import rep_sample_common as rc
import sgan_common as sc
from closed_loop_common import OracleEngine, OracleResampler, assert_episode_matches, load_dist_episodes, scripted_sample_source
from conftest import ROOT
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from oracle import oracle as orc

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SHIM_SO = os.path.join(EMU_DIR, "_build", "libfot_repsample_emu.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
ENTRIES = ("fot_loop_plan_sample", "fot_loop_run_best_samples", "fot_debug_loop_block")


# ---- 4. symbols and refusals --------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for sym in ENTRIES:
        assert hasattr(lib, sym), f"{sym} not exported by libfot.so"
        assert sym in _abi.SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} not declared in include/fot.h"
    assert re.search(r"#define\s+FOT_LOOP_PLAN_DISTRIBUTION\s+0\b", header) and _abi.LOOP_PLAN_DISTRIBUTION == 0
    assert re.search(r"#define\s+FOT_LOOP_PLAN_REPRESENTATIVE\s+1\b", header) and _abi.LOOP_PLAN_REPRESENTATIVE == 1
    assert _abi.ABI_VERSION == 8                                    # additions only: the version and the words stay
    assert re.search(r"#define\s+FOT_ABI_VERSION\s+8\b", header)


def test_python_refusals():
    ep = load_dist_episodes()
    cfg = dict(ep["meta"]["variants"]["s4_eps0"]["config"])
    tracks = [ep["s4_eps0_ped_traj"]]
    src = scripted_sample_source(4, cfg["pred_len"])
    assert cfg["distribution_aware_planning"]
    # the new keyword together with distribution_aware_planning: both named
    with pytest.raises(ValueError, match="plan_on_representative_sample.*distribution_aware_planning"):
        BatchedClosedLoop(cfg, tracks, sample_source=src, device_samples=True, plan_on_representative_sample=True)
    plain = dict(cfg, distribution_aware_planning=False)
    with pytest.raises(ValueError, match="plan_on_representative_sample needs device_samples=True"):
        BatchedClosedLoop(plain, tracks, sample_source=src, plan_on_representative_sample=True, engine=OracleEngine(plain),
                          resampler=OracleResampler(plain))
    # the keyword off: the refusal and its message as they were
    msg = "device_samples needs a sample_source, distribution_aware_planning"
    for kw in (dict(), dict(plan_on_representative_sample=False)):
        with pytest.raises(ValueError, match=msg):
            BatchedClosedLoop(plain, tracks, sample_source=src, device_samples=True, engine=OracleEngine(plain),
                              resampler=OracleResampler(plain), **kw)
    # ... and with it on, a stand-in engine still cannot take device samples
    with pytest.raises(ValueError, match=msg):
        BatchedClosedLoop(plain, tracks, sample_source=src, device_samples=True, engine=OracleEngine(plain),
                          resampler=OracleResampler(plain), plan_on_representative_sample=True)


# ---- 1. fot_repsample.hpp against NumPy ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(EMU_DIR, "fot_repsample_emu.cpp"), os.path.join(CSRC, "fot_repsample.hpp"),
            os.path.join(CSRC, "fot_predscore.hpp")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        # (no contraction of a * b + c: atol + rtol |cur| is rounded as NumPy rounds it)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-o", SHIM_SO,
                        srcs[0]], check=True)
    L = C.CDLL(SHIM_SO)
    vp = C.c_void_p
    L.rs_close_of.argtypes = [C.c_double, C.c_double]
    L.rs_prepend_of.argtypes = [C.c_int, vp, vp]
    L.rs_block_run.argtypes = [C.c_int, C.c_int, vp, vp, vp]
    L.rs_block_lanes.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp]
    return L


def _np_close(first, cur):
    with np.errstate(invalid="ignore"):
        return bool(np.abs(np.float64(first) - np.float64(cur)) <= rc.ATOL + rc.RTOL * np.abs(np.float64(cur)))


def test_prepend_rule_at_its_threshold(shim):
    """One coordinate at atol + rtol |cur| times 1 +- 1e-3 ... 1e-12 and exactly on it, for current positions of several
    magnitudes and both signs: the header's answer is NumPy's, and the two sides of the threshold answer differently."""
    checked = 0
    for cur in (0.0, 1e-9, 0.3, -0.3, 7.25, -41.03125, 123.456, 2.0e4, -2.0e4):
        thr = rc.ATOL + rc.RTOL * abs(cur)
        assert shim.rs_close_of(cur, cur) == 1
        for sign in (1.0, -1.0):
            for e in range(3, 13):
                for side in (1.0, -1.0):
                    first = cur + sign * thr * (1.0 + side * 10.0 ** -e)
                    assert shim.rs_close_of(first, cur) == int(_np_close(first, cur)), (cur, sign, e, side)
                    checked += 1
            # past the rounding of cur + thr the factor decides: 1e-3 lies outside it for every magnitude above
            assert shim.rs_close_of(cur + sign * thr * (1.0 + 1e-3), cur) == 0
            assert shim.rs_close_of(cur + sign * thr * (1.0 - 1e-3), cur) == 1
            on = cur + sign * thr                                    # "exactly on it", as far as cur + thr is representable
            assert shim.rs_close_of(on, cur) == int(_np_close(on, cur))
    # exactly on it where the sum IS exact: |first - cur| == atol + rtol |cur| bit for bit counts as close (<=)
    assert shim.rs_close_of(rc.ATOL, 0.0) == 1 and _np_close(rc.ATOL, 0.0)
    assert shim.rs_close_of(np.nextafter(rc.ATOL, 1.0), 0.0) == 0
    for bad in ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.inf)):
        assert shim.rs_close_of(*bad) == int(_np_close(*bad)) == 0
    assert checked == 9 * 2 * 10 * 2


@pytest.mark.parametrize("P", [1, 2, 5, 64, 65, 257])
def test_episode_rule_in_every_pedestrian_and_axis(shim, P):
    """All pedestrians close: not prepended.  One coordinate across the threshold -- or a NaN -- in the first, a middle or
    the last pedestrian, on either axis: prepended.  The lane scheme of the kernel answers alike for any lane count."""
    rng = np.random.default_rng(100 + P)
    T = 6
    cur = np.column_stack([rng.uniform(-40.0, 40.0, P), rng.uniform(-6.0, 6.0, P)])
    track = np.zeros((P, T, 2))
    track[:, 0] = cur
    track[:, 1:] = cur[:, None, :] + np.cumsum(rng.normal(0.0, 0.1, (P, T - 1, 2)), axis=1)
    track[:, 1] = cur + 0.5 * (rc.ATOL + rc.RTOL * np.abs(cur)) * rng.choice([-1.0, 1.0], (P, 2))      # inside the threshold
    p = lambda a: np.ascontiguousarray(a).ctypes.data

    def run(track, cur):
        first = np.ascontiguousarray(track[:, 1])
        want = rc.prepend_rule(first, cur)
        assert shim.rs_prepend_of(P, p(first), p(cur)) == int(want)
        blk, pre = rc.host_block(track[:, 1:], cur)
        for lanes in (0, 1, 3, 64, 256, 1024):
            out = np.full((P, T, 2), -7.0)
            tr, cu = np.ascontiguousarray(track), np.ascontiguousarray(cur)
            got = shim.rs_block_run(P, T, p(tr), p(cu), p(out)) if lanes == 0 else shim.rs_block_lanes(lanes, P, T, p(tr), p(cu), p(out))
            assert got == int(pre) == int(want), lanes
            assert out.tobytes() == np.ascontiguousarray(blk).tobytes(), lanes
        return want

    assert run(track, cur) is False
    for who in sorted({0, P // 2, P - 1}):
        for ax in (0, 1):
            thr = rc.ATOL + rc.RTOL * abs(cur[who, ax])
            moved = track.copy()
            moved[who, 1, ax] = cur[who, ax] + thr * (1.0 + 1e-3)
            assert run(moved, cur) is True, (who, ax)
            inside = track.copy()
            inside[who, 1, ax] = cur[who, ax] - thr * (1.0 - 1e-3)
            assert run(inside, cur) is False, (who, ax)
            for arr in ("first", "cur"):
                t2, c2 = track.copy(), cur.copy()
                if arr == "first":
                    t2[who, 1, ax] = np.nan
                else:
                    c2[who, ax] = np.nan
                    t2[:, 0] = c2
                assert run(t2, c2) is True, (who, ax, arr)


def test_both_block_forms_equal_numpy_concatenate(shim):
    rng = np.random.default_rng(7)
    P, n_dense = 5, 50
    dense = rng.normal(0.0, 10.0, (P, n_dense, 2))
    p = lambda a: np.ascontiguousarray(a).ctypes.data
    for cur in (dense[:, 0].copy(), dense[:, 0] + 0.1):              # not prepended / prepended
        track = np.concatenate([cur[:, None], dense], axis=1)        # the distribution block's layout: entry 0 is the current position
        out = np.zeros((P, n_dense + 1, 2))
        pre = shim.rs_block_run(P, n_dense + 1, p(track), p(cur), p(out))
        if np.array_equal(cur, dense[:, 0]):
            assert pre == 0 and np.array_equal(out, np.concatenate([dense, dense[:, -1:]], axis=1))
        else:
            assert pre == 1 and np.array_equal(out, np.concatenate([cur[:, None], dense], axis=1))


# ---- 2. the repeated last entry is the same obstacle ---------------------------------------------------------------------------------
N_DENSE = 50                                     # the planner's n_total = round(max_t / dt) + 1 = n_dense + 1


def _oracle():
    return orc.make_params(**syn.CONFIG3_PLANNER), orc.Spline(syn.STRAIGHT_WX, syn.STRAIGHT_WY)


def _crossing(seed):
    """An ego on the straight path and 1 .. 6 pedestrians that walk across its lattice within the horizon: [P, n_dense, 2]."""
    rng = np.random.default_rng(seed)
    ego = (rng.uniform(0.0, 20.0), rng.uniform(-0.5, 0.5), rng.uniform(-0.05, 0.05), rng.uniform(4.0, 8.0), rng.uniform(-0.5, 0.5))
    P = int(rng.integers(1, 7))
    side = rng.choice([-1.0, 1.0], P)
    start = np.column_stack([ego[0] + rng.uniform(6.0, 38.0, P), side * rng.uniform(1.5, 6.0, P)])
    vel = np.column_stack([rng.normal(0.0, 0.4, P), -side * rng.uniform(0.6, 1.8, P)])
    t = (np.arange(N_DENSE) + 1.0) * 0.1
    return ego, start[:, None, :] + t[None, :, None] * vel[:, None, :]


def _assert_same_plan(a, b, label):
    assert (a.status, a.best_index, a.n_cand) == (b.status, b.best_index, b.n_cand), label
    assert a.stats == b.stats, label
    np.testing.assert_array_equal(a.cand_status, b.cand_status, err_msg=label)
    np.testing.assert_array_equal(a.cand_keep, b.cand_keep, err_msg=label)
    np.testing.assert_array_equal(a.cand_cost, b.cand_cost, err_msg=label)     # (NaN == NaN)
    assert (a.new_prev_s, a.new_last_kappa) == (b.new_prev_s, b.new_last_kappa), label
    assert (a.path is None) == (b.path is None), label
    if a.path is not None:
        assert a.cost == b.cost, label
        for f in orc.PATH_FIELDS:
            np.testing.assert_array_equal(a.path[f], b.path[f], err_msg=f"{label} {f}")


def _plan_both(params, sp, ego, dyn):
    padded = np.concatenate([dyn, dyn[:, -1:]], axis=1)
    assert padded.shape[1] == N_DENSE + 1
    a = orc.plan(params, sp, orc.make_ego(*ego), 8.0, dyn=dyn, table=True)
    b = orc.plan(params, sp, orc.make_ego(*ego), 8.0, dyn=padded, table=True)
    return a, b


def test_repeated_last_entry_plans_like_the_shorter_tensor():
    params, sp = _oracle()
    hit, nan_seen = 0, 0
    for seed in range(24):
        ego, dyn = _crossing(9100 + seed)
        if seed % 8 == 7:                                            # a NaN track: ignored at every time step, either way
            dyn[0, int(seed) % N_DENSE, 0] = np.nan
            nan_seen += 1
        a, b = _plan_both(params, sp, ego, dyn)
        _assert_same_plan(a, b, f"seed {seed}")
        hit += a.stats is not None and a.stats["collision_error"] > 0
    assert hit >= 12 and nan_seen == 3                               # the pedestrians do cross the lattice


def test_repeated_last_entry_when_only_the_last_time_index_collides():
    """A pedestrian far from the road until its LAST dense sample, which lies where the ego is five seconds on: only path
    samples k = n_dense - 1 and k = n_dense (the clipped index, frenet_planner.py:1226-1227) see it."""
    params, sp = _oracle()
    ego = (5.0, 0.0, 0.0, 6.0, 0.0)
    far = np.tile(np.array([[[500.0, 300.0]]]), (1, N_DENSE, 1))
    free = orc.plan(params, sp, orc.make_ego(*ego), 8.0, dyn=far, table=True)
    assert free.stats["collision_error"] == 0 and free.status == orc.PLAN_OK
    # a candidate of the full horizon (n_dense + 1 samples) that passed every check: the pedestrian's last sample goes where
    # that candidate's last sample lies
    idx = int(np.flatnonzero((free.cand_nt == N_DENSE + 1) & (free.cand_status == orc.ST_OK))[0])
    keep, arr, _ = orc.candidate_path(params, sp, free.frenet0, 8.0, idx)
    assert keep == N_DENSE + 1
    last = far.copy()
    last[0, -1] = (arr[orc.PATH_FIELDS.index("x"), N_DENSE], arr[orc.PATH_FIELDS.index("y"), N_DENSE])
    a, b = _plan_both(params, sp, ego, last)
    _assert_same_plan(a, b, "last index only")
    assert a.stats["collision_error"] > 0
    assert a.cand_status[idx] == orc.STATUS_NAMES.index("collision_error")          # that candidate collides now
    # ... and with the last sample moved away again nothing collides: no other time index did
    again = last.copy()
    again[0, -1] = far[0, -1]
    assert orc.plan(params, sp, orc.make_ego(*ego), 8.0, dyn=again, table=True).stats["collision_error"] == 0
    # the one-before-last sample alone is seen by k = n_dense - 2 only in the padded tensor as well
    prev = far.copy()
    prev[0, -2] = last[0, -1]
    a2, b2 = _plan_both(params, sp, ego, prev)
    _assert_same_plan(a2, b2, "one before the last")


# ---- 3. the episodes the GPU tests run: no near-tie among the deviation sums -----------------------------------------------------
def _spy_gaps(sim):
    seen = []
    orig = sim._best_sample

    def spy(dist, off):
        seen.append(rc.gaps(np.asarray(dist), np.asarray(off)))
        return orig(dist, off)
    sim._best_sample = spy
    return seen


def test_reference_episode_has_no_near_tie():
    """s5_best_only through the five-call loop on the oracle: at every step the two smallest dev[s] of every episode differ
    by more than 1e-9 relative -- the condition under which the device's order of summation and NumPy's choose alike."""
    ep = load_dist_episodes()
    var = ep["meta"]["variants"]["s5_best_only"]
    cfg = dict(var["config"])
    sim = BatchedClosedLoop(cfg, [ep["s5_best_only_ped_traj"]], engine=OracleEngine(cfg), resampler=OracleResampler(cfg),
                            sample_source=scripted_sample_source(var["n_samples"], cfg["pred_len"]))
    seen = _spy_gaps(sim)
    hist = sim.run()[0]
    assert_episode_matches(hist, sim.episodes[0].termination_reason, ep, "s5_best_only")
    assert len(seen) == var["steps"] and all(len(g) == 1 for g in seen)
    low = min(float(g.min()) for g in seen)
    print(f"s5_best_only: smallest relative gap of the two smallest deviation sums over {len(seen)} steps: {low:.3e}")
    assert low > rc.GAP


class _CpuCounterSampler:
    """The counter-seeded SganSampler restated on the CPU: the NumPy noise (noise_common) into the NumPy forward pass
    (sgan_common.restate) in float32.  Its samples are those of the library's kernels up to float32 rounding -- some 1e-6
    relative, far from the 1e-9 the gaps are held to."""
    needs_history = True

    def __init__(self, model, S, seed):
        self.args = sc.case_args(model)
        self.state = sc.seeded_state(self.args, sc.case_seed(model), sc.case_scale(model))
        self.num_samples, self.counter_seed = S, seed

    def __call__(self, window, off, slots=None, steps=None):
        counts = np.diff(off)
        assert self.args["noise_mix_type"] == "ped"
        row_slot, row_step = np.repeat(slots, counts), np.repeat(steps, counts)
        row_idx = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, np.int64)
        noise = nc.noise(self.counter_seed, nc.GAUSSIAN, self.num_samples, row_slot, row_step, row_idx, self.args["noise_dim"][0])
        return sc.restate(self.args, self.state, window, np.asarray(off), noise, dtype=np.float32)


def test_sampler_episodes_of_the_gpu_tests_have_no_near_tie():
    cfg, tracks = rc.loop_inputs()
    src = _CpuCounterSampler(rc.LOOP_MODEL, rc.LOOP_SAMPLES, rc.LOOP_SEED)
    sim = BatchedClosedLoop(cfg, tracks, engine=OracleEngine(cfg), resampler=OracleResampler(cfg), sample_source=src)
    seen = _spy_gaps(sim)
    sim.run(rc.LOOP_STEPS)
    assert len(seen) == rc.LOOP_STEPS
    low = min(float(g.min()) for g in seen if len(g))
    print(f"sampler episodes: smallest relative gap over {len(seen)} steps: {low:.3e}")
    assert low > rc.GAP
