"""A sample count per slot of a sweep loop (fot_loop_set_slot_samples), the part that needs no GPU: the two symbols; the
ragged layout of csrc/fot_sweep.hpp -- the code the host and the kernels' tables run -- against a NumPy restatement, past
2^31 points on offsets alone; the premise that the count matters on the crowd the GPU tests use, on the oracle loop; and
the argument checks of the two Python sources.

The arithmetic runs in a program of its own (tests/emu/fot_slot_samples_emu.cpp): built plainly and a second time with
-fsanitize=address,undefined, and run as it is (never loaded into Python).  The GPU leg is tests/test_gpu_slot_samples.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import loop_sweep_common as sw
import recorded_samples_common as rs
import slot_samples_common as ss
from closed_loop_common import OracleEngine, OracleResampler, load_episodes, scenario_config, scripted_sample_source
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.prediction import RecordedSamples, SganSampler, record_samples

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
DIST, REP = sw.DIST, sw.REP


def test_library_exports_the_entry_points():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "fot.h")) as f:
        header = f.read()
    for name in ("fot_loop_set_slot_samples", "fot_debug_loop_slot_samples"):
        assert hasattr(lib, name) and name in _abi.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert _abi.ABI_VERSION == 8 and re.search(r"#define\s+FOT_ABI_VERSION\s+8\b", header)   # additions: the version stays
    assert "the slots of one sweep share one" not in header


# ---- the arithmetic of fot_sweep.hpp ------------------------------------------------------------------------------------------------
def build(tag, flags):
    exe = os.path.join(EMU_DIR, "_build", "fot_slot_samples_emu_" + tag)
    srcs = [os.path.join(EMU_DIR, "fot_slot_samples_emu.cpp"), os.path.join(CSRC, "fot_sweep.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, srcs[0]], check=True)
    return exe


PEDS = (0, 1, 33, 65, 30)
RUNNING = ([0, 1, 2, 3, 4], [1, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 3], [1, 3], [3], [0], [])


def frame_cases():
    """(counts, slots, slot_S, modes, T, select_all) of every frame case: fixed ragged ones, random ones, equal counts, and
    offsets past 2^31 points."""
    rng = np.random.default_rng(20240921)
    out = []
    for slot_S in (ss.COUNTS, (1, 1, 1, 1, 1), (254, 64, 65, 1, 20), (6, 6, 6, 6, 6)):
        for modes in ([DIST] * 5, [REP] * 5, [DIST, REP, DIST, REP, DIST], [REP, DIST, REP, DIST, REP]):
            for slots in RUNNING:
                out.append(([PEDS[e] for e in slots], slots, slot_S, modes, 51, False))
    for _ in range(60):
        n_slots = int(rng.integers(1, 12))
        slot_P = rng.choice([0, 0, 1, 2, 31, 64, 65, 130], n_slots)
        slot_S = rng.choice([1, 1, 2, 5, 63, 64, 65, 200, 254], n_slots)
        modes = rng.integers(0, 2, n_slots)
        slots = sorted(rng.choice(n_slots, int(rng.integers(0, n_slots + 1)), replace=False).tolist())
        out.append(([int(slot_P[e]) for e in slots], slots, [int(s) for s in slot_S], [int(m) for m in modes],
                    int(rng.choice([2, 51, 256])), bool(rng.integers(0, 2))))
    big = [1_000_000, 0, 1_000_000, 999_999]                         # offsets only: nothing is allocated
    for slot_S in ((254, 1, 64, 200), (1, 254, 254, 1)):
        for modes in ([REP] * 4, [DIST, REP, REP, DIST]):
            out.append((big, [0, 1, 2, 3], slot_S, modes, 256, True))
    return out


def case_lines():
    lines = []
    for counts, slots, slot_S, modes, T, select_all in frame_cases():
        most, ep_S, blk, size, off, sel = ss.frame(counts, slots, slot_S, modes, T, select_all)
        line = "frame %d %d %d %s %s %d %s %s" % (len(counts), T, int(select_all), " ".join(map(str, counts)), " ".join(map(str, slots)),
                                                  len(slot_S), " ".join(map(str, slot_S)), " ".join(map(str, modes)))
        want = [most] + ep_S + blk + [size] + [v for pair in zip(off, sel) for v in pair]
        lines.append((re.sub(" +", " ", line), " ".join(map(str, want))))
    for slot_P, slot_S, T in ((PEDS, ss.COUNTS, 51), ((30,) * 64, (5, 10, 20, 50, 100, 100, 200, 200) * 8, 51),
                              ((2 ** 20,) * 3, (254, 1, 254), 256)):
        lines.append(("capacity %d %d %s %s" % (len(slot_P), T, " ".join(map(str, slot_P)), " ".join(map(str, slot_S))),
                      str(ss.capacity(slot_P, slot_S, T))))
    return lines


def run_cases(exe, env=None):
    cases = case_lines()
    r = subprocess.run([exe], input="\n".join(c[0] for c in cases) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for (line, want), answer in zip(cases, got):
        assert answer.split() == want.split(), (line[:200], answer[:200], want[:200])
    return r


def test_ragged_layout_equals_the_restatement():
    """Random ragged frames with episodes without pedestrians, counts of 1 and of 254, every slot running and the first, a
    middle and the last slot dropped, no episode at all; offsets beyond 2^31 points (computed, nothing allocated)."""
    wants = [w.split() for line, w in case_lines() if line.startswith("frame")]
    assert any(int(v) > 2 ** 31 for w in wants for v in w)
    run_cases(build("o2", ["-O2"]))


def test_program_is_clean_under_address_and_undefined_sanitizers():
    # (the runtimes linked into the program itself: it runs as it is, whatever the environment preloads)
    exe = build("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-static-libubsan"])
    r = run_cases(exe, dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_equal_counts_reduce_to_the_uniform_layout():
    """With every count equal to S the blocks are today's blk_off and the tensor today's sweep_layout; the capacity never
    exceeds sweep_capacity_points of the source's S."""
    for slots in RUNNING:
        counts = [PEDS[e] for e in slots]
        for S, T in ((6, 51), (1, 2), (130, 256)):
            for modes in ([DIST, REP, DIST, REP, DIST], [REP] * 5):
                most, ep_S, blk, size, off, sel = ss.frame(counts, slots, [S] * 5, modes, T)
                uniform = [sum(S * P * T for P in counts[:i]) for i in range(len(counts) + 1)]
                assert blk == uniform and blk[-1] == sw.dist_end(counts, S, T)
                assert (size, off, sel) == sw.layout(counts, slots, modes, blk[-1], T)
                assert most == (S if slots else 0) and ep_S == [S] * len(slots)
    assert ss.capacity(PEDS, ss.COUNTS, 51) < ss.capacity(PEDS, [6] * 5, 51) == (6 + 1) * sum(PEDS) * 51
    # a smaller count moves every later block forward by exactly what it leaves out
    _, _, blk, *_ = ss.frame(PEDS, [0, 1, 2, 3, 4], ss.COUNTS, [DIST] * 5, 51)
    assert blk == [0, 0, 1 * 1 * 51, 51 + 4 * 33 * 51, 51 + 4 * 33 * 51 + 6 * 65 * 51, 51 + 4 * 33 * 51 + 6 * 65 * 51 + 3 * 30 * 51]


# ---- the premise: the count matters on the crowd the GPU tests use ------------------------------------------------------------------
def _oracle_run(cfg, track, ego, samples):
    sim = BatchedClosedLoop(cfg, [track], [ego], engine=OracleEngine(cfg), resampler=OracleResampler(cfg),
                            sample_source=RecordedSamples(samples))
    sim.run(sw.SWEEP_STEPS)
    return [(s["ego"].tobytes(), np.asarray(s["cost"]).tobytes(), np.asarray(s["has_path"]).tobytes()) for s in sim._steps]


def _recording(cfg, track):
    return record_samples(cfg, [track], scripted_sample_source(sw.SWEEP_S, cfg["pred_len"]), sw.SWEEP_STEPS, dtype=np.float64).samples


def test_premise_the_count_matters_on_the_oracle_loop():
    """chance_epsilon = 0.2 over one crowd and scenario: 6 samples allow floor(1.2) = 1 violating sample, the first 4 of
    them floor(0.8) = 0 -- the two loops select different candidates at some lock step.  A loop that plans on its
    representative sample follows sample 0 with a count of 1 and the sample nearest the mean with 6.  (The stand-in engine
    hands the samples over on the host: one configuration, one count -- the uniform loops the sweep's slots are held to.)"""
    assert int(0.2 * 6) == 1 and int(0.2 * 4) == 0 and int(0.2 * 3) == 0
    cfg = sw.condition(*ss.EPS_CONDITION)
    crowd = ss.eps_crowd()
    rec = _recording(cfg, crowd)
    ego = list(cfg["ego_initial_state"])
    six, four = _oracle_run(cfg, crowd, ego, rec), _oracle_run(cfg, crowd, ego, ss.prefix(rec, 4))
    assert len(six) == len(four) == sw.SWEEP_STEPS and any(a != b for a, b in zip(six, four))
    # the representative-mode slot of the ragged sweep: slot 1, its one pedestrian, count 1 against 6
    cfgs, tracks = sw.ragged_conditions(), ss.tracks()
    assert ss.COUNTS[1] == 1 and not cfgs[1]["distribution_aware_planning"] and tracks[1].shape[1] == 1
    ego = sw.ragged_egos(cfgs)[1]
    rec = _recording(cfgs[1], tracks[1])
    six, one = _oracle_run(cfgs[1], tracks[1], ego, rec), _oracle_run(cfgs[1], tracks[1], ego, ss.prefix(rec, 1))
    assert len(six) == len(one) and any(a != b for a, b in zip(six, one))


# ---- the Python rules ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meta():
    return load_episodes()["meta"]


def test_recorded_samples_slot_samples(meta):
    base = dict(scenario_config(meta), distribution_aware_planning=True)
    L = base["pred_len"]
    rec = np.zeros((4, 6, L, 4, 2))
    src = RecordedSamples(rec, slot_samples=[6, 1])
    assert list(src.slot_samples) == [6, 1] and src.num_samples == 6 and RecordedSamples(rec).slot_samples is None
    for bad in ([0, 6], [7, 1], [-1, 2]):
        with pytest.raises(ValueError, match=r"RecordedSamples: slot_samples holds one count in 1 \.\. 6"):
            RecordedSamples(rec, slot_samples=bad)
    for bad in ([[1, 2]], [1.5, 2.0]):
        with pytest.raises(ValueError, match="RecordedSamples: slot_samples holds one integer sample count per slot"):
            RecordedSamples(rec, slot_samples=bad)
    with pytest.raises(ValueError, match="RecordedSamples: slot_samples names 3 slots, the loop has 2"):
        RecordedSamples(rec, slot_samples=[1, 2, 3]).attach([0, 2, 4], L)
    tracks = [np.zeros((40, 2, 2))] * 2
    with pytest.raises(ValueError, match="the sample source's slot_samples names 3 slots, the loop has 2 episodes"):
        BatchedClosedLoop(base, tracks, sample_source=RecordedSamples(rec, slot_samples=[1, 2, 3]), device_samples=True)
    # the five-call step and stand-in engines plan against one count
    needs = "slot_samples needs device_samples=True and the one-call step"
    for kw in (dict(), dict(device_samples=True, fused=False), dict(device_samples=True, engine=OracleEngine(base)),
               dict(device_samples=True, resampler=OracleResampler(base))):
        with pytest.raises(ValueError, match=needs):
            BatchedClosedLoop(base, tracks, sample_source=RecordedSamples(rec, slot_samples=[6, 1]), **kw)
        with pytest.raises(ValueError, match=needs):
            BatchedClosedLoop([base, dict(base, chance_epsilon=0.2)], tracks, sample_source=RecordedSamples(rec, slot_samples=[6, 1]), **kw)


def test_sgan_sampler_slot_samples():
    import sgan_common as sc
    from integrated_path_planning_amd.prediction import SganWeights
    a = sc.case_args("a_pool_step_ped_bn")
    w = SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed("a_pool_step_ped_bn"), sc.case_scale("a_pool_step_ped_bn")))
    s = SganSampler(None, w, 20, counter_seed=7, slot_crowd=[0, 0, 1], slot_samples=[5, 20, 1])
    assert list(s.slot_samples) == [5, 20, 1] and s.num_samples == 20
    assert SganSampler(None, w, 20, counter_seed=7).slot_samples is None
    with pytest.raises(ValueError, match=r"SganSampler: slot_samples holds one count in 1 \.\. 20"):
        SganSampler(None, w, 20, counter_seed=7, slot_samples=[5, 21])
    with pytest.raises(ValueError, match=r"SganSampler: slot_samples holds one count in 1 \.\. 20"):
        SganSampler(None, w, 20, counter_seed=7, slot_samples=[0, 2])
    with pytest.raises(ValueError, match="SganSampler: slot_samples takes every slot's first samples of one draw: it needs counter_seed"):
        SganSampler(None, w, 20, seed=3, slot_samples=[5, 20])
    with pytest.raises(ValueError, match="SganSampler: slot_samples and slot_crowd hold one entry per slot"):
        SganSampler(None, w, 20, counter_seed=7, slot_crowd=[0, 0, 1], slot_samples=[5, 20])
