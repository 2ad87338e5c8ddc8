"""The candidate selection at exact cost ties and non-finite costs: the CPU leg.

plan() selects with the reference's `if cost < min_cost` over the 'ok' candidates in generation order -- the first
minimum wins, a cost not below +inf is never picked.  tests/selection_ties_common.py holds cases whose weights make many
candidates share the minimal cost bit for bit, and says how the winner is moved through tiles, lanes and groups.  Here:

  premises   every case shows, by the oracle's tables and the host's tile tables alone, what it is there for
             (assert_case), and all of them together every place on the list (assert_shown): the winner on lane 0 and on
             the last occupied lane of a tile, in the first and the last tile, in five tiles and three groups, a tied set
             in tiles t and t + 64 before and behind tile 64, a brake-ladder winner, a lowest tied index that is not
             'ok', tied candidates of another keep, every non-finite class;
  emulation  tests/emu/fot_emu.cpp (the kernels' arithmetic headers, its own serial selection) gives the oracle's record
             and status table on every instance;
  merge      csrc/fot_math.hpp select_entry + scan_merge, compiled for the CPU (tests/emu/fot_select_emu.cpp), applied
             in the three shapes the kernels apply them in -- the xor butterfly of wave_argmin, the lane-strided loop
             of select_instance_wave followed by the butterfly (with its keep carry), a serial fold in arrival order --
             on seeded sets in which ties dominate, some with +inf and NaN costs on valid indices, and on the tile
             parts of every case: each shape and every permutation gives what a strict `<` loop written here gives;
  sanitizers the same file as a program of its own, built with -fsanitize=address,undefined and run as it is.

The GPU leg is tests/test_gpu_selection_ties.py.
"""
import os
import subprocess

import numpy as np
import pytest

import limit_boundaries_common as lb
import selection_ties_common as st
from helpers import assert_record_matches_oracle
from integrated_path_planning_amd import _abi

CASES = st.cases()
IDS = [f"{c.lattice}-{c.weights}-{k}" for k, c in enumerate(CASES)]


@pytest.fixture(scope="module")
def sel():
    return st.SelectEmu()


@pytest.fixture(scope="module")
def emu():
    return lb.Emu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_premises_of_the_case(sel, case):
    prem = st.premises(case, sel)
    print("\n" + "\n".join(st.describe(case, prem)))
    st.assert_case(case, prem)


def test_cases_together_show_every_place(sel):
    st.assert_shown([(c, st.premises(c, sel)) for c in CASES])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_matches_the_oracle(emu, case):
    for i, (req, want) in enumerate(zip(case.reqs, case.wants)):
        lab = case.label(i)
        rec, status, keep, nt, _ = emu.plan(case.kw, case.waypoints, req, cap=16384)
        lb.check_tables(lab, (rec.n_cand, status, keep, nt), want)
        assert_record_matches_oracle(rec, want, label=lab)
        assert rec.n_keep == (want.cand_keep[want.best_index] if want.best_index >= 0 else 0), lab


# -- the merge ---------------------------------------------------------------------------------------------------------
def strict_loop(status, cost, keep):
    """The reference's selection, written out: ascending index, strict `<` from +inf.  (cost, index, keep)."""
    best, best_cost, best_keep = -1, float("inf"), 0
    for i in range(len(cost)):
        if status[i] == _abi.ST_OK and cost[i] < best_cost:
            best, best_cost, best_keep = i, float(cost[i]), int(keep[i])
    return best_cost, best, best_keep


def check_shapes(sel, label, status, cost, keep, bounds, rng):
    """One candidate table cut into tiles at `bounds`: entries -> butterfly per tile -> parts -> strided / serial."""
    status, cost, keep = np.asarray(status, np.int32), np.asarray(cost, np.float64), np.asarray(keep, np.int32)
    want_cost, want_idx, want_keep = strict_loop(status, cost, keep)
    p_cost, p_idx, p_keep = [], [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        assert hi - lo <= st.WAVE
        s = np.full(st.WAVE, _abi.ST_DROPPED, np.int32)
        c, ix = np.full(st.WAVE, np.inf), np.full(st.WAVE, -1, np.int32)
        s[: hi - lo], c[: hi - lo], ix[: hi - lo] = status[lo:hi], cost[lo:hi], np.arange(lo, hi)
        ec, ei = sel.entries(s, c, ix)
        oc, oi = sel.butterfly(ec, ei)
        w = strict_loop(status[lo:hi], cost[lo:hi], keep[lo:hi])
        assert np.all(oi == (lo + w[1] if w[1] >= 0 else -1)), f"{label}: tile [{lo}, {hi}) butterfly gives {oi[0]} (slots {set(oi.tolist())}), strict loop {lo + w[1]}"
        if w[1] >= 0:
            assert np.all(oc == w[0]), f"{label}: tile [{lo}, {hi})"
        p_cost.append(oc[0]); p_idx.append(oi[0]); p_keep.append(keep[oi[0]] if oi[0] >= 0 else 0)
    differ, g_cost, g_idx, g_keep = sel.strided(p_cost, p_idx, p_keep)
    assert not differ, f"{label}: the slots of the strided merge disagree"
    assert (g_idx, g_keep) == (want_idx, want_keep), f"{label}: strided merge gives {(g_idx, g_keep)}, strict loop {(want_idx, want_keep)}"
    assert want_idx < 0 or g_cost == want_cost, label
    n = len(p_cost)
    orders = [np.arange(n), np.arange(n)[::-1]] + [rng.permutation(n) for _ in range(4)]
    for perm in orders:
        s_cost, s_idx = sel.serial(p_cost, p_idx, perm)
        assert s_idx == want_idx, f"{label}: serial fold in order {perm[:8]}... gives {s_idx}, strict loop {want_idx}"
        assert want_idx < 0 or s_cost == want_cost, label


@pytest.mark.parametrize("seed", range(40))
def test_merge_shapes_on_seeded_sets(sel, seed):
    """Costs from 3 - 5 values, a third of the sets with +inf and NaN on valid indices, parts of 0 .. 64 candidates (0: an
    empty tile, idx -1), 1 .. 320 parts."""
    rng = np.random.default_rng(4200 + seed)
    n_parts = int(rng.integers(1, 321)) if seed % 4 else (64, 65, 128, 320)[seed // 4 % 4]
    sizes = rng.integers(0, st.WAVE + 1, n_parts)
    if seed % 5 == 0:
        sizes[rng.random(n_parts) < 0.5] = 0                 # many empty parts
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    n = int(bounds[-1])
    values = rng.permutation([0.0, 1.5, np.nextafter(1.5, 2.0), -2.0, 7.25])[: rng.integers(3, 6)]
    cost = rng.choice(values, n)
    if seed % 3 == 0:
        bad = rng.random(n) < 0.25
        cost[bad] = rng.choice([np.inf, np.nan], int(bad.sum()))
    if seed % 6 == 3:
        cost[:] = rng.choice([np.inf, np.nan], n)            # nothing below +inf at all
    status = np.where(rng.random(n) < (0.7 if seed % 2 else 0.05), _abi.ST_OK, rng.integers(0, 6, n))
    keep = rng.integers(1, 250, n)
    check_shapes(sel, f"seed {seed}", status, cost, keep, bounds, rng)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_merge_shapes_on_the_cases_tables(sel, case):
    """The oracle's own candidate tables, cut as either cut of the lattice cuts them."""
    rng = np.random.default_rng(7)
    for i, (req, w) in enumerate(zip(case.reqs, case.wants)):
        for grouped in (False, True):
            c0, n = sel.tile_tables(case.kw, st.n_tv_of(case.kw, req.target_speed), grouped)
            bounds = np.minimum(np.concatenate([c0, [c0[-1] + n[-1]]]), w.n_cand)
            check_shapes(sel, f"{case.label(i)} {'grouped' if grouped else 'wave'} cut", w.cand_status, w.cand_cost,
                         w.cand_keep, bounds, rng)


def test_raw_merge_needs_the_entry_filter(sel):
    """scan_merge alone takes any valid index over an empty slot and keeps a NaN it holds (the nearest-point scans rely
    on their own NaN handling): an 'ok' candidate whose cost is +inf or NaN must be kept out by select_entry."""
    cost, idx = np.full(st.WAVE, np.inf), np.full(st.WAVE, -1, np.int32)
    cost[5], idx[5] = np.inf, 5
    assert sel.butterfly(cost, idx)[1][0] == 5                      # the merge itself would select it
    ec, ei = sel.entries(np.full(st.WAVE, _abi.ST_OK, np.int32), cost, np.arange(st.WAVE, dtype=np.int32))
    assert np.all(ei == -1) and np.all(ec == np.inf)
    ec, ei = sel.entries([_abi.ST_OK, _abi.ST_OK, 2, _abi.ST_OK], [np.nan, 3.0, 1.0, np.inf], [7, 8, 9, 10])
    assert ei.tolist() == [-1, 8, -1, -1] and ec[1] == 3.0


# -- the program of its own, plain and instrumented -------------------------------------------------------------------
def run_program(exe, n_sets, env=None):
    r = subprocess.run([exe, str(n_sets)], capture_output=True, text=True, timeout=600, env=env)
    assert r.stdout.split() == ["sets", str(n_sets), "differences", "0"], r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0, r.stderr[-4000:]
    return r


def test_select_program():
    run_program(st.build_select("o2", ["-O2"], main=True), 300)


def test_select_program_is_clean_under_address_and_undefined_sanitizers():
    # (the runtimes linked into the program itself: it runs as it is, whatever the environment preloads)
    exe = st.build_select("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-static-libasan", "-static-libubsan"], main=True)
    r = run_program(exe, 100, dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
