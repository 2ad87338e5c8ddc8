"""What k_frenet_state's one-wave NaN fallback rests on: the arg-min of a sample scan is the same entry whether 64 or 256
workers share out the samples.

A worker takes the samples l, l + W, ... and keeps its first strict minimum (csrc/fot_math.hpp scan_samples; a NaN
distance counts as -inf in the global scan, as np.argmin takes it); a wave merges its 64 workers with the xor butterfly
(wave_argmin), and four waves are folded in ascending order (block_argmin) -- both through scan_merge, the shared code
this test calls on the CPU (tests/emu/fot_select_emu.cpp).  The lowest index wins among equal distances in every
one of these steps, so who evaluated which sample cannot matter: random distances, exact ties, rows that are all NaN.
"""
import numpy as np
import pytest

import selection_ties_common as st

WAVE = st.WAVE


@pytest.fixture(scope="module")
def sel():
    return st.SelectEmu()


def worker_scan(dist, lane, workers, nan_first):
    """scan_samples for one worker: (dist, idx) of its first strict minimum, (inf, -1) if it has none"""
    best, idx = np.inf, -1
    for i in range(lane, len(dist), workers):
        d = dist[i]
        if nan_first and np.isnan(d):
            d = -np.inf
        if d < best:
            best, idx = d, i
    return best, idx


def block_scan(sel, dist, workers, nan_first):
    """the scan of `workers` threads (whole waves): butterfly per wave, waves folded in ascending order"""
    per_wave = []
    for w in range(workers // WAVE):
        cost, idx = zip(*(worker_scan(dist, w * WAVE + l, workers, nan_first) for l in range(WAVE)))
        oc, oi = sel.butterfly(np.array(cost, np.float64), np.array(idx, np.int32))
        assert len(set(int(v) for v in oi)) == 1                  # every lane of the wave holds the wave's entry
        per_wave.append((float(oc[0]), int(oi[0])))
    cost, idx = zip(*per_wave)
    return sel.serial(np.array(cost, np.float64), np.array(idx, np.int32), np.arange(len(per_wave), dtype=np.int32))


def argmin_of(dist, nan_first):
    d = np.where(np.isnan(dist), -np.inf, dist) if nan_first else dist
    ok = ~np.isnan(d) & (d < np.inf)
    return int(np.flatnonzero(ok & (d == d[ok].min()))[0]) if ok.any() else -1


def both(sel, dist, nan_first):
    one = block_scan(sel, dist, WAVE, nan_first)
    four = block_scan(sel, dist, 4 * WAVE, nan_first)
    assert one[1] == four[1] == argmin_of(dist, nan_first), (one, four)
    assert one[0] == four[0] or (np.isnan(one[0]) and np.isnan(four[0]))
    return one


# sample counts: fewer than a wave, the window's 100, one more than the workgroup, the bench path's and a long path's
COUNTS = (1, 63, 100, 257, 600, 5000)


@pytest.mark.parametrize("nan_first", [False, True], ids=["window", "global"])
@pytest.mark.parametrize("n", COUNTS)
def test_random_distances(sel, n, nan_first):
    rng = np.random.default_rng([n, 1])
    both(sel, rng.uniform(0.0, 50.0, n), nan_first)


@pytest.mark.parametrize("nan_first", [False, True], ids=["window", "global"])
@pytest.mark.parametrize("n", COUNTS)
def test_exact_ties(sel, n, nan_first):
    rng = np.random.default_rng([n, 2])
    dist = rng.choice([0.5, 0.75, 2.0], n)                       # three values: the minimum is held by many samples
    _, idx = both(sel, dist, nan_first)
    assert idx == int(np.argmin(dist))
    both(sel, np.full(n, 1.25), nan_first)                        # one value: sample 0
    if n > 70:                                                    # the minimum twice, in different waves' and lanes' shares
        dist = np.full(n, 3.0)
        dist[[69, n - 1]] = 1.0
        assert both(sel, dist, nan_first)[1] == 69


@pytest.mark.parametrize("n", COUNTS)
def test_nan_rows(sel, n):
    dist = np.full(n, np.nan)
    assert both(sel, dist, True)[1] == 0                          # np.argmin of an all-NaN row: its first entry
    assert both(sel, dist, False)[1] == -1                        # the window scan: no sample is below +inf
    if n > 70:                                                    # NaNs among numbers: the first NaN (global), none (window)
        rng = np.random.default_rng([n, 3])
        dist = rng.uniform(0.0, 9.0, n)
        dist[[n - 2, 66]] = np.nan
        assert both(sel, dist, True)[1] == 66
        assert both(sel, dist, False)[1] == int(np.nanargmin(dist))
