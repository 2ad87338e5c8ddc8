"""The kernel headers' spline on reference paths of 65, 513, 2000 and 4000 knots (tests/long_paths_common.py), on the CPU
through tests/emu: the tridiagonal solve of build_spline against the oracle's coefficients (pinned to the reference's
by the `long_*` goldens, tests/test_oracle_golden.py), spline_index's binary search -- twelve levels deep at 4000 knots
-- on every knot and one ulp either side, and the sample count of the global nearest-point scan."""
import ctypes as C

import numpy as np
import pytest

import long_paths_common as lp
from oracle import oracle as orc
from test_emu_logic import emu  # noqa: F401  (the fixture that builds tests/emu)

KNOTS = (65, 513, 2000, 4000)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module", params=KNOTS)
def fitted(request, emu):  # noqa: F811
    n = request.param
    wx, wy = lp.road(n)
    out = np.zeros(9 * n)
    assert emu.emu_spline(n, wx.ctypes.data_as(_dp), wy.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == 0
    return n, out.reshape(9, n), orc.Spline(wx, wy).coeffs()


def test_one_road_for_every_knot_count():
    wx, wy = lp.road(lp.ROAD_MAX_KNOTS)
    for n in (2, 27, 65, 1500):
        ax, ay = lp.road(n)
        assert np.array_equal(ax, wx[:n]) and np.array_equal(ay, wy[:n])
    step = np.hypot(np.diff(wx), np.diff(wy))
    assert 1.0 <= step.min() and step.max() <= 4.0


def test_tridiagonal_solve_against_the_oracle(fitted):
    n, got, want = fitted
    for f, key in enumerate(["s", "ax", "bx", "cx", "dx", "ay", "by", "cy", "dy"]):
        assert len(want[f]) in (n, n - 1)
        # (the tolerance of test_emu_logic.py::test_native_spline_fit)
        np.testing.assert_allclose(got[f, :len(want[f])], want[f], rtol=1e-10, atol=1e-11, err_msg=f"{key} at {n} knots")


def test_segment_lookup_on_every_knot_and_one_ulp_either_side(fitted, emu):  # noqa: F811
    n, got, _ = fitted
    knots = np.ascontiguousarray(got[0])
    assert np.all(np.diff(knots) > 0.0)
    s = np.ascontiguousarray(np.concatenate([knots, np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf),
                                             0.5 * (knots[1:] + knots[:-1]), [-1.0, knots[-1] + 1.0]]))
    idx = np.full(len(s), -7, np.int32)
    emu.emu_spline_index(n, knots.ctypes.data_as(_dp), len(s), s.ctypes.data_as(_dp), idx.ctypes.data_as(_ip))
    want = np.clip(np.searchsorted(knots, s, "right") - 1, 0, n - 2)
    np.testing.assert_array_equal(idx, want)
    assert set(idx[:n].tolist()) == set(range(n - 1))                       # every segment is reached through its knot


def test_global_scan_sample_count(fitted, emu):  # noqa: F811
    n, got, _ = fitted
    knots = np.ascontiguousarray(got[0])
    s_end = float(knots[-1])
    emu.emu_global_search_count.restype = C.c_int
    assert emu.emu_global_search_count(n, knots.ctypes.data_as(_dp)) == max(int(s_end / 0.1), 100)
    if n == 2000:
        assert int(s_end / 0.1) > 49000                                     # the 5 km road: no cap anywhere near
    short = np.array([0.0, 4.0, 9.0])                                       # below 10 m: the floor of 100 samples
    assert emu.emu_global_search_count(3, short.ctypes.data_as(_dp)) == 100
