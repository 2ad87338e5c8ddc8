"""k_cull's index arithmetic without integer divisions (csrc/fot_math.hpp), against the plain forms it replaces.

k_cull ran a division by a run-time value per lane in four places; a division is some twenty vector instructions.  It
now uses

* ``div_by_magic(j, P, div_magic(P))`` for the sample index ``j / P`` of a scattered entry, ``div_magic(P)`` built on
  the host into InstDesc.p_magic: exact for EVERY 32-bit dividend and divisor >= 1 (the bound is in the header);
* ``small_quotient(i, n, KG)`` for ``i / n_ext`` and ``i / n_tab`` with ``i < KG * n``;
* ``offsets_fit32(bytes)`` to pick 32-bit byte offsets into a prediction tensor below 2 GiB;
* ``spline_index_guess``: the segment an even knot spacing would give, accepted only if it is the segment, otherwise
  the bisection -- the index of ``spline_index`` for every input and every scale.

tests/emu/fot_cull_index_emu.cpp loops the header's own functions.  Ranges: the library takes at most 65534 * 8 obstacle
points per instance (fot_setup.hpp), so j and P stay below 2^20; n_ext <= FOT_MAX_TI + FOT_MAX_BRAKE = 96 and
n_tab <= CULL_PBOX = 96; KG = 4.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SO = os.path.join(EMU_DIR, "_build", "libfot_cull_index.so")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")

N_MAX = 1 << 20                  # dividends: obstacle indices of one instance
D_MAX = 65534 * 8                # divisors: pedestrians per sample (fot_setup.hpp's limit on points per instance)
u64p = C.POINTER(C.c_uint64)
i64p = C.POINTER(C.c_int64)
f64p = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    srcs = [os.path.join(EMU_DIR, "fot_cull_index_emu.cpp")] + [os.path.join(CSRC, f) for f in ("fot_math.hpp", "fot_types.h")]
    srcs.append(os.path.join(ROOT, "include", "fot.h"))
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SO, srcs[0]],
                       check=True)
    L = C.CDLL(SO)
    L.ci_div_magic.argtypes = [C.c_uint32]; L.ci_div_magic.restype = C.c_uint32
    L.ci_div.argtypes = [C.c_uint32, C.c_uint32]; L.ci_div.restype = C.c_uint32
    L.ci_div_check_range.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, u64p]; L.ci_div_check_range.restype = C.c_int64
    L.ci_div_check_multiples.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, u64p, u64p, i64p]
    L.ci_div_check_multiples.restype = C.c_int64
    L.ci_small_quotient_check.argtypes = [C.c_int, C.c_int]; L.ci_small_quotient_check.restype = C.c_int64
    L.ci_offsets_fit32.argtypes = [C.c_int64]; L.ci_offsets_fit32.restype = C.c_int
    L.ci_spline_guess_check.argtypes = [C.c_int, f64p, C.c_int64, f64p, C.c_float, i64p]
    L.ci_spline_guess_check.restype = C.c_int64
    return L


def test_magic_division_is_exact_for_small_divisors_exhaustively(lib):
    """Divisors 1..64 (and the power of two and the prime next to it), every dividend 0 .. 2^20 - 1."""
    for d in list(range(1, 65)) + [127, 128, 4093, 4096, 4099]:
        first = C.c_uint64(0)
        bad = lib.ci_div_check_range(d, 0, N_MAX, C.byref(first))
        assert bad == 0, f"{bad} wrong quotients for divisor {d}, first at dividend {first.value}"


def test_magic_division_is_exact_at_the_multiples_of_every_divisor(lib):
    """Every divisor the limits allow for P (and with it every n_tv, n_ext, n_tab), dividends 0 .. 2^20 - 1 at the
    multiples of the divisor and one either side -- where a quotient one too small or one too large shows."""
    fd, fn, cnt = C.c_uint64(0), C.c_uint64(0), C.c_int64(0)
    bad = lib.ci_div_check_multiples(1, D_MAX, N_MAX, C.byref(fd), C.byref(fn), C.byref(cnt))
    assert cnt.value > 30_000_000                              # (~ 3 * 2^20 * ln(2^20) pairs)
    assert bad == 0, f"{bad} wrong quotients, first: {fn.value} / {fd.value}"


def test_magic_division_holds_over_the_whole_32_bit_range(lib):
    """The bound in the header does not depend on the dividend's size: the top of the 32-bit range, divisors 1, 2, 3,
    primes, powers of two and 2^32 - 1, and random pairs."""
    top = 1 << 32
    for d in (1, 2, 3, 7, 13, 29, 641, 65536, 65537, (1 << 20) - 1, 1 << 20, (1 << 31) - 1, 1 << 31, top - 1):
        first = C.c_uint64(0)
        assert lib.ci_div_check_range(d, top - 200_000, top, C.byref(first)) == 0, (d, first.value)
        assert lib.ci_div_check_range(d, 0, 200_000, C.byref(first)) == 0, (d, first.value)
        for q in range(0, top // d, max(1, top // d // 1000)):             # multiples +- 1 across the range
            for n in (q * d - 1, q * d, q * d + 1):
                if 0 <= n < top:
                    assert lib.ci_div(n, d) == n // d, (n, d)
    rng = np.random.default_rng(26)
    n = rng.integers(0, top, 200_000, dtype=np.uint64)
    d = np.maximum(rng.integers(0, top, 200_000, dtype=np.uint64) >> rng.integers(0, 32, 200_000, dtype=np.uint64), 1)
    for a, b in zip(n.tolist(), d.tolist()):
        assert lib.ci_div(a, b) == a // b, (a, b)
    assert lib.ci_div_magic(1) == 0xFFFFFFFF and lib.ci_div_magic(2) == 1 << 31 and lib.ci_div_magic(3) == 0x55555555


def test_small_quotient_is_the_quotient_below_kg_multiples(lib):
    """i / n for every i < KG * n, n = 1 .. 1024 (k_cull: n <= 96), KG = 1 .. 8 (k_cull: 4)."""
    for kg in range(1, 9):
        for n in range(1, 1025):
            assert lib.ci_small_quotient_check(n, kg) == 0, (n, kg)


def test_the_32_bit_offset_form_ends_at_two_gib(lib):
    assert lib.ci_offsets_fit32((1 << 31) - 1) == 1
    assert lib.ci_offsets_fit32(1 << 31) == 0
    assert lib.ci_offsets_fit32((1 << 31) + 1) == 0
    assert lib.ci_offsets_fit32(0) == 1 and lib.ci_offsets_fit32(245_000) == 1
    # the largest tensor the limits allow does not fit: 2^20 obstacles x 128 steps of float64 points
    assert lib.ci_offsets_fit32((1 << 20) * 128 * 16) == 0 and lib.ci_offsets_fit32((1 << 20) * 128 * 8 - 8) == 1


def _knot_sets():
    rng = np.random.default_rng(2600)
    yield "even", np.arange(0.0, 61.0, 1.0)
    yield "two knots", np.array([0.0, 10.0])
    yield "even, offset origin", 1234.5 + 0.37 * np.arange(513)
    yield "uneven", np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 3.0, 200))])
    yield "repeated knots", np.sort(np.concatenate([np.arange(0.0, 20.0, 0.5), [3.0, 3.0, 7.5]]))
    yield "one long segment", np.concatenate([np.arange(0.0, 10.0, 0.1), [1000.0]])


@pytest.mark.parametrize("name,knots", list(_knot_sets()), ids=[k[0] for k in _knot_sets()])
def test_guessed_segment_is_the_bisection_s_segment(lib, name, knots):
    """Arguments on every knot, one float64 step either side of it, mid-segment and random, with the path's own scale
    and with useless ones (0, far too large, NaN): the index is spline_index's.  On an evenly sampled path nearly all
    lookups are settled by the guess (otherwise the shortcut would be dead code)."""
    s = np.ascontiguousarray(knots, np.float64)
    rng = np.random.default_rng(len(s))
    v = np.concatenate([s, np.nextafter(s, -np.inf), np.nextafter(s, np.inf), 0.5 * (s[1:] + s[:-1]),
                        rng.uniform(s[0], s[-1], 20_000)])
    v = np.ascontiguousarray(np.clip(v, s[0], s[-1]))
    for scale in (-1.0, 0.0, 1e9, float("nan"), 1e-9):
        acc = C.c_int64(0)
        bad = lib.ci_spline_guess_check(len(s), s.ctypes.data_as(f64p), len(v), v.ctypes.data_as(f64p), scale, C.byref(acc))
        assert bad == 0, f"{name}, scale {scale}: {bad} of {len(v)} indices differ from spline_index"
        if scale == -1.0 and name.startswith("even"):
            assert acc.value > 0.95 * len(v), (name, acc.value, len(v))
