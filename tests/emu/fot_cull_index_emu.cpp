// fot_cull_index_emu.cpp -- TEST-ONLY entry points into the index arithmetic k_cull uses instead of integer divisions
// (csrc/fot_math.hpp: div_magic / div_by_magic, small_quotient, offsets_fit32) and into its segment lookup that starts
// from a guess (spline_index_guess), each checked against the plain form it replaces.  The loops run here, in C++, so
// that tests/test_cull_index_cpu.py can cover whole ranges; it builds this file with g++ into tests/emu/_build/ and
// loads it with ctypes.  Never loaded by the product.
#include <cstdint>

#include "../../integrated_path_planning_amd/csrc/fot_math.hpp"

using namespace fot;

extern "C" {

uint32_t ci_div_magic(uint32_t d) { return div_magic(d); }

uint32_t ci_div(uint32_t n, uint32_t d) { return div_by_magic(n, d, div_magic(d)); }

// dividends [n_lo, n_hi) against divisor d: the number of quotients that differ from n / d, the first such n in *first
int64_t ci_div_check_range(uint32_t d, uint64_t n_lo, uint64_t n_hi, uint64_t *first)
{
    const uint32_t m = div_magic(d);
    int64_t bad = 0;
    for (uint64_t n = n_lo; n < n_hi; ++n)
        if (div_by_magic((uint32_t)n, d, m) != (uint32_t)n / d && bad++ == 0) *first = n;
    return bad;
}

// every divisor in [d_lo, d_hi], dividends below n_max at the multiples of the divisor and one either side of them
int64_t ci_div_check_multiples(uint32_t d_lo, uint32_t d_hi, uint64_t n_max, uint64_t *first_d, uint64_t *first_n, int64_t *checked)
{
    int64_t bad = 0, cnt = 0;
    for (uint64_t d = d_lo; d <= d_hi; ++d) {
        const uint32_t m = div_magic((uint32_t)d);
        for (uint64_t q = 0; q * d <= n_max + d; ++q)
            for (int64_t e = -1; e <= 1; ++e) {
                const int64_t n = (int64_t)(q * d) + e;
                if (n < 0 || (uint64_t)n >= n_max) continue;
                ++cnt;
                if (div_by_magic((uint32_t)n, (uint32_t)d, m) != (uint32_t)n / (uint32_t)d && bad++ == 0) { *first_d = d; *first_n = (uint64_t)n; }
            }
    }
    *checked = cnt;
    return bad;
}

// i / n for every i in [0, kg * n)
int64_t ci_small_quotient_check(int n, int kg)
{
    int64_t bad = 0;
    for (int i = 0; i < kg * n; ++i) bad += small_quotient(i, n, kg) != i / n;
    return bad;
}

int ci_offsets_fit32(int64_t bytes) { return offsets_fit32(bytes) ? 1 : 0; }

// knots s[n]; arguments v[count] inside [s[0], s[n-1]]: lookups whose guess-first index differs from spline_index's;
// *accepted: how many were settled by the guess itself (scale < 0: the path's own spline_guess_scale)
int64_t ci_spline_guess_check(int n, const double *s, int64_t count, const double *v, float scale, int64_t *accepted)
{
    SplineView sp = {};
    sp.s = s; sp.n = n;
    if (scale < 0.0f) scale = spline_guess_scale(sp);
    int64_t bad = 0, acc = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int ref = spline_index(sp, v[i]);
        bad += spline_index_guess(sp, v[i], scale) != ref;
        float gf = (float)(v[i] - s[0]) * scale;
        const float top = (float)(n - 2);
        gf = gf >= 0.0f ? (gf <= top ? gf : top) : 0.0f;
        const int g = (int)gf;
        acc += s[g] <= v[i] && v[i] < s[g + 1];
    }
    *accepted = acc;
    return bad;
}

}  // extern "C"
