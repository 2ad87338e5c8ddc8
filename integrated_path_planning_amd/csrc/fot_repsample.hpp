// fot_repsample.hpp -- planning on the representative prediction sample (fot_loop_plan_sample,
// FOT_LOOP_PLAN_REPRESENTATIVE): the step from "index of the chosen sample" (fot_loopscore.hpp) to the single-sample
// block the plan kernels read.  Plain C++ shared by the kernel (k_loop_rep_block), the host and
// tests/emu/fot_repsample_emu.cpp.
//
// The reference leads the chosen sample with the current positions unless np.allclose(pred[:, 0], current)
// (integrated_simulator.py:508-513), so its tensor has n_dense or n_dense + 1 time entries depending on the sample's
// numbers.  Here every episode's block is [P][n_dense + 1][2] whatever the decision:
//   prepended      [current, dense[0], ..., dense[n_dense - 1]]
//   not prepended  [dense[0], ..., dense[n_dense - 1], dense[n_dense - 1]]      (the last entry once more)
// The second form is the same obstacle to the planner as the reference's [P][n_dense][2]: the collision check clips its
// time index to the last entry (frenet_planner.py:1226-1227), and a track's min / max box and its NaN rule do not see a
// repeated entry.
#pragma once

#include <cmath>
#include <cstdint>

#include "fot_predscore.hpp"

namespace fot {

constexpr double RS_ATOL = 1e-8, RS_RTOL = 1e-5;     // np.allclose's defaults

// one coordinate of np.allclose(first, cur): |first - cur| <= atol + rtol |cur|, product and sum rounded one by one; a NaN
// on either side makes it false
FOT_PS_HD bool rs_close(double first, double cur)
{
#pragma clang fp contract(off)
    const double d = std::fabs(first - cur);
    const double r = RS_RTOL * std::fabs(cur);
    return d <= RS_ATOL + r;
}

// a pedestrian's first dense sample against its current position, both axes
FOT_PS_HD bool rs_close_xy(double fx, double fy, double cx, double cy)
{
    return rs_close(fx, cx) && rs_close(fy, cy);
}

// Entry t of a block of T = n_dense + 1 entries comes from entry rs_src(t, T, prepend) of the chosen sample's track in the
// distribution block, whose entry 0 is the current position and whose entries 1 .. n_dense are the dense samples.
FOT_PS_HD int rs_src(int t, int T, bool prepend)
{
    if (prepend) return t;
    return t + 1 < T ? t + 1 : T - 1;
}

// An episode's rule evaluated sequentially: first / cur [P][2].  True: the current positions lead the block.
inline bool rs_episode_prepend(int P, const double *first, const double *cur)
{
    bool close = true;
    for (int p = 0; p < P; ++p)
        close = rs_close_xy(first[2 * p], first[2 * p + 1], cur[2 * p], cur[2 * p + 1]) && close;
    return !close;
}

// The block of an episode from its chosen sample's tracks, track [P][T][2] (entry 0: the current position), out [P][T][2].
// The host-side form of k_loop_rep_block; returns the prepend flag.
inline bool rs_build_block(int P, int T, const double *track, const double *cur, double *out)
{
    bool close = true;
    for (int p = 0; p < P; ++p) {
        const double *f = track + ((size_t)p * T + 1) * 2;
        close = rs_close_xy(f[0], f[1], cur[2 * p], cur[2 * p + 1]) && close;
    }
    const bool prepend = !close;
    for (int p = 0; p < P; ++p)
        for (int t = 0; t < T; ++t) {
            const double *s = track + ((size_t)p * T + rs_src(t, T, prepend)) * 2;
            double *o = out + ((size_t)p * T + t) * 2;
            if (prepend && t == 0) s = cur + 2 * p;
            o[0] = s[0]; o[1] = s[1];
        }
    return prepend;
}

}  // namespace fot
