// fot_encounter.hpp -- cutting vehicle-pedestrian encounters out of a recorded clip (fot_encounters_extract; the reference's
// _ped_velocities and extract_encounters of src/datasets/vci_encounter.py and _cruise_speeds, cruise_upper_quantile,
// cruise_freewalk, _floor and _far_goals of src/simulation/calibration_harness.py), shared between the kernels
// k_enc_columns / k_enc_compact / k_enc_gather / k_enc_rows, the host (the checks, the candidate spans) and
// tests/emu/fot_encounter_emu.cpp.  Plain C++, float64 throughout, on top of fot_fidelity.hpp's distance and minimum.
//
// A clip is a pedestrian scene [T][A][2] (NaN where a pedestrian is absent), optionally its recorded velocities, and K
// vehicles aligned onto the scene's grid ([K][T] channels, NaN outside a vehicle's support).  A candidate span is a maximal
// run of frames at which all four channels of one vehicle are finite.  Per span: the pedestrians without a NaN position or
// velocity component anywhere in it (the kept columns, ascending), the smallest ego-pedestrian distance over [L][N] with
// its first step and column in row-major order, and per kept pedestrian the boundary conditions of a roll-out (cruise
// speed, far goal).
//
// The arithmetic is NumPy's, operation by operation; nothing here may contract into a fused multiply-add.
#pragma once

#include <cmath>
#include <cstdint>

#include "fot_fidelity.hpp"

namespace fot {

constexpr int ENC_SHORT = 0, ENC_NO_PEDS = 1, ENC_FAR = 2, ENC_KEPT = 3;                  // FOT_ENC_* statuses
constexpr int ENC_CRUISE_NONE = 0, ENC_CRUISE_MEDIAN = 1, ENC_CRUISE_QUANTILE = 2, ENC_CRUISE_FREEWALK = 3;
constexpr int ENC_SCENE_DEVICE = 1, ENC_MEASURE_REAL = 2, ENC_ALL_FLAGS = 3;
constexpr double ENC_FLOOR = 1e-3;               // _floor, and _far_goals' "barely moving"
constexpr int ENC_COL_TILE = 64;                 // k_enc_columns: columns of a block (lane = column)
constexpr int ENC_STEP_WAVES = 4;                // ... and the waves that share a span's steps (wave w: steps w, w + 4, ...)

// fot_encounter_params / fot_encounter_span (include/fot.h)
struct EncParams {
    double min_sep_threshold, dt, accel_threshold, max_distance, cruise_q, free_distance, goal_distance;
    int32_t min_len, cruise_mode, flags, pad_;
};
struct EncSpan {
    double min_separation;
    FidEnc real;
    int64_t row_base;
    int32_t status, vehicle, frame0, frame1, n_ped, min_step, min_col, pad_;
};

// ---- the checks: 0, or FID_BAD_INVALID with *why naming the rule ------------------------------------------------------------
inline int enc_check_params(const EncParams &p, const char **why)
{
    if (!(p.dt > 0.0) || !std::isfinite(p.dt)) { *why = "dt is not finite and positive"; return FID_BAD_INVALID; }
    if (p.min_len < 1) { *why = "min_len < 1"; return FID_BAD_INVALID; }
    if (std::isnan(p.min_sep_threshold) || std::isnan(p.accel_threshold) || std::isnan(p.max_distance)) {
        *why = "min_sep_threshold, accel_threshold or max_distance is NaN"; return FID_BAD_INVALID;
    }
    if (p.cruise_mode < ENC_CRUISE_NONE || p.cruise_mode > ENC_CRUISE_FREEWALK) { *why = "unknown cruise_mode"; return FID_BAD_INVALID; }
    if (p.flags & ~ENC_ALL_FLAGS) { *why = "unknown flag"; return FID_BAD_INVALID; }
    if (p.cruise_mode >= ENC_CRUISE_QUANTILE && !(p.cruise_q >= 0.0 && p.cruise_q <= 1.0)) { *why = "cruise_q outside [0, 1]"; return FID_BAD_INVALID; }
    if (p.cruise_mode == ENC_CRUISE_FREEWALK && std::isnan(p.free_distance)) { *why = "free_distance is NaN"; return FID_BAD_INVALID; }
    if (p.cruise_mode != ENC_CRUISE_NONE && std::isnan(p.goal_distance)) { *why = "goal_distance is NaN"; return FID_BAD_INVALID; }
    return FID_OK;
}

// ---- the candidate spans of vehicle k (host): the maximal runs of frames with x, y, psi and vel all finite, start
// ascending.  emit(frame0, frame1): frame1 is one past the run's last frame
template <typename Emit>
inline void enc_find_spans(int32_t T, const double *xy, const double *psi, const double *vel, const Emit &emit)
{
    int32_t start = -1;
    for (int32_t t = 0; t < T; ++t) {
        const bool here = std::isfinite(xy[2 * (int64_t)t]) && std::isfinite(xy[2 * (int64_t)t + 1]) && std::isfinite(psi[t]) &&
                          std::isfinite(vel[t]);
        if (here && start < 0) start = t;
        else if (!here && start >= 0) { emit(start, t); start = -1; }
    }
    if (start >= 0) emit(start, T);
}

// ---- the pieces ---------------------------------------------------------------------------------------------------------------
// _ped_velocities' fallback at frame t of the WHOLE grid: the forward difference, the last frame repeating the one
// before it; all NaN on a grid of one frame.  pos(t, c): coordinate c of the pedestrian at frame t
template <typename Pos>
FOT_FID_HD double enc_fallback_vel(const Pos &pos, int32_t t, int32_t T, int c, double dt)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (T < 2) return (double)NAN;
    const int32_t s = t < T - 1 ? t : T - 2;
    return (pos(s + 1, c) - pos(s, c)) / dt;
}

// one column's walk over the steps first, first + stride, ... < L of a span: whether any position or velocity component
// is NaN (isnan: an infinity is not absence), and the smallest distance to the ego with its first step.
// pos / vel / ego (step, c): step counts from the span's first frame
struct EncCol { FidMin m; int32_t absent; };
template <typename Pos, typename Vel, typename Ego>
FOT_FID_HD EncCol enc_column(const Pos &pos, const Vel &vel, const Ego &ego, int32_t first, int32_t stride, int32_t L)
{
    EncCol c; c.m = fid_min_zero(); c.absent = 0;
    for (int32_t t = first; t < L; t += stride) {
        const double px = pos(t, 0), py = pos(t, 1), vx = vel(t, 0), vy = vel(t, 1);
        c.absent |= (px != px || py != py || vx != vx || vy != vy) ? 1 : 0;
        c.m = fid_min_take(c.m, fid_dist(px - ego(t, 0), py - ego(t, 1)), t);
    }
    return c;
}
FOT_FID_HD EncCol enc_column_join(EncCol a, const EncCol &b) { a.absent |= b.absent; a.m = fid_min_join(a.m, b.m); return a; }

// the minimum over [L][N] with its first (step, column) in row-major order: (value, step, column) triples ordered by
// value, then step, then column; a NaN anywhere makes the minimum NaN (np.min) and step and column -1.  Exact in any
// order of the joins.
struct EncMin { double v; int32_t step, col, nan; };
FOT_FID_HD EncMin enc_min_zero() { EncMin m; m.v = INFINITY; m.step = -1; m.col = -1; m.nan = 0; return m; }
FOT_FID_HD EncMin enc_min_join(EncMin a, const EncMin &b)
{
    a.nan |= b.nan;
    if (b.col >= 0 && b.step >= 0 &&
        (a.col < 0 || b.v < a.v || (b.v == a.v && (b.step < a.step || (b.step == a.step && b.col < a.col))))) {
        a.v = b.v; a.step = b.step; a.col = b.col;
    }
    return a;
}
FOT_FID_HD EncMin enc_min_of_column(const FidMin &m, int32_t col)
{
    EncMin r; r.v = m.v; r.step = m.step; r.col = m.step >= 0 ? col : -1; r.nan = m.nan; return r;
}

// a span's status from its population and closest approach: equality with the threshold keeps the span, and so does a NaN
FOT_FID_HD int enc_status(int32_t n_ped, double min_separation, double threshold)
{
    if (n_ped == 0) return ENC_NO_PEDS;
    return min_separation > threshold ? ENC_FAR : ENC_KEPT;
}

// ---- order statistics by counting: the rank of entry i among the non-NaN entries of v[0 .. L), ties broken by index.
// The ranks of the n non-NaN entries are 0 .. n-1, each once.  v(i): entry i
template <typename V>
FOT_FID_HD int32_t enc_rank(const V &v, int32_t i, int32_t L)
{
    const double x = v(i);
    int32_t r = 0;
    for (int32_t j = 0; j < L; ++j) { const double y = v(j); r += (y < x || (y == x && j < i)) ? 1 : 0; }
    return r;
}

// which order statistics of n >= 1 sorted values s a cruise speed needs (lo <= hi <= lo + 1), and its value from them
struct EncPick { int32_t lo, hi; double g; };
FOT_FID_HD EncPick enc_pick_median(int32_t n) { EncPick p; p.hi = n / 2; p.lo = (n & 1) ? p.hi : p.hi - 1; p.g = 0.0; return p; }
// np.quantile's linear method: v = q (n - 1), lo = floor(v), g = v - lo; the entry above is clipped to the last one
FOT_FID_HD EncPick enc_pick_quantile(int32_t n, double q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    EncPick p;
    const double v = (double)(n - 1) * q, fl = floor(v);
    p.lo = (int32_t)fl;
    if (p.lo >= n - 1) { p.lo = n - 1; p.hi = n - 1; } else p.hi = p.lo + 1;
    p.g = v - fl;
    return p;
}
// np.median: the middle entry, or the mean of the two middle ones
FOT_FID_HD double enc_median_value(int32_t n, double s_lo, double s_hi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (n & 1) ? s_lo : (s_lo + s_hi) / 2.0;
}
// np.quantile's _lerp: s_lo + d g below g = 0.5, s_hi - d (1 - g) from there on; s_lo where the two are equal
FOT_FID_HD double enc_quantile_value(double s_lo, double s_hi, double g)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = s_hi - s_lo;
    if (d == 0.0) return s_lo;
    if (g < 0.5) { const double a = d * g; return s_lo + a; }
    const double w = 1.0 - g, b = d * w;
    return s_hi - b;
}
// _floor: a cruise speed that is not finite or not above 1e-3 becomes 1e-3
FOT_FID_HD double enc_floor(double c) { return (c - c == 0.0 && c > ENC_FLOOR) ? c : ENC_FLOOR; }

// _far_goals: goal_distance ahead of the first position along the net displacement; a net displacement shorter than 1e-3
// gives way to the first velocity if that is longer than 1e-3, else to +x.  The chosen vector is divided by its own norm
FOT_FID_HD void enc_goal(double x0, double y0, double x1, double y1, double vx0, double vy0, double distance, double *gx, double *gy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double hx = x1 - x0, hy = y1 - y0;
    double norm = fid_dist(hx, hy);
    if (norm < ENC_FLOOR) {
        const double vn = fid_dist(vx0, vy0);
        if (vn > ENC_FLOOR) { hx = vx0; hy = vy0; norm = vn; } else { hx = 1.0; hy = 0.0; norm = 1.0; }
    }
    const double ux = hx / norm, uy = hy / norm;
    const double ax = ux * distance, ay = uy * distance;
    *gx = x0 + ax; *gy = y0 + ay;
}

}  // namespace fot
