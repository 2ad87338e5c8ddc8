// fot_fidelity.hpp -- the fidelity statistics of vehicle-pedestrian encounters (fot_fidelity_eval; the reference's
// min_separation_series and avoidance_onset_distance of src/core/metrics.py and the error of objective_rollout_ade /
// fidelity_report of src/simulation/calibration_harness.py), shared between the kernels k_fidelity_peds /
// k_fidelity_series / k_fidelity_fold, the host (the table checks) and tests/emu/fot_fidelity_emu.cpp.  Plain C++,
// float64 throughout.
//
// An encounter is T steps of an ego position and of N pedestrians, [T][N][2].  Per step: the smallest ego-pedestrian
// distance (the separation series).  Per pedestrian: the first step at which it accelerates away from the ego while in
// range (the avoidance onset) and the distance there; against a second position array, its summed distance to that
// array over the steps 1 .. T-1 and whether its truth-side distance to the ego ever falls to interaction_distance.  Per
// encounter: the series' minimum and its first step, the onsets, the kept pedestrians' error sum and count.
//
// The arithmetic is NumPy's, operation by operation: np.linalg.norm(axis=2) squares, squares, adds and roots;
// np.gradient(f, dt, axis=0) divides central differences by 2 dt and the one-sided ends by dt; np.min keeps a NaN.
// Every product, sum and quotient is rounded on its own -- nothing here may contract into a fused multiply-add, and
// no division becomes a multiplication by a reciprocal.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FOT_FID_HD __host__ __device__ inline
#else
#define FOT_FID_HD inline
#endif

namespace fot {

constexpr double FID_MIN_DIST = 1e-9;            // avoidance_onset_distance: a pedestrian on the ego is skipped

// fot_fidelity_params / fot_fidelity_enc (include/fot.h)
struct FidParams { double accel_threshold, max_distance, interaction_distance; };
struct FidEnc {
    double closest, err_sum;
    int64_t err_count;
    int32_t n_onset, closest_step;
};

constexpr int FID_OK = 0;
constexpr int FID_BAD_INVALID = 1;               // FOT_ERR_INVALID

// ---- the checks: 0, or FID_BAD_INVALID with *why naming the rule ------------------------------------------------------------
inline int fid_check_params(const FidParams &p, const char **why)
{
    if (std::isnan(p.accel_threshold) || std::isnan(p.max_distance)) { *why = "accel_threshold or max_distance is NaN"; return FID_BAD_INVALID; }
    return FID_OK;
}

// step_off [n_enc + 1] from 0 and increasing; n_ped [n_enc] not negative; dt [n_enc] finite and positive
inline int fid_check_tables(int64_t n_enc, const int32_t *step_off, const int32_t *n_ped, const double *dt, const char **why)
{
    if (n_enc < 0) { *why = "n_enc is negative"; return FID_BAD_INVALID; }
    if (!step_off || !n_ped || !dt) { *why = "step_off / n_ped / dt is NULL"; return FID_BAD_INVALID; }
    if (step_off[0] != 0) { *why = "step_off does not start at 0"; return FID_BAD_INVALID; }
    for (int64_t e = 0; e < n_enc; ++e) {
        const int64_t n = (int64_t)step_off[e + 1] - step_off[e];
        if (n < 0) { *why = "step_off decreases"; return FID_BAD_INVALID; }
        if (n == 0) { *why = "an encounter of 0 steps"; return FID_BAD_INVALID; }
        if (n_ped[e] < 0) { *why = "n_ped is negative"; return FID_BAD_INVALID; }
        if (!(dt[e] > 0.0) || !std::isfinite(dt[e])) { *why = "dt is not finite and positive"; return FID_BAD_INVALID; }
    }
    return FID_OK;
}

// ---- the pieces ---------------------------------------------------------------------------------------------------------------
// np.linalg.norm(axis=2): sqrt(dx dx + dy dy), the squares summed, then rooted (sum_sq_unfused of fot_math.hpp)
FOT_FID_HD double fid_dist(double dx, double dy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = dx * dx, b = dy * dy;
    return sqrt(a + b);
}

// np.min of two: a NaN on either side stays (fmin would drop it)
FOT_FID_HD double fid_min(double a, double b) { return (a < b || a != a) ? a : b; }

// np.gradient(f, dt, axis=0) at step t of T >= 2: one-sided at both ends, central inside
template <typename F>
FOT_FID_HD double fid_gradient(const F &f, int t, int T, double dt)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (t == 0) return (f(1) - f(0)) / dt;
    if (t == T - 1) return (f(T - 1) - f(T - 2)) / dt;
    const double two_dt = 2.0 * dt;
    return (f(t + 1) - f(t - 1)) / two_dt;
}

// the same rule on a window of three values (the velocity's: before, here, after)
FOT_FID_HD double fid_gradient3(double before, double here, double after, int t, int T, double dt)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (t == 0) return (after - here) / dt;
    if (t == T - 1) return (here - before) / dt;
    const double two_dt = 2.0 * dt;
    return (after - before) / two_dt;
}

// the acceleration's component along the ego -> pedestrian direction: acc . (rel / dist), the two products rounded
// apart.  dist is neither 0 nor beyond the range when this is called.
FOT_FID_HD double fid_away(double ax, double ay, double rx, double ry, double dist)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ux = rx / dist, uy = ry / dist;
    const double a = ax * ux, b = ay * uy;
    return a + b;
}

// the reference's `continue`, negated: a NaN distance is NOT skipped (its away is NaN and never an onset)
FOT_FID_HD bool fid_in_range(double dist, double max_distance) { return !(dist < FID_MIN_DIST) && !(dist > max_distance); }

// ---- a pedestrian's onset: the first step, ascending, in range and with away > accel_threshold --------------------------------
// pos(t, c), ego(t, c): coordinate c of step t.  vel(t, c): the caller's velocity, or the gradient of the positions
// (fid_gradient over pos).  A window of three velocities slides along; every step forms one new velocity.  *away_out:
// the value that crossed the threshold (NaN without an onset).  T < 2: no onset.
template <typename Pos, typename Vel, typename Ego>
FOT_FID_HD void fid_onset(const Pos &pos, const Vel &vel, const Ego &ego, int T, double dt, const FidParams &p,
                          int32_t *step_out, double *dist_out, double *away_out)
{
    *step_out = -1; *dist_out = NAN; *away_out = NAN;
    if (T < 2) return;
    double vbx = 0.0, vby = 0.0, vx = vel(0, 0), vy = vel(0, 1), vax = vel(1, 0), vay = vel(1, 1);
    for (int t = 0; t < T; ++t) {
        const double rx = pos(t, 0) - ego(t, 0), ry = pos(t, 1) - ego(t, 1);
        const double dist = fid_dist(rx, ry);
        if (fid_in_range(dist, p.max_distance)) {
            const double ax = fid_gradient3(vbx, vx, vax, t, T, dt), ay = fid_gradient3(vby, vy, vay, t, T, dt);
            const double away = fid_away(ax, ay, rx, ry, dist);
            if (away > p.accel_threshold) { *step_out = t; *dist_out = dist; *away_out = away; return; }
        }
        vbx = vx; vby = vy; vx = vax; vy = vay;
        if (t + 2 < T) { vax = vel(t + 2, 0); vay = vel(t + 2, 1); }
    }
}

// ---- a pedestrian's roll-out error against the truth: the distances of the steps 1 .. T-1 summed in ascending order, and
// whether the pedestrian is kept: interaction_distance NaN keeps all, else min_t |truth - ego| <= interaction_distance
// (the minimum as np.min forms it: a NaN distance leaves the pedestrian out)
template <typename Pos, typename Truth, typename Ego>
FOT_FID_HD void fid_ped_error(const Pos &pos, const Truth &truth, const Ego &ego, int T, double interaction_distance,
                              double *sum_out, int32_t *keep_out)
{
    double sum = 0.0, nearest = INFINITY;
    for (int t = 0; t < T; ++t) {
        const double qx = truth(t, 0), qy = truth(t, 1);
        nearest = fid_min(nearest, fid_dist(qx - ego(t, 0), qy - ego(t, 1)));
        if (t >= 1) sum = sum + fid_dist(pos(t, 0) - qx, pos(t, 1) - qy);
    }
    *sum_out = sum;
    *keep_out = (interaction_distance != interaction_distance) || nearest <= interaction_distance ? 1 : 0;
}

// ---- a step's separation: the minimum over its n pedestrians in ascending order, +inf without any --------------------------------
template <typename Row>
FOT_FID_HD double fid_separation(const Row &row, int n, double ex, double ey)
{
    double m = INFINITY;
    for (int j = 0; j < n; ++j) m = fid_min(m, fid_dist(row(j, 0) - ex, row(j, 1) - ey));
    return m != m ? (double)NAN : m;
}

// ---- the fold of an encounter -----------------------------------------------------------------------------------------------
// the series' minimum with its first step: (value, step) pairs ordered by value, then by step; a NaN anywhere makes the
// minimum NaN and the step -1.  Exact in any order of the joins.
struct FidMin { double v; int32_t step, nan; };
FOT_FID_HD FidMin fid_min_zero() { FidMin m; m.v = INFINITY; m.step = -1; m.nan = 0; return m; }
FOT_FID_HD FidMin fid_min_take(FidMin m, double v, int32_t step)
{
    if (v != v) { m.nan = 1; return m; }
    if (v < m.v || (v == m.v && (m.step < 0 || step < m.step))) { m.v = v; m.step = step; }
    return m;
}
FOT_FID_HD FidMin fid_min_join(FidMin a, const FidMin &b)
{
    a.nan |= b.nan;
    if (b.step >= 0 && (b.v < a.v || (b.v == a.v && (a.step < 0 || b.step < a.step)))) { a.v = b.v; a.step = b.step; }
    return a;
}

// the record: the kept pedestrians' sums added in ascending pedestrian order (one fixed order, no atomics); without
// pedestrians the series is all +inf and no step holds the minimum
template <typename Sum, typename Keep, typename Step>
FOT_FID_HD FidEnc fid_record(const FidMin &m, int T, int n, bool have_truth, const Sum &ped_sum, const Keep &ped_keep,
                             const Step &onset_step)
{
    FidEnc r;
    r.closest = m.nan ? (double)NAN : m.v;
    r.closest_step = (m.nan || n == 0) ? -1 : m.step;
    r.err_sum = 0.0; r.err_count = 0; r.n_onset = 0;
    int64_t kept = 0;
    for (int j = 0; j < n; ++j) {
        r.n_onset += onset_step(j) >= 0 ? 1 : 0;
        if (have_truth && ped_keep(j)) { r.err_sum = r.err_sum + ped_sum(j); ++kept; }
    }
    r.err_count = have_truth ? (int64_t)(T - 1) * kept : 0;
    return r;
}

}  // namespace fot
