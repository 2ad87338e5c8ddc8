// fot_footprint_obs.hpp -- the observational footprint re-verification of episodes (fot_footprint_recheck; the reference's
// examples/recheck_footprint.py and observational_footprint_metrics of examples/run_footprint_benchmark.py), shared between
// the kernels k_footprint_steps / k_footprint_yaw / k_footprint_fold, the host (the geometry, the table checks) and
// tests/emu/fot_footprint_obs_emu.cpp.  Plain C++, float64 throughout.
//
// Every step of a trajectory -- a pose (x, y, yaw) and that step's P pedestrians -- is measured against three geometries
// that do not depend on what the planner used: the centre (legacy), an n-circle cover of the L x W rectangle (multi) and
// the exact oriented rectangle (rect).  A trajectory's record holds the minima over its steps and, per geometry, the
// number of steps strictly below its threshold.  A step without pedestrians measures +inf three times and counts nowhere.
//
// The arithmetic is NumPy's, operation by operation (footprint.py:38-65): np.linalg.norm(axis=...) sums the squares and
// roots the sum; the circle centres are x + off_k cos yaw; the vehicle frame is a 2 x 2 product; the rectangle distance is
// np.hypot.  Every product and sum is rounded on its own: nothing here may contract into a fused multiply-add.
// Non-finite coordinates: unspecified (fmin drops a NaN where np.min keeps it).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FOT_FPO_HD __host__ __device__ inline
#else
#define FOT_FPO_HD inline
#endif

namespace fot {

constexpr int FPO_MAX_CIRCLES = 8;               // FOT_MAX_CIRCLES
constexpr double FPO_MOVING_EPS = 1e-4;          // reconstruct_yaw: a step moves when hypot(dx, dy) > 1e-4

// fot_footprint_step / fot_footprint_obs (include/fot.h)
struct FpoStep { double legacy, multi, rect; };
struct FpoRecord {
    double legacy_min_dist, multi_min_dist, multi_clearance, rect_min_surface_dist, rect_clearance;
    int32_t legacy_collision_steps, multi_violation_steps, rect_violation_steps, steps, steps_with_peds, _pad;
};

// the geometry as the kernels take it: half extents, the circle offsets and the three thresholds
struct FpoGeom {
    double half_l, half_w;
    double off[FPO_MAX_CIRCLES];
    double radius;                               // hypot(seg / 2, W / 2): EgoFootprint.multi_circle
    double thr_legacy, thr_multi, thr_rect;      // legacy_radius | radius + ped_radius | ped_radius
    int32_t n_circles, _pad;
};

constexpr int FPO_OK = 0;
constexpr int FPO_BAD_INVALID = 1;               // FOT_ERR_INVALID

// ---- the geometry (host): EgoFootprint.multi_circle's offsets and radius --------------------------------------------------
inline int fpo_check_geom(double L, double W, double ped_radius, double legacy_radius, int n_circles, const char **why)
{
    if (!(L > 0.0) || !(W > 0.0) || !std::isfinite(L) || !std::isfinite(W)) { *why = "vehicle_length and vehicle_width must be positive"; return FPO_BAD_INVALID; }
    if (!(ped_radius >= 0.0) || !(legacy_radius >= 0.0) || !std::isfinite(ped_radius) || !std::isfinite(legacy_radius)) { *why = "a radius is negative"; return FPO_BAD_INVALID; }
    if (n_circles < 1 || n_circles > FPO_MAX_CIRCLES) { *why = "n_circles lies outside 1 .. FOT_MAX_CIRCLES"; return FPO_BAD_INVALID; }
    return FPO_OK;
}

inline FpoGeom fpo_geom(double L, double W, double ped_radius, double legacy_radius, int n_circles)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    FpoGeom g{};
    const double seg = L / (double)n_circles;
    const double a = -L / 2.0, b = seg / 2.0, first = a + b;
    for (int k = 0; k < FPO_MAX_CIRCLES; ++k) {
        const double step = seg * (double)k;
        g.off[k] = k < n_circles ? first + step : 0.0;
    }
    g.half_l = L / 2.0; g.half_w = W / 2.0;
    g.radius = std::hypot(b, g.half_w);
    g.thr_legacy = legacy_radius; g.thr_multi = g.radius + ped_radius; g.thr_rect = ped_radius;
    g.n_circles = n_circles;
    return g;
}

// ---- the tables: 0, or FPO_BAD_INVALID with *why naming the rule ------------------------------------------------------------
// step_off [n_traj + 1] from 0, every trajectory at least one step (two when its heading is reconstructed)
inline int fpo_check_steps(int64_t n_traj, const int32_t *step_off, bool have_yaw, const char **why)
{
    if (n_traj < 0) { *why = "n_traj is negative"; return FPO_BAD_INVALID; }
    if (!step_off) { *why = "step_off is NULL"; return FPO_BAD_INVALID; }
    if (step_off[0] != 0) { *why = "step_off does not start at 0"; return FPO_BAD_INVALID; }
    for (int64_t t = 0; t < n_traj; ++t) {
        const int64_t n = (int64_t)step_off[t + 1] - step_off[t];
        if (n < 0) { *why = "step_off decreases"; return FPO_BAD_INVALID; }
        if (n == 0) { *why = "a trajectory of 0 steps"; return FPO_BAD_INVALID; }
        if (n == 1 && !have_yaw) { *why = "a trajectory of 1 step needs its yaw: the gradient takes two"; return FPO_BAD_INVALID; }
    }
    return FPO_OK;
}

// ped_off [steps + 1] non-decreasing from 0
inline int fpo_check_peds(int64_t steps, const int32_t *ped_off, const char **why)
{
    if (!ped_off) { *why = "ped_off is NULL"; return FPO_BAD_INVALID; }
    if (ped_off[0] != 0) { *why = "ped_off does not start at 0"; return FPO_BAD_INVALID; }
    for (int64_t i = 0; i < steps; ++i)
        if (ped_off[i + 1] < ped_off[i]) { *why = "ped_off decreases"; return FPO_BAD_INVALID; }
    return FPO_OK;
}

inline int fpo_check_tables(int64_t n_traj, const int32_t *step_off, const int32_t *ped_off, bool have_yaw, const char **why)
{
    const int bad = fpo_check_steps(n_traj, step_off, have_yaw, why);
    return bad ? bad : fpo_check_peds(step_off[n_traj], ped_off, why);
}

// ---- a step's three values: per pedestrian (legacy, rect) and per (circle, pedestrian) pair (multi) ------------------------
// np.linalg.norm(axis=...): sqrt(dx dx + dy dy), the squares summed, then rooted
FOT_FPO_HD double fpo_norm(double dx, double dy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = dx * dx, b = dy * dy;
    return sqrt(a + b);
}

// circle_centers: x + off cos yaw (and y + off sin yaw)
FOT_FPO_HD double fpo_centre(double x, double off, double h)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = off * h;
    return x + d;
}

FOT_FPO_HD double fpo_legacy(double px, double py, double x, double y) { return fpo_norm(px - x, py - y); }

FOT_FPO_HD double fpo_multi(double px, double py, double cx, double cy) { return fpo_norm(px - cx, py - cy); }

// world_to_vehicle_frame, then rectangle_surface_distance
FOT_FPO_HD double fpo_rect(double px, double py, double x, double y, double c, double s, double half_l, double half_w)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dx = px - x, dy = py - y;
    const double a = dx * c, b = dy * s, e = dx * s, f = dy * c;
    const double lx = a + b, ly = f - e;
    const double ex = fmax(fabs(lx) - half_l, 0.0), ey = fmax(fabs(ly) - half_w, 0.0);
    return hypot(ex, ey);
}

// ---- heading reconstruction (reconstruct_yaw) -----------------------------------------------------------------------------
// np.gradient at unit spacing: one-sided at both ends, (v[i + 1] - v[i - 1]) / 2 inside.  n >= 2.
template <typename V>
FOT_FPO_HD double fpo_gradient(const V &v, int i, int n)
{
    if (i == 0) return v(1) - v(0);
    if (i == n - 1) return v(n - 1) - v(n - 2);
    return (v(i + 1) - v(i - 1)) / 2.0;
}

FOT_FPO_HD bool fpo_moving(double dx, double dy) { return hypot(dx, dy) > FPO_MOVING_EPS; }

// The hold-forward is an inclusive scan over the steps of (source index, its heading) with "the later moving step wins":
// a standing step carries index -1.  Indices grow with the step, so the operator is a maximum of the index.
struct FpoHold { int32_t src; double yaw; };
FOT_FPO_HD FpoHold fpo_hold_join(FpoHold earlier, FpoHold later) { return later.src > earlier.src ? later : earlier; }
// what a step takes: the held heading; in front of the first moving step that first heading; 0 when nothing moves
FOT_FPO_HD double fpo_hold_pick(FpoHold held, bool any_moving, double first_yaw)
{
    return held.src >= 0 ? held.yaw : (any_moving ? first_yaw : 0.0);
}

// ---- the fold of a trajectory: minima and counts, exact in any order --------------------------------------------------------
struct FpoAcc {
    double legacy, multi, rect;
    int32_t n_legacy, n_multi, n_rect, with_peds;
};
FOT_FPO_HD FpoAcc fpo_acc_zero()
{
    FpoAcc a;
    a.legacy = a.multi = a.rect = INFINITY;
    a.n_legacy = a.n_multi = a.n_rect = a.with_peds = 0;
    return a;
}
FOT_FPO_HD void fpo_acc_step(FpoAcc &a, const FpoGeom &g, double legacy, double multi, double rect, bool has_peds)
{
    a.legacy = fmin(a.legacy, legacy); a.multi = fmin(a.multi, multi); a.rect = fmin(a.rect, rect);
    a.n_legacy += legacy < g.thr_legacy ? 1 : 0;
    a.n_multi += multi < g.thr_multi ? 1 : 0;
    a.n_rect += rect < g.thr_rect ? 1 : 0;
    a.with_peds += has_peds ? 1 : 0;
}
FOT_FPO_HD void fpo_acc_merge(FpoAcc &a, const FpoAcc &b)
{
    a.legacy = fmin(a.legacy, b.legacy); a.multi = fmin(a.multi, b.multi); a.rect = fmin(a.rect, b.rect);
    a.n_legacy += b.n_legacy; a.n_multi += b.n_multi; a.n_rect += b.n_rect; a.with_peds += b.with_peds;
}
FOT_FPO_HD FpoRecord fpo_acc_record(const FpoAcc &a, const FpoGeom &g, int32_t steps)
{
    FpoRecord r;
    r.legacy_min_dist = a.legacy;
    r.multi_min_dist = a.multi; r.multi_clearance = a.multi - g.thr_multi;
    r.rect_min_surface_dist = a.rect; r.rect_clearance = a.rect - g.thr_rect;
    r.legacy_collision_steps = a.n_legacy; r.multi_violation_steps = a.n_multi; r.rect_violation_steps = a.n_rect;
    r.steps = steps; r.steps_with_peds = a.with_peds; r._pad = 0;
    return r;
}

}  // namespace fot
