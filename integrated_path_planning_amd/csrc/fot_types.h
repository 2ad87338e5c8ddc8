// fot_types.h -- plain-old-data shared by the host code and the gfx950 kernels.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include "../../include/fot.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define FOT_HD __host__ __device__ __forceinline__
#else
#define FOT_HD inline
#endif

namespace fot {

constexpr int WAVE = 64;                 // gfx950 wavefront
constexpr int WAVES_PER_GROUP = 4;       // waves of one k_evaluate workgroup
// k_evaluate works on TILES, one per wave: up to 64 consecutive candidates of one instance whose longitudinal
// profiles fit one wave's share of LDS (tile_extent, fot_math.hpp).
constexpr int TILE_MAX_PROFILES = 8;     // profiles a tile may span (more brake-ladder entries: next tile)
constexpr int N_XCD = 8;
constexpr int LON_FIELDS = 10;           // rows of a GlobalTab table: s, s_d, s_dd, rx, ry, cos_r, sin_r, kappa_r, dkappa_r, 1/s_d
constexpr int ST_PENDING = FOT_ST_OK;    // passed the kinematic checks, collision check outstanding

struct d2 { double x, y; };
struct f2 { float x, y; };
constexpr float FAR32 = 1.0e18f;         // padding obstacle of the float32 broad-phase rows

// one time horizon: quartic / quintic boundary-value inverses (frenet_planner.py:586-617)
struct TimeInfo {
    double T;
    double qa[4];                        // inverse of [[3T^2,4T^3],[6T,12T^2]], row-major
    double qi[9];                        // inverse of the 3x3 quintic matrix, row-major
    int32_t n_t;                         // round(T/dt)+1 samples
    int32_t _pad;
};

// per-handle constants, resident in HBM, read through scalar loads
struct DevParams {
    double max_speed, max_accel, max_curvature, max_lat_accel;
    double dt, d_road_w, max_road_width, min_t, d_t_s;
    double k_j, k_t, k_d, k_s_dot, k_lat, k_lon;
    double sq_r, sq_r_dyn;               // squared combined radii (frenet_planner.py:1172-1175)
    double chance_epsilon;
    double road_lim;                     // max_road_width + 1e-9 (frenet_planner.py:982)
    double circ_off[FOT_MAX_CIRCLES];
    int32_t n_ti, n_di, n_side, n_brake; // n_brake = valid ladder entries
    int32_t n_total;                     // round(max_t/dt)+1
    int32_t n_circ;                      // expanded points per sample (>= 1)
    int32_t has_footprint;
    int32_t _pad;
    TimeInfo ti[FOT_MAX_TI];
    TimeInfo brake[FOT_MAX_BRAKE];
};

// cubic spline in HBM: 9 arrays of n doubles (b, d padded to n)
struct SplineView {
    const double *s, *ax, *bx, *cx, *dx, *ay, *by, *cy, *dy;
    int32_t n;
    int32_t _pad;
};

// host-built description of one instance
struct InstDesc {
    fot_ego ego;
    double target_speed;
    double max_stop;                     // NaN = none
    double lim_speed, lim_accel, lim_curv, lim_lat;
    double step_limit;                   // max(c_max_speed, max_speed)*dt*3 (frenet_planner.py:955)
    int32_t n_tv;
    int32_t n_down;                      // tv[k] = target - k*d_t_s for k <= n_down, else 0.0
    int32_t n_grid;                      // n_ti*n_tv*n_di
    int32_t cand_off;                    // first candidate slot (multiple of 64)
    int32_t n_cand_max;                  // n_grid + n_brake
    int32_t lon_off;                     // first longitudinal-profile slot
    int32_t n_static;
    uint32_t p_magic;                    // div_magic(P) (fot_math.hpp): k_cull's sample index j / P without a division
                                         // (in what was alignment padding: no other member moves)
    int64_t static_off;                  // points into the caller's static_xy
    int32_t dyn_mode, S, P, T;
    int64_t dyn_off;                     // points into the caller's dyn_xy
    int64_t ent_off;                     // first broad-phase entry slot of this instance
    int32_t ent_cap;                     // entry slots per time step (multiple of 16): S*P + n_static rounded up
    int32_t tile0;                       // number of this instance's first tile in the batch (tile-range rows)
    int32_t n_tiles;                     // tiles of this instance
    int32_t shape_off;                   // its lattice shape's first entry in the handle's tile table
    int32_t dyn_tmajor;                  // 1: the dynamic tensor is [T][S][P][2] (FOT_DYN_LAYOUT_TSP), 0: [S][P][T][2]
    int32_t max_viol;                    // floor(eps*S)
    int32_t n_chained;                   // instances right behind this one that continue its nearest-point cache
    int32_t scen;                        // its scenario: DevParams element and SplineView table entry of the handle
    int64_t nan_off;                     // first of this instance's S * P track flags (fot_kernels.hip scan_nan_tracks)
};

// device-produced per-instance state
struct InstState {
    double frenet0[6];
    double ref0[6];
    double new_prev_s;
    int32_t c2f_ok;
    int32_t n_brake;                     // 0 when s_d <= BRAKE_MIN_SPEED
    int32_t n_cand;
    int32_t _pad;
};

// one longitudinal profile (Ti x tv grid entry or brake-ladder entry)
struct LonInfo {
    double a0, a1, a2, a3, a4;
    double Js;                           // sum s_ddd^2 over all samples
    double sd_last;                      // s_d at the last (untruncated) sample
    double T;
    int32_t n_t;                         // samples incl. brake padding
    int32_t n_eval;                      // samples on the polynomial (== n_t unless brake)
};

// What a workgroup of the grouped evaluation kernels needs before its first time step and that no lane of it decides:
// one record per (instance, position of the group in the evaluation's launch order), built by k_frenet_state once the
// instance's Frenet state is known (fot_math.hpp build_group_head), fetched by the workgroup with one coalesced load.
// Position `pos` holds the instance's group n_groups - 1 - pos (the last group is evaluated first).
constexpr int GROUP_HEAD_TILES = 4, GROUP_HEAD_PROFILES = 16;   // == GROUP_TILES, GROUP_MAX_PROFILES (fot_math.hpp)
enum : int32_t {
    GROUP_HEAD_ABSENT = 0,               // no such group in this instance's lattice: no workgroup's business
    GROUP_HEAD_EMPTY = 2,                // its tiles exist but hold nothing to evaluate (no Frenet state, or the group
                                         // lies past n_cand: the brake ladder of a standing ego): they only count as done
    GROUP_HEAD_FULL = 1
};
struct alignas(128) GroupHead {
    int32_t present;                     // GROUP_HEAD_ABSENT / _EMPTY / _FULL; ABSENT: the only word that is written
    int32_t grp_tile0;                   // first tile of the group, inside the instance; EMPTY: nothing else is written
    int32_t slot_lo, n_stage;            // staged profiles: slots [slot_lo, slot_lo + n_stage)
    int32_t total_rows;                  // rows of all staged profiles
    int32_t n_total, n_circ_fp;          // P.n_total, loop_const().n_circ_fp
    int32_t cand_off, tile0, ent_cap, max_viol;         // of the InstDesc
    int32_t n_grid, n_tv, n_di, n_side, n_ti;           // what decode_candidate reads
    int32_t row0[GROUP_HEAD_PROFILES + 1];              // first row of profile p; total_rows from n_stage on
    int32_t t_cand0[GROUP_HEAD_TILES], t_n[GROUP_HEAD_TILES];   // per tile: first candidate, candidates below n_cand
    int32_t t_n_loop[GROUP_HEAD_TILES];                 // time steps: the longest of the tile's own profiles
    int32_t t_own_lo[GROUP_HEAD_TILES], t_own_hi[GROUP_HEAD_TILES];   // own profiles, relative to slot_lo (t_n > 0)
    int64_t ent_off;
    double d_road_w, dt, road_lim;       // of the DevParams
    double lim_speed, lim_accel, lim_curv, lim_lat;     // of the InstDesc
    double ego_x, ego_y;
    double frenet0[6];
    LonInfo info[GROUP_HEAD_PROFILES];   // profile_info(.., slot_lo + p, true); zero from n_stage on
};
static_assert(sizeof(GroupHead) % 128 == 0 && sizeof(GroupHead) == 1536, "whole 128-byte lines");

// What of a GroupHead the lattice alone decides -- the planner constants, the terminal-speed grid size, whether the brake
// ladder is there, the group position -- built once per handle on the host, next to the tile table and whenever that is
// rebuilt (fot_setup.hpp build_head_templates).  k_frenet_state copies it and fills in what the instance decides
// (fot_math.hpp group_head_compose).
// The handle's table: [variant][group of the tile table | one entry for the positions a shape does not have]
// (fot_math.hpp head_template_index).
constexpr int HEAD_COMMON_DWORDS = 344 / 4;                     // GroupHead in front of `info`, as 32-bit words
enum : int32_t { HEAD_VARIANT_GRID = 0, HEAD_VARIANT_BRAKE = 1, HEAD_VARIANTS = 2 };   // n_cand == n_grid / n_grid + n_brake
struct HeadProfile {                     // staged profile p of the group; n_t == 0 from n_stage on
    int32_t ti, itv;                     // horizon and terminal-speed index; itv < 0: entry ti of the brake ladder
    int32_t n_t, n_eval;                 // LonInfo's
    double T;
};
struct alignas(128) HeadTemplate {
    uint32_t common[HEAD_COMMON_DWORDS]; // the GroupHead's bytes in front of `info`; the instance's fields are zero
    uint32_t _pad[2];
    HeadProfile prof[GROUP_HEAD_PROFILES];
};
static_assert(sizeof(HeadTemplate) == 768, "whole 128-byte lines");
static_assert(offsetof(GroupHead, info) == 4 * HEAD_COMMON_DWORDS, "HeadTemplate::common is the GroupHead in front of info");

}  // namespace fot
