/*
 * fot.h -- C ABI of libfot.so, the MI355X (gfx950) Frenet optimal-trajectory planner.
 *
 * Drop-in boundary for ONE hot path of mnhrk15/integrated_path_planning:
 * FrenetPlanner.plan() (reference src/planning/frenet_planner.py:227-304) and
 * everything it calls.  The reference is pure Python and has no FFI of its own;
 * each entry point below names the reference interface it replaces, and
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no exceptions across the boundary; every call returns FOT_OK (0)
 *     or a negative FOT_ERR_*; fot_last_error(h) has the message.
 *   - "no feasible trajectory" is NOT an error: fot_result.status says so
 *     (the reference returns None, frenet_planner.py:294-304).
 *   - the caller owns every buffer it passes; the library neither keeps nor
 *     modifies inputs (reference: integrated_simulator.py:698 passes copies).
 *   - one handle = one GPU + one stream + its own workspace.  Handles share no
 *     state, so one handle per host thread / per rank is safe; a single handle
 *     is not thread-safe, and its calls execute in the order they were made even
 *     when they are enqueued on different caller streams: every enqueue first waits
 *     (on the device) for the handle's previous one, because they share the workspace
 *     and the scratch buffers.  To keep several batches in flight use one handle per
 *     batch in flight.  (The reference planner is not thread-safe either: it carries
 *     _last_kappa and converter._prev_s, frenet_planner.py:218, coordinate_converter.py:283;
 *     here that state is explicit in fot_ego / fot_result.)
 *   - all arithmetic that decides a candidate's status is float64, like the reference.
 */
#ifndef FOT_H
#define FOT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOT_MAX_NT 256       /* samples per candidate: round(max_t/dt)+1 must be <= 256 (dt = 0.02 s at max_t = 5 s: 251);
                                also the stride of the 15 path arrays of fot_result -- the library only ever touches the
                                first round(max_t/dt)+1 entries of each */
#define FOT_MAX_CIRCLES 8    /* ego footprint circles (footprint.py:26) */
#define FOT_MAX_TI 64        /* time horizons  int((max_t-min_t)/dt)+1  (min_t = 1 s at max_t = 5 s, dt = 0.1 s: 41) */
#define FOT_MAX_TV 32        /* terminal speeds per horizon */
#define FOT_MAX_BRAKE 32     /* brake-ladder entries 0.5 s, 1.0 s, ... < min_t (frenet_planner.py:475): min_t <= 16.4 s */
#define FOT_MAX_SAMPLES 64   /* prediction samples S of a distribution: a fresh handle's capacity (and fot_openloop_eval's,
                                whatever the handle's) */
#define FOT_MAX_PLAN_SAMPLES 254  /* ... what fot_set_sample_capacity can raise a handle to: sample ids travel as
                                uint8_t with 255 for a static obstacle, and 254 samples are four 64-bit mask words */

/* error codes */
#define FOT_OK 0
#define FOT_ERR_INVALID (-1)      /* bad argument */
#define FOT_ERR_UNSUPPORTED (-2)  /* configuration exceeds a FOT_MAX_* limit */
#define FOT_ERR_HIP (-3)          /* HIP runtime failure (no device, out of memory, ...) */
#define FOT_ERR_NO_PATH_SET (-4)  /* fot_set_path_* not called yet */

/* candidate status == index into fot_result.stats[]; order of the reference's
 * last_check_stats dict (frenet_planner.py:910-918, 324) */
enum {
    FOT_ST_SPEED = 0, FOT_ST_ACCEL = 1, FOT_ST_CURVATURE = 2, FOT_ST_LAT_ACCEL = 3,
    FOT_ST_ROAD = 4, FOT_ST_COLLISION = 5, FOT_ST_OK = 6, FOT_ST_STOP_DISTANCE = 7,
    FOT_ST_DROPPED = 8           /* silently dropped, not counted (frenet_planner.py:933-956) */
};

/* fot_result.status */
enum {
    FOT_PLAN_OK = 0,             /* a path was selected */
    FOT_PLAN_NO_PATH = 1,        /* plan() would return None after the checks: no 'ok' candidate with a cost below +inf */
    FOT_PLAN_C2F_FAILED = 2      /* plan() would return None at frenet_planner.py:266-268 */
};

/* obstacle element type */
enum { FOT_F32 = 0, FOT_F64 = 1 };
/* fot_batch.dyn_dims[i][0] */
enum { FOT_DYN_NONE = 0, FOT_DYN_SINGLE = 1, FOT_DYN_DISTRIBUTION = 2 };
/* OR-ed into dyn_dims[i][0]: instance i's tensor is laid out [T][S][P][2] (all pedestrians of one time row
 * contiguous: what the broad phase reads, fully coalesced) instead of the reference's [S][P][T][2].
 * fot_resample_predictions / fot_predict_cv write it when asked to (FOT_OUT_TMAJOR). */
#define FOT_DYN_LAYOUT_TSP 0x10

/* replaces the constructor arguments of FrenetPlanner (frenet_planner.py:149-210) */
typedef struct fot_params {
    double max_speed, max_accel, max_curvature, max_lat_accel;
    double dt, d_road_w, max_road_width;
    double robot_radius, obstacle_radius;
    double min_t, max_t, d_t_s;
    double k_j, k_t, k_d, k_s_dot, k_lat, k_lon;
    double chance_epsilon, collision_margin_inflation;
    int32_t n_circles;           /* 0: single circle of robot_radius; else EgoFootprint (footprint.py:14-45) */
    int32_t _pad;
    double footprint_radius;
    double footprint_offsets[FOT_MAX_CIRCLES];
} fot_params;

/* replaces EgoVehicleState (data_structures.py:32-51) + the planner's cross-call state */
typedef struct fot_ego {
    double x, y, yaw, v, a;
    double last_kappa;           /* FrenetPlanner._last_kappa */
    double prev_s;               /* CoordinateConverter._prev_s */
    int32_t has_prev_s;          /* 0: first call (global nearest-point search); 1: prev_s valid;
                                    2 (FOT_PREV_S_CHAINED): prev_s := new_prev_s of the PREVIOUS instance of the
                                    batch, i.e. this instance is the next plan() call on the same planner object
                                    (the escalation retries of integrated_simulator.py:602-644 in one launch);
                                    3 (FOT_EGO_IS_FRENET): the record IS a Frenet state -- x, y, yaw, v, a, last_kappa
                                    hold s, s_d, s_dd, d, d_d, d_dd -- and the lattice is generated from it as given
                                    (what the reference's tests do through _generate_frenet_paths(FrenetState, ...),
                                    frenet_planner.py:376); no nearest-point search, new_prev_s comes back NaN */
    int32_t _pad;
} fot_ego;
#define FOT_PREV_S_CHAINED 2
#define FOT_EGO_IS_FRENET 3

/* replaces constraint_overrides (frenet_planner.py:921-930); NaN = key absent */
typedef struct fot_overrides {
    double max_speed, max_accel, max_curvature, max_lat_accel;
} fot_overrides;

/* replaces the returned FrenetPath (data_structures.py:149-220) + last_check_stats + state updates */
typedef struct fot_result {
    int32_t status;              /* FOT_PLAN_* */
    int32_t best_index;          /* candidate index in generation order (Ti -> tv -> di, brake ladder last); -1 */
    int32_t n_cand;              /* candidates generated */
    int32_t n_keep;              /* samples in the path arrays below */
    double cost;
    int32_t stats[8];            /* last_check_stats, FOT_ST_* order */
    int32_t stats_valid;         /* 0 when the reference leaves last_check_stats = None */
    int32_t _pad;
    double new_last_kappa;       /* value of _last_kappa after the call */
    double new_prev_s;           /* value of converter._prev_s after the call */
    double frenet0[6];           /* s, s_d, s_dd, d, d_d, d_dd of the ego (frenet_planner.py:371) */
    double ref0[6];              /* rs, rx, ry, rtheta, rkappa, rdkappa (coordinate_converter.py:308) */
    /* path arrays: entries [0, n_keep) hold the path, [n_keep, n_total) are written as zero, entries from
     * n_total = round(max_t/dt)+1 on are NEVER touched, neither in a device-resident record nor in the caller's host
     * record (a caller who compares whole records zero-fills its buffer once) */
    double t[FOT_MAX_NT], s[FOT_MAX_NT], s_d[FOT_MAX_NT], s_dd[FOT_MAX_NT], s_ddd[FOT_MAX_NT];
    double d[FOT_MAX_NT], d_d[FOT_MAX_NT], d_dd[FOT_MAX_NT], d_ddd[FOT_MAX_NT];
    double x[FOT_MAX_NT], y[FOT_MAX_NT], yaw[FOT_MAX_NT], v[FOT_MAX_NT], a[FOT_MAX_NT], c[FOT_MAX_NT];
} fot_result;

/* One batch of independent ego/scenario instances = the arguments of n_inst
 * plan() calls (frenet_planner.py:227-236).  The small per-instance arrays and
 * the shape metadata are ALWAYS host memory; the obstacle coordinates (and the
 * results) are host memory for fot_plan_batch and device memory for
 * fot_plan_batch_device. */
typedef struct fot_batch {
    int32_t n_inst;
    int32_t obstacle_dtype;              /* FOT_F32 | FOT_F64 */
    const fot_ego *ego;                  /* [n_inst] host */
    const double *target_speed;          /* [n_inst] host */
    const fot_overrides *overrides;      /* [n_inst] host, or NULL */
    const double *max_stop_distance;     /* [n_inst] host, NaN = None; or NULL */
    /* static_obstacles [Ns,2] per instance, concatenated; instance i owns points [static_off[i], static_off[i+1]) */
    const void *static_xy;               /* host | device */
    const int32_t *static_off;           /* [n_inst+1] host, or NULL (no static obstacles) */
    /* dynamic_obstacles [P,T,2] / dynamic_obstacles_distribution [S,P,T,2] per instance, concatenated;
     * instance i starts at point dyn_off[i]; dyn_dims[i] = {mode, S, P, T} (S = 1 for FOT_DYN_SINGLE).
     * Non-finite coordinates never hit, and a pedestrian whose track holds a NaN anywhere is no obstacle at ANY
     * time step, as in the reference (np.min / np.max in its box pre-filter, frenet_planner.py:1211-1219): the
     * library finds such tracks itself, whoever produced the tensor. */
    const void *dyn_xy;                  /* host | device */
    const int64_t *dyn_off;              /* [n_inst] host, or NULL (no dynamic obstacles) */
    const int32_t *dyn_dims;             /* [n_inst][4] host */
} fot_batch;

typedef struct fot_handle fot_handle;

const char *fot_version(void);

/* What the library was BUILT with, for a binding to check before its first real call: a binding whose structure layouts
 * or array capacities differ from the library's corrupts memory instead of failing (round 3: an older libfot.so with
 * four profile slots under a binding that allocated three aborted the process at exit with "double free or
 * corruption").  out[i], i < cap: FOT_ABI_VERSION, sizeof of fot_params, fot_ego, fot_overrides, fot_result, fot_batch,
 * fot_resample_params, fot_safety, fot_loop_frame, fot_loop_request, fot_wire_header, then FOT_MAX_NT, FOT_MAX_CIRCLES,
 * FOT_MAX_TI, FOT_MAX_TV, FOT_MAX_BRAKE, FOT_MAX_SAMPLES, FOT_MAX_PRED_LEN, FOT_PROFILE_KERNELS, FOT_MARGIN_GROUPS,
 * sizeof of fot_loop_config, fot_loop_step_out, fot_loop_replay, fot_loop_run_out, fot_loop_summary, fot_pred_origin,
 * fot_pred_score, fot_sgan_desc, then FOT_SGAN_MAX_EMBEDDING, FOT_SGAN_MAX_HIDDEN, FOT_SGAN_MAX_MLP,
 * FOT_SGAN_MAX_BOTTLENECK, FOT_SGAN_MAX_OBS_LEN, FOT_SGAN_MAX_PEDS, FOT_SGAN_POOL_HIDDEN.
 * Returns the number of words the library knows (FOT_ABI_INFO_WORDS of ITS header). */
#define FOT_ABI_VERSION 8
#define FOT_ABI_INFO_WORDS 35
int32_t fot_abi_info(int32_t cap, int32_t *out);

/* FrenetPlanner.__init__ (frenet_planner.py:149-225).  device < 0: current device. */
int fot_create(const fot_params *params, int device, fot_handle **out);
/* Frees the handle.  Idempotent (a pointer fot_create did not return, or one already destroyed, is ignored) and
 * bounded: the handle's streams and the event behind its last enqueue are polled for at most FOT_DESTROY_TIMEOUT_MS
 * (default 5000); if they do not drain, or the HIP runtime is already shutting down, device and pinned memory are left
 * to the process teardown instead of being freed under running work.  Never blocks on a caller's stream. */
void fot_destroy(fot_handle *h);
/* handles created and not yet destroyed in this process (what a binding's exit hook still has to close) */
int32_t fot_live_handles(void);
const char *fot_last_error(const fot_handle *h);   /* h may be NULL: error of the last failed fot_create */

/* reference_path: CubicSpline2D(waypoints) (cubic_spline.py:190-213) built natively ... */
int fot_set_path_waypoints(fot_handle *h, int32_t n, const double *wx, const double *wy);
/* ... or adopted verbatim from an existing CubicSpline2D object: knots s[n] and the
 * CubicSpline1D coefficient arrays a[n], b[n-1], c[n], d[n-1] of sx and sy (cubic_spline.py:30-45) */
int fot_set_path_coeffs(fot_handle *h, int32_t n, const double *s,
                        const double *ax, const double *bx, const double *cx, const double *dx,
                        const double *ay, const double *by, const double *cy, const double *dy);
/* read the spline back (same array sizes); n_out receives the knot count; arrays may be NULL */
int fot_get_path_coeffs(const fot_handle *h, int32_t *n_out, double *s,
                        double *ax, double *bx, double *cx, double *dx,
                        double *ay, double *by, double *cy, double *dy);
/* CubicSpline2D.calc_position/calc_yaw/calc_curvature/calc_curvature_rate (cubic_spline.py:215-288)
 * evaluated on the device; NaN outside the domain.  Host arrays of n doubles. */
int fot_spline_eval(fot_handle *h, int32_t n, const double *s, double *x, double *y,
                    double *yaw, double *kappa, double *dkappa);

/* n_inst x FrenetPlanner.plan() with host-resident obstacles and results; synchronous */
int fot_plan_batch(fot_handle *h, const fot_batch *batch, fot_result *out);
/* same with device-resident obstacle coordinates and a device-resident fot_result[n_inst];
 * enqueued on `stream` (a hipStream_t; NULL = the handle's own stream) and NOT synchronised */
int fot_plan_batch_device(fot_handle *h, const fot_batch *batch, fot_result *out_dev, void *stream);
/* block until everything the handle enqueued on its own stream has finished */
int fot_synchronize(fot_handle *h);

/* ---- scenarios: several planner configurations and reference paths in one handle --------------------------------
 * A scenario is what one reference FrenetPlanner object is (integrated_simulator.py:289, 342-366): one fot_params and
 * one reference path.  Scenario 0 is the handle's own (fot_create's params, fot_set_path_*); fot_add_scenario adds
 * scenarios 1, 2, ... up to FOT_MAX_SCENARIOS in all, and fot_plan_batch_scenarios[_device] plans every instance i of a
 * batch on scenario scenario[i] (a host array of n_inst ids; NULL = scenario 0 for all) in ONE launch sequence.
 * fot_plan_batch / fot_plan_batch_device are these calls with scenario = NULL.
 *   - every scenario of a handle has the handle's dt and max_t (one time grid: n_total, the records, the wire form);
 *     params with another dt or max_t are FOT_ERR_INVALID, any other limit fails as fot_create would fail
 *   - a 65th scenario is FOT_ERR_UNSUPPORTED, an unknown id FOT_ERR_INVALID, an instance whose scenario has no path
 *     FOT_ERR_NO_PATH_SET, a FOT_PREV_S_CHAINED instance on another scenario than its predecessor FOT_ERR_INVALID
 *     (a chain is one planner object); a refused call changes nothing
 *   - fot_debug_candidates / fot_debug_candidate_path / fot_debug_margins answer for instance i on its own scenario
 *   - a closed loop begun with fot_loop_begin_scenarios runs every episode slot on a scenario of its own (below); a loop
 *     begun with fot_loop_begin, and the two-call form fot_loop_plan / fot_loop_observe*, work on scenario 0
 *   - every other entry point works on scenario 0: fot_check_paths, fot_check_collision_paths,
 *     fot_spline_eval, fot_get_path_coeffs (fot_get_scenario_path_coeffs reads any), fot_frenet_state_batch, fot_safety_metrics_batch, fot_debug_time_info */
#define FOT_MAX_SCENARIOS 64
int fot_add_scenario(fot_handle *h, const fot_params *params, int32_t *id_out);
int fot_set_scenario_path_waypoints(fot_handle *h, int32_t id, int32_t n, const double *wx, const double *wy);
int fot_set_scenario_path_coeffs(fot_handle *h, int32_t id, int32_t n, const double *s,
                                 const double *ax, const double *bx, const double *cx, const double *dx,
                                 const double *ay, const double *by, const double *cy, const double *dy);
/* fot_get_path_coeffs for scenario id (0: the same call) */
int fot_get_scenario_path_coeffs(const fot_handle *h, int32_t id, int32_t *n_out, double *s,
                                 double *ax, double *bx, double *cx, double *dx,
                                 double *ay, double *by, double *cy, double *dy);
int fot_plan_batch_scenarios(fot_handle *h, const fot_batch *batch, const int32_t *scenario, fot_result *out);
int fot_plan_batch_scenarios_device(fot_handle *h, const fot_batch *batch, const int32_t *scenario,
                                    fot_result *out_dev, void *stream);

/* FrenetPlanner._cartesian_to_frenet_state (frenet_planner.py:334-374) for n egos.
 * frenet[n][6], ref[n][6], new_prev_s[n], ok[n] (1 = converted) -- host arrays */
int fot_frenet_state_batch(fot_handle *h, int32_t n, const fot_ego *ego,
                           double *frenet, double *ref, double *new_prev_s, int32_t *ok);

/* Per-candidate table of instance `inst` of the most recent plan call on this handle
 * (what _check_paths put in each list, frenet_planner.py:932-991).  Arrays of `cap`
 * entries, any may be NULL; returns the number of candidates or a negative error. */
int fot_debug_candidates(fot_handle *h, int32_t inst, int32_t cap, double *cost,
                         int32_t *status, int32_t *keep, int32_t *n_t);

/* All 15 FrenetPath arrays of candidate `index` of instance `inst` of the most recent plan call, BEFORE
 * truncation (what _generate_frenet_paths + _calc_global_paths produce, frenet_planner.py:376-503, 736-889):
 * arrays[15][FOT_MAX_NT] in fot_result field order, *n_t = generated samples. */
int fot_debug_candidate_path(fot_handle *h, int32_t inst, int32_t index, double *arrays, int32_t *n_t);

/* Epsilon-band report for instance `inst` of the most recent plan call: per candidate and per group of decisions the
 * smallest relative distance |value - threshold| / |threshold| of every comparison made on it (speed :964, accel :966,
 * curvature incl. the 0.5 m/s gate and the low-speed rules :968/:995-1033, lateral acceleration :975, road :982,
 * collision radius :1198/:1233 against the obstacles the broad phase kept, stop filter :307-324, structural:
 * singularity :826, EPS_S_DOT :792, step length :955).  margins[cap][FOT_MARGIN_GROUPS]; +inf = no such decision.
 * A status that differs from the reference's with all margins far above float64 rounding is a logic error; a margin
 * at rounding level marks a decision that a re-association may flip.  Returns the number of candidates. */
#define FOT_MARGIN_GROUPS 8
int fot_debug_margins(fot_handle *h, int32_t inst, int32_t cap, double *margins);

/* Test hook.  A plan call of a few egos cuts every candidate's time range into up to 4 segments evaluated by
 * different waves and merged (the decisions are the same: every per-candidate accumulator of _check_paths /
 * _path_is_collision_free merges associatively); large batches walk it in one piece.  n_seg = 1..4 forces the number
 * of segments for the handle's later plan calls, 0 restores the choice by batch size. */
int fot_debug_set_eval_segments(fot_handle *h, int32_t n_seg);

/* Test hook.  How the handle cuts a lattice into tiles (the unit of work of the evaluation kernel): 0 = chosen by
 * the lattice (default), 1 = per-wave rows (k_evaluate: every wave stages the rows of its own tile), 2 = groups
 * (k_evaluate_group: four tiles share one row table).  Same decisions, byte-identical records either way; the GPU
 * tests run every reference case under both cuts and under 1..4 time segments.  Rebuilds the handle's tile table
 * (synchronises the device); applies to the handle's later plan calls. */
int fot_debug_set_tile_cut(fot_handle *h, int32_t cut);

/* Test hook.  The evaluation kernels have a lean form for launches that cannot use the chance budget or a second block
 * of time steps: every scenario of the handle has at most 64 samples per candidate and the single centre circle (no
 * footprint circles), and every instance of the launch has max_viol == 0 (epsilon = 0).  The library picks it per launch;
 * same decisions, byte-identical records.  form = 1 makes the handle's later plan calls run the general form whatever
 * they are eligible for, 0 restores the choice by eligibility, -1 changes nothing.  Returns (>= 0) the forms the launches
 * of the handle's most recent plan call took -- 0: none yet, 1: general, 2: lean, 3: both (a batch split into lanes) --
 * or a negative FOT_ERR_*.  A wide launch (fot_set_sample_capacity: an instance of more than FOT_MAX_SAMPLES samples)
 * adds 4 (the general form with a four-word sample mask) or 8 (the lean form) instead of 1 or 2. */
int fot_debug_set_eval_form(fot_handle *h, int32_t form);

/* The sample capacity of the handle: the largest S of a prediction distribution that EVERY entry taking one accepts --
 * fot_plan_batch, fot_plan_batch_device, their _scenarios forms, fot_check_collision_paths and fot_check_paths; the
 * frames of fot_loop_plan / fot_loop_step (dist_S); fot_loop_set_samples(_shared); fot_loop_set_sampler(_shared,
 * _models); fot_sgan_sample(_model) and fot_sgan_noise; fot_prediction_scores and fot_loop_prediction_scores; and with
 * them fot_loop_scores_enable, fot_loop_plan_sample and the sweep loops, which take the S of the loop's predictor.
 * Beyond it they return FOT_ERR_UNSUPPORTED with a message that names S and the capacity, and change nothing.  A fresh
 * handle has FOT_MAX_SAMPLES.  fot_set_sample_capacity accepts FOT_MAX_SAMPLES <=
 * n_samples <= FOT_MAX_PLAN_SAMPLES; anything else is FOT_ERR_INVALID and leaves the handle as it was.  The capacity is
 * the handle's, for all its scenarios.  A launch with an instance of more than FOT_MAX_SAMPLES samples is WIDE: it runs
 * evaluation kernels of its own that count distinct samples in four mask words (lean-eligible launches: kernels that
 * need no sample ids) and has no flat form.  Every other launch runs the kernels it ran before, raised capacity or not.
 * The fot_debug_* entries work after a wide launch.  The prediction scores and the representative-sample selection of a
 * distribution of more than FOT_MAX_SAMPLES samples run wide forms of their kernels too (per-sample tables of
 * FOT_MAX_PLAN_SAMPLES rows); with at most FOT_MAX_SAMPLES samples every entry runs the kernels of a fresh handle and
 * returns its bytes, raised capacity or not.
 * A loop that is set up: RAISING the capacity is always accepted (a loop's buffers are sized by its own S, not by the
 * capacity, so nothing of a begun loop moves).  LOWERING it below the samples of the handle's loop -- the S of a resident
 * loop's sampler or recording (from the set call until the next fot_loop_begin* / fot_loop_set_replay), or the dist_S of
 * a stepwise loop's current frame -- is FOT_ERR_INVALID and leaves the capacity as it was.
 * Out of scope: fot_openloop_eval keeps FOT_MAX_SAMPLES whatever the handle's capacity; summaries together with a sampler
 * or a recording stay refused.  (The slots of one sweep may keep sample counts of their own: fot_loop_set_slot_samples.)
 * fot_max_plan_samples: the FOT_MAX_PLAN_SAMPLES the library was built with, for a binding to compare with its own.
 * Additions: no structure, capacity word of fot_abi_info or FOT_ABI_VERSION changes; a binding looks the symbols up. */
int fot_set_sample_capacity(fot_handle *h, int32_t n_samples);
int fot_get_sample_capacity(const fot_handle *h, int32_t *out);
int32_t fot_max_plan_samples(void);

/* Test hook.  The lean evaluation kernels have a flat form for reference paths that are exactly straight: one coordinate
 * of the path's spline has all first-, second- and third-derivative coefficients exactly zero and the other is finite
 * and strictly monotonic.  Every row of such a path has curvature and curvature rate +-0, and the flat form leaves out
 * the arithmetic that exists for them; same decisions, byte-identical records.  The library decides per path where the
 * path is set, and a lean-eligible launch takes the flat form when every path its instances use is flat.  on = 0 keeps
 * the handle's later plan calls on the other kernels, 1 restores the choice by eligibility (the default), -1 changes
 * nothing.  Returns 1 when a launch of the handle's most recent plan call took a flat kernel, 0 when none did, or a
 * negative FOT_ERR_*.  fot_debug_set_eval_form reports a flat launch as lean. */
int fot_debug_set_flat(fot_handle *h, int32_t on);

/* FrenetPlanner._build_time_cache (frenet_planner.py:586-617) as the library holds it for a horizon of `time`
 * seconds: the sample count n_t = round(time / dt) + 1 and the closed-form inverses of the quartic / quintic
 * boundary-value matrices (row-major 2x2 and 3x3) that every lattice polynomial is solved with.  Host only. */
int fot_debug_time_info(const fot_handle *h, double time, int32_t *n_t, double *quartic_inv4, double *quintic_inv9);

/* FrenetPlanner._path_is_collision_free (frenet_planner.py:1035-1233) for n_paths externally
 * supplied paths against ONE obstacle set.  x, y, yaw, t: [n_paths][FOT_MAX_NT] host, len[n_paths];
 * static_xy [n_static][2] double host; dyn [S][P][T][2] double host with mode as in dyn_dims.
 * free_out[n_paths]: 1 = collision free. */
int fot_check_collision_paths(fot_handle *h, int32_t n_paths, const int32_t *len,
                              const double *x, const double *y, const double *yaw, const double *t,
                              int32_t n_static, const double *static_xy,
                              int32_t mode, int32_t S, int32_t P, int32_t T, const double *dyn,
                              int32_t *free_out);

/* FrenetPlanner._check_paths (frenet_planner.py:891-993) followed by _apply_stop_distance_filter (:307-324)
 * for n_paths externally supplied paths: arrays [n_paths][FOT_MAX_NT] host (yaw, d, s may be NULL = zeros),
 * len[n_paths] = samples of x, y and t (0: the path is skipped, as the reference skips an empty path and one whose x
 * and t differ in length).  The reference applies every rule over the arrays that rule reads, which an externally
 * constructed path may hold in different lengths; rule_len[n_paths][FOT_CHECK_RULE_LENS] carries them, each
 * 0..FOT_MAX_NT and possibly larger than len[i]:
 *   [0] n_geo = min(len x, y, yaw, s, d): the low-speed curvature rules apply while k < n_geo (:1017-1022)
 *   [1] len d: the road-corridor test runs over all of d (:982)
 *   [2] [3] [4] len v, a, c: finiteness (:944) and the limits (:964, :966) run over all of each; the curvature rules
 *       (:1013) and the lateral acceleration (:975) over min(len v, len c)
 *   [5] len s: the stop filter reads s[len s - 1] - s[0] and v[len v - 1] (:317-318; no v: never at rest, no s: no travel)
 * NULL = every array holds len[i] samples.  Nothing beyond an array's own length is read into a decision.  yaw is read
 * up to len[i] by the collision test with a footprint (a shorter yaw is held by the caller, :1158-1161).
 * overrides may be NULL, max_stop_distance NaN = None, obstacle set as in fot_check_collision_paths.
 * status_out[n_paths]: FOT_ST_* (FOT_ST_OK = 'ok', FOT_ST_DROPPED = silently skipped). */
#define FOT_CHECK_RULE_LENS 6
int fot_check_paths(fot_handle *h, int32_t n_paths, const int32_t *len, const int32_t *rule_len,
                    const double *x, const double *y, const double *yaw, const double *v, const double *a,
                    const double *c, const double *d, const double *s, const double *t,
                    const fot_overrides *overrides, double max_stop_distance,
                    int32_t n_static, const double *static_xy,
                    int32_t mode, int32_t S, int32_t P, int32_t T, const double *dyn, int32_t *status_out);

/* ---- the obstacle-tensor producer in front of the planner ------------------------------
 * TrajectoryPredictor.process_prediction (trajectory_predictor.py:233-313) for S prediction samples, fused
 * with the current-position prepend of IntegratedSimulator._update_prediction (integrated_simulator.py:503-525):
 * raw Social-GAN predictions (0.4 s grid, anchored at the last observation) -> the planner's [S][P][T][2]
 * obstacle tensor on the dt grid, written where fot_plan_batch_device reads it (no host round trip).
 *   pred    [S][pred_len][P][2] (pred_dtype), host or device memory according to on_device
 *   anchor  [P][2] host, or NULL (no anchor point);  current [P][2] host, or NULL (no prepend)
 *   out     [S][P][T][2] (out_dtype), same memory space as pred; *T_out = n_dense (+1 with current)
 *   sample_dist [S] host or NULL: sum over (p, k) of |sample - sample mean|, whose first minimum is
 *               predict_single_best's representative sample (:346-351); requesting it synchronises
 * pred_len <= FOT_MAX_PRED_LEN, T <= FOT_MAX_NT.  stream: NULL = the handle's stream. */
#define FOT_MAX_PRED_LEN 32
typedef struct fot_resample_params {
    double sgan_dt, sim_dt, plan_horizon;
} fot_resample_params;
/* bits of the `on_device` argument below */
#define FOT_OUT_DEVICE 1     /* pred / out are device memory (else host memory) */
#define FOT_OUT_TMAJOR 2     /* out is written [T][S][P][2] (FOT_DYN_LAYOUT_TSP) instead of [S][P][T][2] */
int fot_resample_n_dense(const fot_resample_params *rp, int32_t pred_len);
int fot_resample_predictions(fot_handle *h, const fot_resample_params *rp, int32_t S, int32_t pred_len, int32_t P,
                             const void *pred, int32_t pred_dtype, const double *anchor, const double *current,
                             double staleness, void *out, int32_t out_dtype, int32_t on_device, int32_t *T_out,
                             double *sample_dist, void *stream);
/* TrajectoryPredictor.predict_cv (:188-231): obs_last / obs_prev [P][2] host (obs_prev NULL = zero velocity)
 * -> out [P][T][2] with the same prepend / memory-space conventions.  obs_dtype FOT_F32: the observations are float32
 * (what PedestrianObserver.get_observation hands over, observer.py:134) and the velocity is formed in float32 as NumPy
 * does for float32 arrays; FOT_F64: float64 observations, float64 velocity. */
int fot_predict_cv(fot_handle *h, const fot_resample_params *rp, int32_t pred_len, int32_t P,
                   const void *obs_last, const void *obs_prev, int32_t obs_dtype, const double *current,
                   double staleness, void *out, int32_t out_dtype, int32_t on_device, int32_t *T_out, void *stream);

/* ---- compute_safety_metrics_static (data_structures.py:301-388) for n egos in one launch ----
 * ego [n][4] = x, y, yaw, v; pedestrians of ego i: ped_pos / ped_vel [ped_off[i] .. ped_off[i+1])[2]  (host arrays).
 * use_footprint != 0: the handle's multi-circle footprint (footprint= argument of the reference); otherwise, or when the
 * handle has none, the single centre circle of ego_radius. */
typedef struct fot_safety {
    double min_distance, ttc, clearance, clearance_ahead;
    int32_t collision;
    int32_t _pad;
} fot_safety;
int fot_safety_metrics_batch(fot_handle *h, int32_t n, const double *ego, const int32_t *ped_off,
                             const double *ped_pos, const double *ped_vel, double ego_radius, double ped_radius,
                             int32_t use_footprint, fot_safety *out);

/* ---- the device work of one closed-loop step (IntegratedSimulator.step, integrated_simulator.py:678-747)
 * of n episodes in two calls with ONE synchronisation each; the prediction tensor never leaves HBM.
 *
 * fot_loop_plan, with a frame: _update_prediction's constant-velocity branch (:424-527 -> trajectory_predictor.py
 * :188-231) for the pedestrians of all episodes, written into the handle's own tensor -- per episode a [P_e][T_e][2]
 * float64 block, T_e = n_dense + prepend[e] -- and compute_safety_metrics_static on the current ego states (:529-560);
 * then n_req plan() calls (:562-600), request j against the block of episode req[j].episode.  Without a frame
 * (NULL) the requests run against the tensor of the previous call: the escalation retries of one step (:602-644).
 * *records points at n_req records in pinned host memory owned by the handle, valid until the next fot_loop_plan.
 *
 * fot_loop_observe: the metrics of the new ego states against the same frame's pedestrians (:864-870) and the arc
 * length of the nearest point of the reference path (the goal test's converter, :873-883), ego i = episode i:
 * ego5 [n][5] = x, y, yaw, v, a; prev_s [n], NaN = no cached arc length.  _begin enqueues the two launches and returns,
 * _end waits and hands the results over (any may be NULL); no other call on the handle in between.
 *
 * fot_loop_set_static: the static obstacle points every request of the loop sees (kept in HBM, one copy per request);
 * it is fot_loop_set_scenario_static for scenario 0.  These two calls and fot_loop_observe* are the two-call form: they
 * work on scenario 0 whatever loop the handle has begun. */
typedef struct fot_loop_frame {
    int32_t n_episodes;
    int32_t pred_len;               /* of the predictor (trajectory_predictor.py:188) */
    int32_t use_footprint;          /* as fot_safety_metrics_batch */
    int32_t _pad;
    const int32_t *ped_off;         /* [n_episodes + 1]: pedestrians of episode e = rows [ped_off[e], ped_off[e+1]) */
    const double *ped_pos, *ped_vel;    /* [sum P][2] current positions / velocities */
    const float *obs_last, *obs_prev;   /* [sum P][2] the observer's last two samples; obs_last NULL: the predictor is
                                           not ready and the tensor is the current positions alone (T = 1, :495-498) */
    const uint8_t *prepend;         /* [n_episodes] 1: the current positions lead the episode's tracks (:503-511) */
    const double *ego;              /* [n_episodes][4] x, y, yaw, v for the metrics; NULL = no metrics */
    double staleness;               /* time since the observer's last sample (:463-470) */
    double ego_radius, ped_radius;
    fot_resample_params rp;
    /* Distribution-aware planning (integrated_simulator.py:459-460, 514-525, 622-630) without a host round trip: the raw
     * samples of a multi-sample predictor for ALL the frame's pedestrians, [dist_S][pred_len][sum P][2] in DEVICE memory
     * (what dist_S Social-GAN forward passes on PyTorch-ROCm leave), anchored at obs_last.  They are resampled on the
     * device (process_prediction, trajectory_predictor.py:233-313) straight into the handle's tensor, per episode a
     * [dist_S][P_e][n_dense + 1][2] block led by the current positions in EVERY sample, and every request of the step
     * plans against its episode's whole distribution under the handle's chance constraint.  NULL: the constant-velocity
     * predictor above.  dist_dtype FOT_F32 | FOT_F64; dist_S <= the handle's sample capacity
     * (fot_set_sample_capacity; FOT_ERR_UNSUPPORTED beyond it). */
    const void *dist_raw;
    int32_t dist_S, dist_dtype;
} fot_loop_frame;
typedef struct fot_loop_request {
    fot_ego ego;
    fot_overrides overrides;
    double target_speed;
    double max_stop_distance;       /* NaN = None */
    int32_t episode;                /* whose pedestrians */
    int32_t _pad;
} fot_loop_request;
int fot_loop_set_static(fot_handle *h, int32_t n_points, const double *xy);
int fot_loop_plan(fot_handle *h, const fot_loop_frame *frame, int32_t n_req, const fot_loop_request *req,
                  fot_safety *safety_out, const fot_result **records);
int fot_loop_observe(fot_handle *h, int32_t n, const double *ego5, const double *prev_s,
                     fot_safety *safety_out, double *new_prev_s);
int fot_loop_observe_begin(fot_handle *h, int32_t n, const double *ego5, const double *prev_s);
int fot_loop_observe_end(fot_handle *h, fot_safety *safety_out, double *new_prev_s);
/* The WHOLE lock step behind one call: the episodes' state lives in the handle (ego, the planner's nearest-point cache and
 * last curvature, the fail-safe state machine), a step is
 *   prediction + current metrics + the level-0 plan() of every running episode (fot_loop_plan with the frame)
 *   -> every further escalation level of the episodes whose first attempt failed, in one more launch
 *   -> the reference's retry loop replayed on the records (integrated_simulator.py:576-653, state_machine.py:116-247)
 *   -> ego update from the selected path's sample 1, or the emergency stop (:655-676, :749-802)
 *   -> metrics of the new states + the goal test's nearest point (fot_loop_observe).
 * fot_loop_config: IntegratedSimulator's and FailSafeStateMachine's constants as the reference resolves them from its
 * configuration (state_machine.py:32-98); emergency_decel NaN = 2 x max_accel.
 * fot_loop_begin: n_episodes slots, ego5 [n][5] = x, y, yaw, v, a; every machine NORMAL, no caches.
 * fot_loop_step: frame as for fot_loop_plan (its `ego` is ignored: the handle knows the egos), episode[i] = the slot
 * of the frame's episode i (distinct); out arrays of frame->n_episodes entries, any may be NULL.  out->records: the
 * step's records in pinned memory owned by the handle (level 0 of episode i = record i, escalation levels behind),
 * valid until the next loop call; out->record[i]: the record whose path episode i follows (-1: emergency stop). */
typedef struct fot_loop_config {
    double dt, target_speed, max_accel, emergency_decel;
    double clearance_caution, clearance_emergency;               /* recovery thresholds (combined radii subtracted) */
    double trigger_clearance_caution, trigger_time_headway;      /* preventive escalation */
    double envelope_decel, envelope_standoff;                    /* speed envelope on the clearance ahead */
    double caution_accel, caution_speed, caution_speed_mult;     /* CAUTION: overrides, target speed factor */
    double emergency_accel, emergency_lat_accel;                 /* EMERGENCY: overrides */
    int32_t max_replan;                                          /* integrated_simulator.py:383 */
    int32_t _pad;
} fot_loop_config;
typedef struct fot_loop_step_out {
    double *ego;                /* [n][5] the new ego states */
    double *jerk;               /* [n] */
    int32_t *state;             /* [n] 0 / 1 / 2 = NORMAL / CAUTION / EMERGENCY after the step */
    int32_t *stats;             /* [n][8] last_check_stats of the last plan() of the step; a row of -1: None */
    int32_t *record;            /* [n] */
    int32_t *keep;              /* [n] samples of the followed path (0: none) */
    double *cost;               /* [n] */
    fot_safety *before, *after; /* [n] metrics of the current / of the new ego states */
    double *s_now;              /* [n] arc length of the new state's nearest path point */
    const fot_result *records;  /* out */
    int32_t n_records;          /* out */
    int32_t _pad;
} fot_loop_step_out;
int fot_loop_begin(fot_handle *h, int32_t n_episodes, const fot_loop_config *cfg, const double *ego5);
/* ---- episodes of different scenarios in one lock step ---------------------------------------------------------------
 * fot_loop_begin_scenarios is fot_loop_begin with a scenario per episode slot: slot e runs on scenario slot_scenario[e]
 * (fot_add_scenario; 0 = the handle's own), with the fail-safe and simulator constants cfg[slot_scenario[e]] and, when
 * use_footprint[slot_scenario[e]] != 0 (use_footprint NULL = all 0), the scenario's multi-circle footprint in the safety
 * metrics.  cfg / use_footprint: n_cfg entries indexed by scenario id; entries of scenarios no slot names are not read.
 * fot_loop_begin is this call with every slot on scenario 0.  Per slot from then on: the reference path and planner
 * constants of its plan() calls (escalation retries included), the path of the goal test's nearest point, the metrics'
 * footprint, the state machine's and the emergency stop's constants, the static obstacle points
 * (fot_loop_set_scenario_static: scenario id's point set, kept once in HBM; a step's per-request blocks are gathered from
 * the sets on the device) and, in fot_loop_run, the goal: s_end is the last knot of the slot's own path, and
 * fot_loop_replay.s_end is ignored.  fot_loop_frame.use_footprint / fot_loop_replay.use_footprint are ignored too.
 * fot_loop_step and fot_loop_run take no new argument: the slot knows its scenario.
 * Common to the scenarios of a loop: dt (and max_t: fot_add_scenario), and what the frame / the replay carries once:
 * ego_radius, ped_radius, pred_len, obs_len, sgan_dt, goal_distance.
 * Refusals; a refused call changes nothing, a run in progress goes on: slot_scenario[e] not a scenario of the handle, or
 * n_cfg <= slot_scenario[e], or configurations in use with different dt (FOT_ERR_INVALID); a slot's scenario without a
 * path (FOT_ERR_NO_PATH_SET); fot_loop_set_scenario_static with an unknown id (FOT_ERR_INVALID); fot_loop_step of a
 * scenario loop with dist_raw samples (FOT_ERR_UNSUPPORTED: constant-velocity predictor only). */
int fot_loop_begin_scenarios(fot_handle *h, int32_t n_episodes, int32_t n_cfg, const fot_loop_config *cfg,
                             const int32_t *use_footprint, const int32_t *slot_scenario, const double *ego5);
int fot_loop_set_scenario_static(fot_handle *h, int32_t id, int32_t n_points, const double *xy);
int fot_loop_step(fot_handle *h, const fot_loop_frame *frame, const int32_t *episode, fot_loop_step_out *out);

/* ---- whole replayed episodes behind one call ------------------------------------------------------------------------
 * With replayed pedestrians nothing in an episode depends on the caller between two lock steps, so the caller hands the
 * recording over once and the library runs the steps itself: a C caller's episode is three calls,
 *   fot_loop_begin (slots, fail-safe constants, initial egos) -> fot_loop_set_replay (recording, observer and predictor
 *   constants, goal) -> fot_loop_run (up to max_steps lock steps; again until it returns 0).
 * fot_loop_set_replay copies the recording of every episode slot into HBM, where it stays, and runs the warm-up
 * (warmup_frames frames that only fill the observer, integrated_simulator.py:406-422; int(obs_len * sgan_dt / dt) in the
 * reference).  It needs a fot_loop_begin with the same number of slots before it.  Refusals -- the codes fot_loop_plan has
 * for the same faults; a refused call changes nothing: no fot_loop_begin / n_slots differs from its count / ped_off not
 * starting at 0 or decreasing / a slot with n_frames < 1 or > n_frames_max / obs_len < 2 / bad predictor parameters
 * (FOT_ERR_INVALID), pred_len > FOT_MAX_PRED_LEN or n_dense + 1 > FOT_MAX_NT (FOT_ERR_UNSUPPORTED).
 * The predictor is constant velocity, or -- after fot_loop_set_sampler, below -- the model of fot_sgan_load with the
 * library's own noise; a frame with dist_raw samples of any other producer stays with fot_loop_step.  The slots run on scenario 0 after fot_loop_begin, each on its own scenario after
 * fot_loop_begin_scenarios.
 *
 * fot_loop_run: one lock step is what the closed loop around fot_loop_step does, in this order: the replay frame and the
 * observer's clock advance (observer.py:28-102, its 1e-9 sampling tolerance, samples rounded through float32), the frame
 * of the running episodes is built ON THE DEVICE from the resident recording, the prepend decision per episode
 * (integrated_simulator.py:503-511), the body of fot_loop_step, then termination: `collision` of the new state's metrics
 * ends the episode with code 1, else s_end - s_now < goal_distance with code 2.  The step's records stay in HBM; the host
 * reads a digest of each (status, counts, cost, state updates, sample 1).  Returns the number of lock steps executed
 * (0: no episode runs any more) or a negative error.
 * Per-step outputs, entry [k][slot] of arrays sized max_steps x n_slots (any pointer may be NULL): entries of a slot that
 * does not run at step k are not written, except followed = -1.  frame / obs_*_frame: replay frame counters (row
 * min(frame, n_frames[slot] - 1) of a slot's recording); obs_last_frame / obs_prev_frame are the frames of the observer's
 * last two samples, -1 while it fills: with the staleness all a caller needs to rebuild the step's pedestrian frame and
 * prediction (fot_predict_cv) from its own copy of the recording.
 * paths non-NULL: the first n_keep samples of the 15 path arrays of the record every running slot followed, as one dense
 * block [k][15][n_slots][n_total] (fot_result array order t .. c, n_total = fot_wire_n_total), zero beyond n_keep and for
 * slots without a path; it is kept in HBM during the run and copied out once at the end of the call.
 * While a replay is set fot_loop_step on the same handle is refused (FOT_ERR_INVALID): the handle owns the clock.  The
 * next fot_loop_begin drops the replay. */
typedef struct fot_loop_replay {
    int32_t n_slots;                /* == n_episodes of fot_loop_begin */
    int32_t n_frames_max;           /* frames (rows) of pos / vel */
    int32_t obs_len, pred_len;      /* observer window; predictor (trajectory_predictor.py:188) */
    int32_t warmup_frames;
    int32_t use_footprint;          /* as fot_safety_metrics_batch */
    const int32_t *ped_off;         /* [n_slots + 1]: pedestrians of slot e = columns [ped_off[e], ped_off[e+1]) */
    const int32_t *n_frames;        /* [n_slots] recorded frames of each slot (>= 1); its last frame is held afterwards */
    const double *pos, *vel;        /* [n_frames_max][ped_off[n_slots]][2] host memory, frame 0 = time 0 before warm-up */
    fot_resample_params rp;
    double ego_radius, ped_radius;
    double s_end;                   /* arc length of the reference path's end (a scenario loop: ignored, each slot's own path's end) */
    double goal_distance;           /* the goal test's distance (2.0 m in the reference, integrated_simulator.py:873-883) */
} fot_loop_replay;
typedef struct fot_loop_run_out {
    double *ego;                    /* [max_steps][n_slots][5] the new ego states */
    double *jerk;                   /* [max_steps][n_slots] */
    int32_t *state;                 /* machine state after the step */
    int32_t *stats;                 /* [max_steps][n_slots][8], a row of -1: None */
    int32_t *followed;              /* 1: a path was followed, 0: emergency stop, -1: the slot does not run at this step */
    int32_t *keep;                  /* samples of the followed path (0: none) */
    double *cost;
    fot_safety *after;              /* metrics of the new ego states */
    double *s_now;                  /* arc length of the new state's nearest path point */
    int32_t *frame;                 /* [max_steps] replay frame of the step */
    int32_t *obs_last_frame, *obs_prev_frame;   /* [max_steps] */
    double *staleness;              /* [max_steps] */
    int32_t *steps;                 /* [n_slots] lock steps the slot has taken since fot_loop_set_replay */
    int32_t *termination;           /* [n_slots] 0: runs, 1: collision, 2: goal */
    double *paths;                  /* [max_steps][15][n_slots][n_total], or NULL */
} fot_loop_run_out;
int fot_loop_set_replay(fot_handle *h, const fot_loop_replay *replay);
int fot_loop_run(fot_handle *h, int32_t max_steps, fot_loop_run_out *out);

/* ---- per-episode summary metrics, accumulated while the resident loop runs --------------------------------------------
 * What the reference computes of an episode's whole history when it ends (calculate_aggregate_metrics,
 * src/core/metrics.py:272-320; one row of metrics_summary.csv), restricted to what a replayed loop with the
 * constant-velocity predictor produces.  Per slot, over its L = steps lock steps so far:
 *   - from every step's NEW ego state and the metrics of that state (fot_loop_run_out.after): min_dist, collision_count,
 *     min_ttc (over steps with 0 < ttc < inf, else inf), max / mean / rms of |jerk|, max / mean of |a|; L = 0 gives the
 *     reference's values of an empty history (0, 0, inf, 0 ...);
 *   - prediction error against the recording.  Step i's prediction is the dense track [P][n_dense][2] without the
 *     prepended current position; d_i[p][k] = Euclidean distance of dense sample k to the pedestrian's position at step
 *     i + 1 + k, recording row min(frame_i + 1 + k, n_frames[slot] - 1).
 *       planning_ade / planning_fde / planning_eval_count (metrics.py:225-269): E = min(n_dense, L - (i + 1)), origins
 *       with E == 0 skipped; sum_p mean_{k<E} d_i[p][k] and sum_p d_i[p][E-1] over the origins, divided by the count (+= P).
 *       ade / fde / ade_eval_count (metrics.py:31-114): stride = round(sgan_dt / sim_dt), samples k = stride j - 1,
 *       j = 1 .. pred_len; an origin counts if n_dense > stride pred_len - 1 and i + stride pred_len < L.
 *       ade_per_agent / fde_per_agent: equal to ade / fde (the constant-velocity predictor's samples are identical, so
 *       best-of-N picks nothing; a multi-sample predictor's loop gets them from fot_loop_prediction_scores);
 *       pred_samples: num_samples of fot_loop_summary_enable if an origin counted, else 0.
 *       nll = NaN, nll_eval_count = 0 (identical samples are skipped, metrics.py:155-158).
 *     Steps without a prediction (observer not ready) and slots without pedestrians contribute nothing; with no counted
 *     origin the means are NaN and the counts 0.
 *   - steps, termination (0: runs, 1: collision, 2: goal), total_time = steps * dt.
 * fot_loop_summary_enable: between fot_loop_set_replay and the first step of a run (on = 0 switches it off again).  A
 * loop that never enables it launches and allocates nothing for it.  With it, every lock step launches one more kernel
 * behind the prediction (no host synchronisation): per running slot the row c_i[k] = sum_p d_i[p][k] goes into a ring of
 * n_dense rows in HBM, and the row it replaces -- its horizon is complete by then -- is folded into running totals.
 * fot_loop_summaries folds the ring's remaining rows with their truncated horizons into a COPY of the totals, so it may
 * be called between two fot_loop_run calls and the run goes on.  A slot's numbers do not depend on the other slots.
 * Refusals (FOT_ERR_INVALID, a refused call changes nothing): no replay set; sgan_dt / sim_dt not an integer; num_samples
 * < 1; enabling or disabling after the first step; n_slots differing from the loop's; summaries not enabled; out NULL.
 * fot_loop_begin* drops the accumulators with the replay. */
typedef struct fot_loop_summary {
    double min_dist, min_ttc;
    double max_jerk, mean_jerk, rms_jerk, max_accel, mean_accel;
    double ade, fde, ade_per_agent, fde_per_agent;
    double planning_ade, planning_fde;
    double nll;
    double total_time;
    int32_t collision_count, pred_samples, ade_eval_count, planning_eval_count, nll_eval_count;
    int32_t steps, termination, _pad;
} fot_loop_summary;
int fot_loop_summary_enable(fot_handle *h, int32_t on, int32_t num_samples);
int fot_loop_summaries(fot_handle *h, int32_t n_slots, fot_loop_summary *out);

/* ---- prediction scores: best-of-N ADE / FDE and the KDE log-likelihood of a sample distribution, on the device --------
 * The six keys of the reference's summary that compare predictors (calculate_aggregate_metrics, src/core/metrics.py:
 * 272-320: ade, fde, ade_per_agent, fde_per_agent, nll, nll_eval_count) are functions of the whole [S][P][T][2] sample
 * distribution of every step.  One record per prediction origin holds what that origin contributes
 * (_standard_ade_fde_details :31-114, _kde_nll_details :117-176), computed by one workgroup from the tensor where it lies.
 * With q[s][p][k] dense sample k of the origin's block (the prepended current position skipped: `skip`), evaluation
 * indices k_j = stride j - 1, j = 1 .. E, truth g[p][j] and d[s][p][j] = |q[s][p][k_j] - g[p][j]|:
 *   ade_scene = min_s mean_{p, j} d                      fde_scene = min_s mean_p d[s][p][E]      (one sample per scene)
 *   ade_agent_sum = sum_p min_s mean_j d[s][p][j]        fde_agent_sum = sum_p min_s d[s][p][E]   (minADE / minFDE)
 *   log_lik_sum, nll_count: evaluated only if S >= 2 and the samples differ somewhere ((p, j, axis) with max_s != min_s;
 *   otherwise 0 / 0 and FOT_PRED_NLL not set, :155-158).  Per (p, j) and axis the bandwidth b = max(std_s(q, ddof = 1)
 *   S^(-1/6), 0.05) with a two-pass standard deviation; l_s = -1/2 sum_axis ((q - g) / b)^2 - log(2 pi b_x b_y);
 *   log p = max(max_s l + log(mean_s exp(l_s - max l)), -20); log_lik_sum = sum_{p, j} log p, nll_count = P E.
 * All of it in float64 whatever the tensor's element type (a float32 tensor gives the scores of the rounded samples), every
 * reduction in an order fixed by (S, P, E) alone, no floating-point atomics: an origin's record is byte-identical alone
 * and inside any batch.  flags: FOT_PRED_NLL; FOT_PRED_NONFINITE: a sample at an evaluation index or a truth coordinate
 * was not finite -- the terms it enters are NaN, as NumPy's min / maximum give.  An episode folds the records of its
 * origins with a complete horizon in step order as the reference does: total_ade += ade_scene n_peds, total_fde +=
 * fde_scene n_peds, the agent sums and log_lik_sum as they are, counts += n_peds / nll_count; ade = total_ade / count ...,
 * nll = -log_lik / nll_eval_count.
 *
 * fot_prediction_scores (stateless, synchronous): origin i's block starts at POINT desc[i].offset of `tensor` (host memory,
 * or device memory with on_device != 0; dtype FOT_F32 | FOT_F64), laid out [S][P][T][2] (layout 0) or [T][S][P][2]
 * (FOT_DYN_LAYOUT_TSP); skip 1: sample 0 of every track is the prepended current position.  truth: host [sum P][E][2]
 * float64, the origins' pedestrians one after the other; out: host, n_origins records.  stream NULL = the handle's.
 * P = 0 gives a zero record (n_peds 0).  Refusals, a refused call changes nothing: stride < 1, E < 1, S < 1, P < 0,
 * stride E - 1 >= T - skip, skip not 0 / 1, a negative offset, an unknown layout or dtype (FOT_ERR_INVALID); S >
 * the handle's sample capacity or E > FOT_MAX_PRED_LEN -- the kernel keeps E truth points per pedestrian of a tile in LDS
 * (FOT_ERR_UNSUPPORTED).
 * fot_loop_prediction_scores: the same for the distribution blocks the most recent fot_loop_step / fot_loop_plan frame
 * with dist_raw left in the handle's own tensor (float64, [dist_S][P_e][n_dense + 1][2], skip 1): n_episodes == the
 * frame's, truth [sum P][E][2] in the frame's pedestrian order.  The samples stay in HBM; the call is enqueued on the
 * loop's stream and synchronises once.  FOT_ERR_INVALID when the last frame carried no distribution, n_episodes differs,
 * or a replay is set (fot_loop_run owns the handle's tensor then). */
#define FOT_PRED_NLL 1
#define FOT_PRED_NONFINITE 2
typedef struct fot_pred_origin {
    int64_t offset;                 /* first point (2-vector) of the block in the tensor */
    int32_t S, P, T;                /* samples, pedestrians, entries per track (the prepended one included) */
    int32_t layout;                 /* 0 | FOT_DYN_LAYOUT_TSP */
    int32_t skip;                   /* 0 | 1 */
    int32_t _pad;
} fot_pred_origin;
typedef struct fot_pred_score {
    double ade_scene, fde_scene, ade_agent_sum, fde_agent_sum, log_lik_sum;
    int32_t n_peds, n_samples, nll_count, flags;
} fot_pred_score;
int fot_prediction_scores(fot_handle *h, int32_t n_origins, const fot_pred_origin *desc, const void *tensor, int32_t dtype,
                          int32_t on_device, int32_t stride, int32_t E, const double *truth, fot_pred_score *out,
                          void *stream);
int fot_loop_prediction_scores(fot_handle *h, int32_t n_episodes, int32_t stride, int32_t E, const double *truth,
                               fot_pred_score *out);

/* ---- Social-GAN sample generation on the device -------------------------------------------------------------------------
 * float32 inference of the reference's default predictor (src/prediction/sgan_vendor/models.py, TrajectoryGenerator.forward
 * in eval mode, then relative_to_abs) for many scenes at once; a scene is one episode's pedestrians.  What the reference
 * runs as num_samples forward passes (trajectory_predictor.py:340-346) is one call: the encoder runs once per pedestrian,
 * the first pooling and the context MLP once per scene, and only the part behind the noise once per sample.  The output
 * [S][pred_len][sum P][2] float32 is what fot_loop_frame.dist_raw and fot_resample_predictions read.
 *
 * Supported: num_layers 1; pooling none ('lstm') or the pool net ('sgan'), also at every decoder step; noise mixed per
 * pedestrian or per scene; a noise_dim of one entry, 0 included (without noise and pooling and with encoder_h_dim ==
 * decoder_h_dim the context MLP is absent, as in the reference).  BatchNorm is an eval-mode affine map: the caller folds
 * it into the Linear in front of it, the library never sees it.  FOT_ERR_UNSUPPORTED: social pooling (FOT_SGAN_SPOOL),
 * dropout > 0, num_layers > 1, a dimension above its FOT_SGAN_MAX_*, pred_len > FOT_MAX_PRED_LEN, S > the handle's sample capacity,
 * a scene of more than FOT_SGAN_MAX_PEDS pedestrians.
 *
 * Weights: ONE packed float32 blob, every matrix row-major [out][in] as torch stores it, LSTM gates in torch's order
 * i, f, g, o, with E = embedding_dim, He / Hd = encoder / decoder_h_dim, M = mlp_dim, B = bottleneck_dim, nd = noise_dim:
 *   encoder      spatial_embedding W [E][2], b [E]; LSTM W_ih [4 He][E], W_hh [4 He][He], b_ih [4 He], b_hh [4 He]
 *   pool net     (pooling) spatial_embedding W [E][2], b [E]; W [512][E + He], b [512]; W [B][512], b [B]
 *   context MLP  (noise, pooling or He != Hd) W [M][He + B], b [M]; W [Hd - nd][M], b [Hd - nd]   (B = 0 without pooling)
 *   decoder      spatial_embedding W [E][2], b [E]; LSTM W_ih [4 Hd][E], W_hh [4 Hd][Hd], b_ih [4 Hd], b_hh [4 Hd];
 *                hidden2pos W [2][Hd], b [2]
 *   per step     (pooling and pool_every_timestep) pool net as above with Hd for He; MLP W [M][Hd + B], b [M]; W [Hd][M], b [Hd]
 * fot_sgan_weight_count gives the blob's length for a descriptor (no handle, no device: it also answers the refusals
 * above).  fot_sgan_load replaces the handle's model; fot_sgan_unload drops it.
 *
 * fot_sgan_sample (synchronous: `out` is written when it returns; enqueued on `stream`, NULL = the handle's):
 *   ped_off [n_scenes + 1] host, non-decreasing from 0; empty scenes are allowed
 *   obs     [obs_len][sum P][2] float32 absolute positions (the observer's window); the displacements the model reads are
 *           formed here: row 0 zero, row t = obs[t] - obs[t - 1] in float32 (observer.py:126-135)
 *   noise   [S][rows][nd] float32, rows = sum P (FOT_SGAN_NOISE_PED) or n_scenes (FOT_SGAN_NOISE_GLOBAL); may be NULL when
 *           nd == 0.  The caller draws it (the reference takes the same through user_noise)
 *   flags   FOT_OUT_DEVICE: out is device memory; FOT_SGAN_OBS_DEVICE / FOT_SGAN_NOISE_DEVICE: so is obs / noise
 *   out     [S][pred_len][sum P][2] float32 absolute positions
 * Every output element is one thread's sum in index order and the pool's max is exact in any order: a scene's numbers are
 * the same bits alone and inside any launch, whatever the placement of the tensors.
 * FOT_ERR_INVALID, nothing changed: no model loaded, n_scenes < 0, offsets not starting at 0 or decreasing, S < 1, a NULL
 * tensor that is needed; fot_sgan_load with n other than fot_sgan_weight_count's. */
#define FOT_SGAN_MAX_EMBEDDING 64
#define FOT_SGAN_MAX_HIDDEN 128      /* encoder_h_dim, decoder_h_dim */
#define FOT_SGAN_MAX_MLP 1024
#define FOT_SGAN_MAX_BOTTLENECK 1024
#define FOT_SGAN_MAX_OBS_LEN 32
#define FOT_SGAN_MAX_PEDS 256        /* pedestrians of one scene */
#define FOT_SGAN_POOL_HIDDEN 512     /* first layer of the pool net: fixed by the reference (models.py:159) */
#define FOT_SGAN_POOL_NONE 0
#define FOT_SGAN_POOL_NET 1
#define FOT_SGAN_SPOOL 2
#define FOT_SGAN_NOISE_PED 0
#define FOT_SGAN_NOISE_GLOBAL 1
#define FOT_SGAN_OBS_DEVICE 4
#define FOT_SGAN_NOISE_DEVICE 8
typedef struct fot_sgan_desc {
    int32_t obs_len, pred_len;
    int32_t embedding_dim, encoder_h_dim, decoder_h_dim, mlp_dim, bottleneck_dim, noise_dim;
    int32_t num_layers;
    int32_t pooling_type;           /* FOT_SGAN_POOL_NONE | FOT_SGAN_POOL_NET | FOT_SGAN_SPOOL (refused) */
    int32_t pool_every_timestep;    /* counts only with pooling (models.py:81) */
    int32_t noise_mix_type;         /* FOT_SGAN_NOISE_PED | FOT_SGAN_NOISE_GLOBAL */
    float dropout;                  /* > 0 is refused */
    int32_t _pad;
} fot_sgan_desc;
int fot_sgan_weight_count(const fot_sgan_desc *desc, int64_t *n);
int fot_sgan_load(fot_handle *h, const fot_sgan_desc *desc, int64_t n, const float *weights);
int fot_sgan_unload(fot_handle *h);
int fot_sgan_sample(fot_handle *h, int32_t n_scenes, const int32_t *ped_off, const void *obs, int32_t S, const void *noise,
                    int32_t flags, void *out, void *stream);

/* ---- counter-based noise for the sampler, and the resident loop's Social-GAN predictor -------------------------------------
 * fot_sgan_noise writes the tensor [S][rows][noise_dim] that fot_sgan_sample takes as `noise`, drawn by the library itself:
 * Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; 10 rounds) with
 *   key     = the 64-bit seed, low word first
 *   counter = { b = d / 4, p | (s << 16), step, slot }
 * for dimension d of sample s of the row that is pedestrian p of slot `row_slot[r]` (row_index[r]: its index WITHIN the
 * slot; 0 for a model with noise per scene, FOT_SGAN_NOISE_GLOBAL, whose rows are scenes) at that slot's own step count
 * row_step[r] (fot_loop_run_out.steps before the step).  One block x0 .. x3 yields dimensions 4 b .. 4 b + 3:
 *   FOT_NOISE_RAW          the uint32 words themselves (what bit-for-bit tests read)
 *   FOT_NOISE_UNIFORM      (x >> 8) 2^-24, torch.rand's [0, 1)
 *   FOT_NOISE_UNIFORM_SYM  (uniform - 0.5) 2: the reference's noise_type 'uniform' (sgan_vendor/models.py get_noise), [-1, 1)
 *   FOT_NOISE_GAUSSIAN     Box-Muller on (x0, x1) and (x2, x3): u1 = ((x >> 8) + 1) 2^-24 in (0, 1], u2 = (x' >> 8) 2^-24,
 *                          r = sqrt(-2 ln u1), outputs r cos(2 pi u2), r sin(2 pi u2), in float64, rounded once to float32
 * A number is a function of (seed, slot, step, p, s, d) alone -- no atomics, nothing of the launch shape or of the other
 * rows -- so a stepwise caller can ask for exactly the noise a resident loop used for any subset of slots at any step.  In
 * a loop whose slots share their crowds' samples (fot_loop_set_sampler_shared, below) the `slot` word is the CROWD's id:
 * row_slot = crowd id, row_step and row_index reproduce any step of such a loop, and crowd c draws what slot c of a loop
 * without crowds draws.  It
 * is NOT torch.randn's stream: seeds are not comparable with the reference's runs.  (To run a resident loop on the
 * reference's own samples, record them once and hand the tensor to fot_loop_set_samples, below.)
 * row_slot / row_step / row_index: host [rows]; flags FOT_OUT_DEVICE: out is device memory.  Synchronous, enqueued on
 * `stream` (NULL = the handle's).  No model needs to be loaded.  FOT_ERR_INVALID, nothing changed: an unknown kind or
 * flag, S < 1, rows < 0, noise_dim < 0, a NULL table or `out` that is needed, a negative table entry, row_index > 65535;
 * FOT_ERR_UNSUPPORTED: S > the handle's sample capacity.
 *
 * fot_loop_set_sampler(h, S, seed, kind): between fot_loop_set_replay and the first step.  The resident loop then predicts
 * with the model of fot_sgan_load instead of constant velocity: once the observer is ready, a step gathers the window
 * [obs_len][rows][2] float32 from the recording in HBM (the observer's sample frames, clamped to each slot's recording),
 * draws the noise above (kind: FOT_NOISE_GAUSSIAN | FOT_NOISE_UNIFORM_SYM) for the running slots at their step counts,
 * runs the sampler and resamples the S samples into each episode's [S][P_e][n_dense + 1][2] block, the current positions
 * leading every sample -- what fot_loop_step makes of a frame with dist_raw.  Nothing is synchronised and nothing crosses
 * the bus in between; level 0, the escalation levels, the resolve and the history run as without a sampler.  seed, slot
 * and fot_loop_run_out.steps reproduce any step's noise through fot_sgan_noise.
 * Refusals, a refused call changes nothing.  FOT_ERR_INVALID: no replay set; no model loaded; after the first step; S < 1;
 * an unknown kind; the model's obs_len / pred_len differ from the replay's.  FOT_ERR_UNSUPPORTED: S > the handle's sample capacity; a
 * slot of more than FOT_SGAN_MAX_PEDS pedestrians; a loop begun with fot_loop_begin_scenarios; summaries enabled
 * (fot_loop_summary_enable is refused in turn while a sampler is set: its prediction-error ring reads the
 * constant-velocity tensor's layout).  fot_sgan_load / fot_sgan_unload are refused (FOT_ERR_INVALID) while a sampler is
 * set; fot_loop_begin* and fot_loop_set_replay drop the sampler.
 * Both entries are additions: no structure, capacity or existing entry changes, so FOT_ABI_VERSION and the words of
 * fot_abi_info stay as they are; a binding that needs the entries looks the symbols up. */
#define FOT_NOISE_RAW 0
#define FOT_NOISE_UNIFORM 1
#define FOT_NOISE_GAUSSIAN 2
#define FOT_NOISE_UNIFORM_SYM 3
#define FOT_NOISE_KINDS 4
int fot_sgan_noise(fot_handle *h, uint64_t seed, int32_t kind, int32_t S, int32_t rows, int32_t noise_dim,
                   const int32_t *row_slot, const int32_t *row_step, const int32_t *row_index, int32_t flags, void *out,
                   void *stream);
int fot_loop_set_sampler(fot_handle *h, int32_t S, uint64_t seed, int32_t kind);

/* ---- prediction scores and episode summaries of a resident loop with a sampler or a recording (fot_loop_set_samples) ----
 * fot_loop_scores_enable(h, on): between fot_loop_set_sampler / fot_loop_set_samples and the first step (on = 0 switches
 * it off again).  Every
 * sampled lock step then, on the loop's stream behind the resample and ahead of the safety and plan launches and without
 * a synchronisation of its own,
 *   - chooses every running episode's representative sample (predict_single_best, trajectory_predictor.py:346-351): over
 *     the episode's own pedestrians and the n_dense dense samples (the prepended current position is not part of it)
 *     dev[s] = sum_{p,k} |q[s][p][k] - mean_s q[.][p][k]|, the first minimum (S = 1: sample 0);
 *   - writes that sample's error row into the prediction-error ring of fot_loop_summary_enable (planning_ade,
 *     planning_fde, planning_eval_count: the reference evaluates them on predicted_trajectories, the representative sample);
 *   - scores the whole distribution where it lies in HBM, one fot_pred_score record per running episode as
 *     fot_loop_prediction_scores gives it (skip = 1, float64), against the resident recording: the truth of origin frame f
 *     is row min(f + stride j, n_frames[slot] - 1), j = 1 .. pred_len, stride = round(sgan_dt / sim_dt).  The records land
 *     in pinned memory and are folded per slot on the host once their horizon is complete: the record of a slot's step i
 *     counts when the slot takes step i + stride pred_len (metrics.py:78), ade_scene n_peds, fde_scene n_peds, the agent
 *     sums and log_lik_sum added in step order, the counts n_peds and nll_count beside them.
 * Everything the mode needs is allocated here.  With stride pred_len - 1 >= n_dense no origin ever has a complete horizon
 * and ade .. nll stay NaN / 0 (accepted, as the reference does).  A loop that does not enable the mode launches and
 * allocates nothing of this, and its steps' outputs are the same bytes with the mode on and off.
 * Refusals (FOT_ERR_INVALID, nothing changed): no replay set; neither a sampler nor a recording set; after the first
 * step; sgan_dt / sim_dt not an integer.  fot_loop_begin*, fot_loop_set_replay, fot_loop_set_sampler and
 * fot_loop_set_samples drop the mode, as they drop the sampler or the recording.
 *
 * fot_loop_score_summaries(h, n_slots, out): one fot_loop_summary per slot of the steps run so far; may be called between
 * two fot_loop_run calls, the run goes on.  min_dist .. mean_accel, steps, termination, total_time: as fot_loop_summaries.
 * ade, fde (scene-level best-of-N), ade_per_agent, fde_per_agent, ade_eval_count, nll, nll_eval_count, pred_samples (S if
 * an origin counted, else 0): the fold above; records whose horizon is not complete yet do not count.  planning_ade,
 * planning_fde, planning_eval_count: the ring, with the truncated horizon E = min(n_dense, L - (i + 1)).
 * FOT_ERR_INVALID: scores not enabled; n_slots differs from the loop's; out is NULL.
 *
 * fot_loop_last_best_sample(h, n_slots, out): out[slot] = the representative sample the most recent lock step chose for
 * the slot; -1: the slot did not run, the step did not predict (observer not ready), or the slot has no pedestrians.
 * Together with seed, slot and step it rebuilds a step's predicted_trajectories without redoing the selection.
 * FOT_ERR_INVALID as above.
 * The three entries are additions: no structure, capacity or existing entry changes, FOT_ABI_VERSION and the words of
 * fot_abi_info stay as they are; a binding that needs them looks the symbols up. */
int fot_loop_scores_enable(fot_handle *h, int32_t on);
int fot_loop_score_summaries(fot_handle *h, int32_t n_slots, fot_loop_summary *out);
int fot_loop_last_best_sample(fot_handle *h, int32_t n_slots, int32_t *out);

/* ---- planning on the representative prediction sample (the reference's default: distribution_aware_planning = False,
 *      integrated_simulator.py:447-455, 503-513), the samples never leaving HBM ----
 * fot_loop_plan_sample(h, mode): what the requests of a lock step plan against when its frame carries a distribution
 * (fot_loop_frame.dist_raw; the sampled step of a fot_loop_run with a sampler or a recording):
 *   FOT_LOOP_PLAN_DISTRIBUTION    the whole distribution under the chance constraint (the default)
 *   FOT_LOOP_PLAN_REPRESENTATIVE  every episode's representative sample (predict_single_best: the sample closest to the
 *                                 sample mean over the episode's own pedestrians, the selection of fot_loop_scores_enable),
 *                                 as FOT_DYN_SINGLE with S = 1; chance_epsilon plays no part, collision_margin_inflation
 *                                 applies as in any single-sample plan.  The escalation levels plan against the same block.
 * The frame is resampled into the distribution blocks as before (fot_loop_prediction_scores and the scores of a resident
 * loop read them unchanged); the selection and one more kernel follow on the same stream and leave, per episode, ONE block
 * [P_e][n_dense + 1][2] whatever the reference's conditional prepend decides:
 *   prepended      [current, dense[0], ..., dense[n_dense - 1]]
 *   not prepended  [dense[0], ..., dense[n_dense - 1], dense[n_dense - 1]]     (the last entry once more)
 * The episode prepends unless |dense[0] - current| <= 1e-8 + 1e-5 |current| holds for all its pedestrians on both axes
 * (np.allclose; a NaN makes it false).  The second form is the same obstacle as the reference's [P_e][n_dense][2]: the
 * collision check clips its time index to the last entry (frenet_planner.py:1226-1227), and a track's min / max box and
 * the NaN-track rule do not see a repeated entry.  dist_S = 1 selects sample 0 and goes through the same rule.  A frame
 * without dist_raw (observer not ready, constant velocity) behaves as in mode 0.
 * Allowed after fot_loop_begin; with a replay set only before the run's first step.  fot_loop_begin* resets the mode to
 * FOT_LOOP_PLAN_DISTRIBUTION.  With the mode on fot_loop_last_best_sample answers for stepwise loops too (the slots of
 * fot_loop_begin; fot_loop_plan's episode i is slot i).  What the mode needs is allocated when it is switched on or grows
 * with the frames; a loop that never switches it on launches and allocates nothing new.
 * FOT_ERR_INVALID (nothing changed): unknown mode; no loop begun; after a resident run's first step.
 * FOT_ERR_UNSUPPORTED (nothing changed): a loop begun with fot_loop_begin_scenarios.
 *
 * fot_loop_run_best_samples(h, n_steps, n_slots, out): fot_loop_last_best_sample for every lock step of the most recent
 * fot_loop_run call, out[k][slot], k < n_steps = that call's return value -- a run of many steps per call keeps what each
 * step planned on.  FOT_ERR_INVALID: no replay set, the mode is off, n_steps or n_slots differ from the call's.
 *
 * fot_debug_loop_block (tests): the block the most recent frame's `episode` (index in the frame) plans against, copied
 * to xy[cap_points][2], with its pedestrians *P and time entries *T.  Mode 1 with a distribution: the [P][n_dense + 1][2]
 * block above and *prepended = 1 / 0 (-1 without pedestrians); otherwise the episode's block of the handle's tensor
 * ([dist_S][P][T][2] of a distribution) and *prepended = -1.  Synchronous.  FOT_ERR_INVALID: no frame, episode out of
 * range, a block of more than cap_points points (*P and *T are set).
 * Additions only: FOT_ABI_VERSION and the words of fot_abi_info stay as they are. */
#define FOT_LOOP_PLAN_DISTRIBUTION 0
#define FOT_LOOP_PLAN_REPRESENTATIVE 1
int fot_loop_plan_sample(fot_handle *h, int32_t mode);
int fot_loop_run_best_samples(fot_handle *h, int32_t n_steps, int32_t n_slots, int32_t *out);
int fot_debug_loop_block(fot_handle *h, int32_t episode, int32_t cap_points, double *xy, int32_t *P, int32_t *T,
                         int32_t *prepended);

/* ---- a resident loop that predicts from a recorded sample tensor -------------------------------------------------------
 * With replayed pedestrians the observer's window does not depend on the ego, so neither does the predictor's output: the
 * samples of a run can be produced once, by anything -- the reference's own generator on PyTorch under torch.manual_seed,
 * an LSTM, a scripted source -- and stay exact for every planner configuration run over the same recording.  This is
 * the way to run resident on the reference's own samples; the sampler's seeds above stay incomparable with them.
 *
 * fot_loop_set_samples(h, S, n_steps, first_step, samples, dtype, flags): between fot_loop_set_replay and the first step,
 * where fot_loop_set_sampler would be called.  samples is [n_steps][S][pred_len][n_cols][2], n_cols = ped_off[n_slots] of
 * the replay (the columns of all slots in the replay's own order), pred_len the replay's, dtype FOT_F32 | FOT_F64.  Row r
 * belongs to lock step first_step + r, counted since fot_loop_set_replay (fot_loop_run_out.steps of a running slot before
 * the step); its values are raw predictions on the predictor's own time step anchored at the observer's last sample --
 * what fot_loop_frame.dist_raw carries for one step.  Without FOT_OUT_DEVICE the tensor is host memory and copied to HBM
 * once, here; with it, device memory (aligned to one [x, y] element) that is used in place and never written: the caller
 * has finished writing it before the call and keeps it alive until the next fot_loop_begin*, fot_loop_set_replay or
 * fot_loop_set_samples on the handle, so one tensor serves a whole sweep of loops without a copy.
 * A step of fot_loop_run then predicts from the recording where it would have predicted with a sampler (observer ready,
 * a running slot with pedestrians): behind the frame kernel one gather (k_loop_sample_rows) forms the step's raw tensor
 * [S][pred_len][rows][2] of the running slots from row step - first_step, in the recording's own element type, and the
 * ragged resample of the sampler branch lays every episode's [S][P_e][n_dense + 1][2] float64 block out, the current
 * positions leading every sample.  Level 0, the escalation levels, the resolve and the history follow as behind a sampler;
 * fot_loop_scores_enable, fot_loop_score_summaries, fot_loop_last_best_sample, fot_loop_plan_sample, fot_loop_run_best_samples
 * and fot_debug_loop_block work as they do there.  Steps that do not predict read nothing: their rows may hold anything.
 * A step that would predict but lies outside [first_step, first_step + n_steps) is not run: fot_loop_run stops before it
 * and returns the steps executed, or FOT_ERR_INVALID (the step is named in fot_last_error) if there were none.
 * Sampler and recording exclude each other (FOT_ERR_INVALID for the second of the two); fot_loop_summary_enable stays
 * refused as with a sampler; fot_loop_begin* and fot_loop_set_replay drop the recording.  No model needs to be loaded, and
 * fot_sgan_load / fot_sgan_unload stay allowed.  Everything the mode needs is allocated here; a loop that never calls the
 * entry launches and allocates nothing new.
 * Refusals, a refused call changes nothing.  FOT_ERR_INVALID: no replay set; after the first step; S < 1; n_steps < 1;
 * first_step < 0; samples NULL (or device memory not aligned to an element); an unknown dtype or flag; a sampler set.
 * FOT_ERR_UNSUPPORTED: S > the handle's sample capacity; a loop begun with fot_loop_begin_scenarios; summaries enabled.
 * An addition: FOT_ABI_VERSION and the words of fot_abi_info stay as they are; a binding looks the symbol up. */
int fot_loop_set_samples(fot_handle *h, int32_t S, int32_t n_steps, int32_t first_step, const void *samples, int32_t dtype,
                         int32_t flags);

/* ---- sweep loops: every slot on its own scenario AND in its own plan mode over sample distributions ---------------------
 * A campaign runs one crowd and one predictor output under conditions that differ in the plan mode (the representative
 * sample against the whole distribution), chance_epsilon and collision_margin_inflation.  One loop runs such a sweep.
 *
 * fot_loop_begin_sweep(h, n_episodes, n_cfg, cfg, use_footprint, slot_scenario, slot_plan_mode, ego5):
 * fot_loop_begin_scenarios -- the same arguments, the same refusals -- plus slot_plan_mode[e], FOT_LOOP_PLAN_DISTRIBUTION
 * or FOT_LOOP_PLAN_REPRESENTATIVE; NULL: every slot plans against the distribution; any other value: FOT_ERR_INVALID
 * (nothing changed).  The loop is a scenario loop in every respect, except that a lock step with a distribution is
 * accepted: fot_loop_step takes a frame with dist_raw, fot_loop_set_sampler and fot_loop_set_samples(_shared) are allowed.
 * Such a step resamples the frame into every episode's [dist_S][P_e][n_dense + 1][2] block as a one-configuration loop
 * does; the episodes in representative mode then choose their sample and leave their [P_e][n_dense + 1][2] planning block
 * (fot_loop_plan_sample above: the same selection, the same prepend rule) BEHIND the step's distribution blocks in the
 * same tensor, compacted in frame order.  One plan call serves all requests: a request addresses its episode's
 * distribution block as FOT_DYN_DISTRIBUTION with dist_S samples, or its planning block as FOT_DYN_SINGLE with one, each
 * on its slot's scenario -- chance_epsilon and collision_margin_inflation are the scenario's, and in representative mode
 * chance_epsilon plays no part.  The escalation levels plan against the same block in the same mode as their episode's
 * level 0.  An episode's numbers are the bits it computes in a uniform loop of its own configuration and mode, whatever
 * its company.  A frame or step without a distribution plans as a scenario loop does (the same bytes).
 * fot_loop_scores_enable, fot_loop_score_summaries, fot_loop_last_best_sample, fot_loop_run_best_samples work as on a
 * fot_loop_begin loop; the two best-sample queries answer -1 for a slot in distribution mode unless scores are enabled
 * (the selection then runs for every running episode).  fot_debug_loop_block answers per episode in that episode's mode.
 * fot_loop_plan_sample: FOT_ERR_INVALID, the modes were given per slot.  fot_loop_summary_enable: as on any loop, allowed
 * with constant velocity, refused while a sampler or a recording is set.  fot_loop_begin* ends the sweep loop.
 * What the sweep needs is allocated by fot_loop_set_sampler / fot_loop_set_samples(_shared) or grows with the frames.
 *
 * fot_loop_set_samples_shared(h, S, n_steps, first_step, samples, dtype, flags, n_rec_cols, slot_col0):
 * fot_loop_set_samples for a recording [n_steps][S][pred_len][n_rec_cols][2] whose columns are not the replay's:
 * pedestrian p of slot e reads column slot_col0[e] + p, and several slots may name the same columns -- K conditions over
 * one crowd keep ONE copy of its samples in HBM.  fot_loop_set_samples is this call with n_rec_cols = ped_off[n_slots] and
 * slot_col0 = ped_off.  When it may be called, the in-place use of a device tensor, the rows that are read and the
 * refusals are fot_loop_set_samples's (a fot_loop_begin_scenarios loop included); allowed on fot_loop_begin loops and on
 * sweep loops.  Further FOT_ERR_INVALID (nothing changed): slot_col0 NULL; an entry < 0; slot_col0[e] + P_e > n_rec_cols;
 * n_rec_cols < 1 with pedestrians in the replay.
 * Both entries are additions: no structure, capacity or existing entry changes, FOT_ABI_VERSION and the words of
 * fot_abi_info stay as they are; a loop that never calls them launches and allocates nothing new.
 *
 * fot_loop_set_sampler_shared(h, S, seed, kind, n_crowds, slot_crowd): fot_loop_set_sampler for slots that share crowds --
 * the K conditions of a sweep over one crowd.  slot_crowd[e] in [0, n_crowds) names slot e's crowd; the ids need not be
 * dense.  With replayed pedestrians the observer's window does not depend on the ego, so every lock step the library
 * samples each ACTIVE crowd -- one with a running slot that has pedestrians -- ONCE: the active crowds in ascending id are
 * the generator's scenes, a scene's window is that of the crowd's lowest running slot, and the noise counter's `slot` word
 * is the crowd's id, its `step` word the slots' step count (all slots of a resident loop start at fot_loop_set_replay, so
 * the running ones agree).  The crowds' raw samples [S][pred_len][crowd rows][2] are then gathered into the step's raw
 * tensor of the running episodes, and everything behind it -- resampling, selection, planning blocks, scores, safety, the
 * plan, each slot in its own mode and on its own scenario -- runs per slot as before.  Every condition of a cell therefore
 * plans against the SAME samples, crowd c draws exactly what slot c of a loop without crowds draws, and
 * fot_sgan_noise(seed, ..., row_slot = crowd id, row_step, row_index) reproduces any step.  fot_loop_set_sampler is this
 * call with slot_crowd[e] = e: the launches and bytes of before.  When it may be called and the refusals are
 * fot_loop_set_sampler's (fot_loop_begin loops and sweep loops); further FOT_ERR_INVALID, nothing changed: slot_crowd NULL
 * or n_crowds < 1; an id outside [0, n_crowds); two slots of one crowd that differ in their pedestrian count, in n_frames,
 * or in any byte of their columns of `pos` over their recorded frames (compared once, on the host, by this call; the
 * message names both slots).  Everything the mode needs is allocated by the call; fot_loop_begin* and fot_loop_set_replay
 * drop it with the sampler.  Not supported: one distribution block per crowd (resampling, selection and scores still run
 * per slot, as for a shared recording), S > the handle's sample capacity, crowds whose slots stand at different step counts.
 *
 * fot_debug_loop_sampler_shape (tests): the scenes and pedestrian rows the most recent lock step handed to the generator --
 * 0 / 0 if that step did not sample; FOT_ERR_INVALID without a sampler.  It shows that the work was shared, not only the
 * numbers.
 * Both entries are additions as well: FOT_ABI_VERSION stays, a binding that needs them looks the symbols up. */
int fot_loop_set_sampler_shared(fot_handle *h, int32_t S, uint64_t seed, int32_t kind, int32_t n_crowds,
                                const int32_t *slot_crowd);
int fot_debug_loop_sampler_shape(fot_handle *h, int32_t *n_scenes, int32_t *n_rows);
int fot_loop_begin_sweep(fot_handle *h, int32_t n_episodes, int32_t n_cfg, const fot_loop_config *cfg,
                         const int32_t *use_footprint, const int32_t *slot_scenario, const int32_t *slot_plan_mode,
                         const double *ego5);

/* ---- several Social-GAN models per handle, and a model per slot of a sampler loop --------------------------------------------
 * A handle holds up to fot_sgan_max_models() (8) loaded models, each with its own device image and work arrays: what model m
 * computes never depends on what else is loaded or was sampled in between.  fot_sgan_load_model / fot_sgan_unload_model /
 * fot_sgan_sample_model take the model's id in front of the arguments of fot_sgan_load / fot_sgan_unload / fot_sgan_sample,
 * which are these entries with model = 0: their behaviour, launches and bytes are as before.  FOT_ERR_INVALID, nothing
 * changed: a model outside 0 .. fot_sgan_max_models() - 1; sampling or unloading a model that is not loaded; a load or
 * unload of ANY model while a loop sampler is set.  fot_destroy releases all models.
 *
 * fot_loop_set_sampler_models(h, S, seed, n_models, model_kind, n_crowds, slot_crowd, slot_model): fot_loop_set_sampler_shared
 * for slots that also name their model -- the 'sgan' and 'lstm' conditions of a campaign cell in ONE loop.  slot_model[e] in
 * [0, n_models) is the id of a loaded model, model_kind[m] (FOT_NOISE_GAUSSIAN | FOT_NOISE_UNIFORM_SYM) the noise kind of
 * model m, the checkpoint's own noise_type; slot_crowd as in the shared call (its consistency check runs per crowd whatever
 * the models).  A sampling UNIT is a (crowd, model) pair, active when one of its running slots has pedestrians.  Every lock
 * step, for each model in ascending id that has an active unit: its active units in ascending crowd id
 * are the generator's scenes, a scene's window is that of the unit's lowest running slot, the noise counter's `slot` word is
 * the crowd's id, its `step` word the slots' step count, its kind model_kind[m], the dimensions and the mix type model m's.
 * A model without an active unit launches nothing that step.  The first active model samples on the loop's stream, every
 * later one on a side stream of its own, forked from and joined to the loop's stream by events -- their work arrays are
 * separate and nothing is synchronised with the host (FOT_LOOP_MODEL_STREAMS=0 in the environment of the set call keeps all
 * of them on the loop's stream: same bytes, for measurements).  The models' raw tensors [S][pred_len][rows_m][2] are gathered
 * into the step's raw tensor of the running episodes by one launch (k_loop_model_rows) and everything behind it runs per slot
 * as before: every slot's numbers are the bits of the loop that has only that slot's model loaded, and
 * fot_sgan_noise(seed, model_kind[m], ..., row_slot = crowd id, ...) fed through fot_sgan_sample_model(m) reproduces any step.
 * With n_models = 1 the call is fot_loop_set_sampler_shared with kind = model_kind[0]: the launches and bytes of before.
 * When it may be called and the refusals are fot_loop_set_sampler_shared's; further FOT_ERR_INVALID, nothing changed:
 * slot_model or model_kind NULL; n_models outside 1 .. fot_sgan_max_models(); a slot naming an id outside [0, n_models) or a
 * model that is not loaded; an unknown kind; a named model whose obs_len / pred_len differ from the replay's.  Everything is
 * allocated by the call, sized for every model's worst case; fot_loop_begin* and fot_loop_set_replay drop it.
 *
 * fot_debug_loop_sampler_shapes (tests): for model ids 0 .. cap - 1 the scenes and pedestrian rows the most recent lock step
 * handed to that model -- 0 / 0 for a model that launched nothing; FOT_ERR_INVALID without a sampler.
 * All entries are additions: no structure, capacity word of fot_abi_info or FOT_ABI_VERSION changes; a binding that needs them
 * looks the symbols up. */
int32_t fot_sgan_max_models(void);
int fot_sgan_load_model(fot_handle *h, int32_t model, const fot_sgan_desc *desc, int64_t n, const float *weights);
int fot_sgan_unload_model(fot_handle *h, int32_t model);
int fot_sgan_sample_model(fot_handle *h, int32_t model, int32_t n_scenes, const int32_t *ped_off, const void *obs, int32_t S,
                          const void *noise, int32_t flags, void *out, void *stream);
int fot_loop_set_sampler_models(fot_handle *h, int32_t S, uint64_t seed, int32_t n_models, const int32_t *model_kind,
                                int32_t n_crowds, const int32_t *slot_crowd, const int32_t *slot_model);
int fot_debug_loop_sampler_shapes(fot_handle *h, int32_t cap, int32_t *n_scenes, int32_t *n_rows);
int fot_loop_set_samples_shared(fot_handle *h, int32_t S, int32_t n_steps, int32_t first_step, const void *samples,
                                int32_t dtype, int32_t flags, int32_t n_rec_cols, const int32_t *slot_col0);

/* ---- a sample count per slot of a sweep loop -------------------------------------------------------------------------------------
 * fot_loop_set_slot_samples(h, n_slots, slot_S): slot e of a sweep loop (fot_loop_begin_sweep) uses the FIRST slot_S[e]
 * samples of what its source provides -- the sample-count ablation (5, 10, 20, 50, 100 samples of one predictor output over
 * one crowd) as slots of ONE loop, whose crowd is gathered or sampled once per lock step.  Every number of slot e -- records,
 * chosen samples, planning blocks, scores, summaries -- is the bits of the uniform loop of its configuration run on those
 * slot_S[e] samples alone: the chance budget floor(eps * slot_S[e]), best-of-N over slot_S[e] samples, the KDE bandwidth of
 * slot_S[e] samples.  The counter noise is keyed by the sample index and the generator's samples are independent of one
 * another, so the first k samples of a sampler of S are the samples of a sampler of k.
 * When: on a sweep loop, after the source is set and before the first step.  A resident loop's source is
 * fot_loop_set_samples(_shared) or fot_loop_set_sampler(_shared, _models) and 1 <= slot_S[e] <= its S.  A stepwise sweep
 * (fot_loop_step) takes the call before its first step with 1 <= slot_S[e] <= the handle's sample capacity; the source's
 * count is then every frame's dist_S, and a frame whose dist_S lies below the count of one of its episodes' slots is
 * FOT_ERR_INVALID.  fot_loop_begin*, fot_loop_set_replay and a new fot_loop_set_samples* / fot_loop_set_sampler* call drop
 * the counts with what they drop.  Lowering the handle's sample capacity is judged against the source's S, as before.
 * A step: running episode i keeps a block [S_i][P_i][T][2] of the step's tensor, the blocks packed by prefix sum and the
 * planning blocks of the representative-mode episodes behind them (fot_sweep.hpp); the gather of a recording's row and the
 * sampler move or draw no more than the largest count among the loop's slots; the ragged resample's work follows
 * sum S_i P_i; selection, planning block, plan request and score origin of an episode take its own S_i; a launch is wide
 * when one of its running episodes has more than FOT_MAX_SAMPLES samples, so a step whose running counts are all within
 * FOT_MAX_SAMPLES takes the narrow launches whatever the source's S.  Without the call, and in every step whose running
 * slots all have slot_S[e] == S, the launches and bytes are those of before.
 * fot_loop_last_best_sample and fot_loop_run_best_samples answer in [0, slot_S[e]); fot_debug_loop_block answers with the
 * episode's own count of samples; fot_loop_score_summaries reports pred_samples per slot.
 * Refused, nothing changed: FOT_ERR_INVALID -- h or slot_S NULL; n_slots not the loop's; an entry outside 1 .. S; a resident
 * loop without a source; after the first step.  FOT_ERR_UNSUPPORTED -- a loop that is not a sweep loop (fot_loop_begin and
 * fot_loop_begin_scenarios loops keep one count, and their kernels are untouched).
 * Not supported: one distribution block per crowd; the cost of a slot of more than FOT_MAX_SAMPLES samples is that of the wide
 * selection and score kernels' sequential sample walk and of k_cull's NaN scan, as in a uniform loop of that count.
 *
 * fot_debug_loop_slot_samples(h, n_slots, out) (tests): out[i] = the sample count of running episode i of the most recent
 * frame (0: it carried no distribution), -1 behind the frame's episodes; n_slots: the entries of out, at least the frame's
 * episodes.  It shows that the counts were used, not only that the numbers look right.
 * Both entries are additions: no structure, capacity word of fot_abi_info or FOT_ABI_VERSION changes; a binding looks the
 * symbols up. */
int fot_loop_set_slot_samples(fot_handle *h, int32_t n_slots, const int32_t *slot_S);
int fot_debug_loop_slot_samples(fot_handle *h, int32_t n_slots, int32_t *out);

/* ---- open-loop prediction evaluation of a whole scene (RQ1a) ------------------------------------------------------------------
 * The reference's examples/run_openloop_prediction.py (evaluate_window / evaluate_scene) in ONE stateless, synchronous call:
 * every fixed-population window of obs_len + pred_len frames of a recorded scene is observed for obs_len frames, predicted
 * (constant velocity, or S samples of a loaded Social-GAN model), resampled through process_prediction at sgan_dt = sim_dt =
 * dt and plan_horizon = pred_len dt (stride 1, E = pred_len, no prepended entry) and scored at its one origin t = obs_len - 1;
 * the windows' records are folded count-weighted.  The scene crosses the bus once and the samples never leave HBM.
 *   scene       [n_frames][n_cols][2] of scene_dtype (FOT_F32 | FOT_F64), host memory or, with FOT_OPENLOOP_SCENE_DEVICE,
 *               device memory (aligned to one point); only the points the windows name are read (absent ones may be NaN)
 *   win_frame0  [n_windows] host: first frame of each window
 *   ped_off     [n_windows + 1] host, non-decreasing from 0;  row_col [ped_off[n_windows]] host: the scene column of every
 *               row, the pedestrians of a window in the caller's order
 *   method      FOT_OPENLOOP_CV (S must be 1; the velocity from the last two float32 observations, zero when obs_len == 1),
 *               or FOT_OPENLOOP_SGAN with `model`, a slot of fot_sgan_load_model whose obs_len / pred_len are the call's
 *   noise       [S][rows][noise_dim] float32 for the whole call, host memory or (FOT_OPENLOOP_NOISE_DEVICE) device memory,
 *               rows = ped_off[n_windows] (FOT_SGAN_NOISE_PED) or n_windows (FOT_SGAN_NOISE_GLOBAL); or NULL: the library
 *               draws fot_sgan_noise's numbers of (seed, noise_kind) with the slot word win_id0 + w, step 0 and the row's
 *               index within its window -- a window's numbers depend neither on its company nor on how a scene is split
 *               over calls.  Ignored for CV and for a model with noise_dim 0
 *   max_rows    rows a chunk of whole windows may hold (0: 8192); the work arrays are sized by it and only grow
 *   records     host, n_windows fot_pred_score records, or NULL;  raw_out host [S][pred_len][rows][2] float32 or NULL: the
 *               generator's raw samples of the whole call (tests; not with CV)
 *   totals      host: sum_ade += ((ade_scene P) / P) P, likewise fde and the per-agent sums (agent_sum / P) P, traj_count
 *               += P for every window with P > 0 whose ade is not NaN; sum_nll += ((-log_lik_sum) / nll_count) nll_count,
 *               nll_count += ... for every window with FOT_PRED_NLL -- the reference's operation order, in window order;
 *               n_windows; flags: the OR of the records' flags.  ade = sum_ade / traj_count ..., nll = sum_nll / nll_count.
 * Per chunk the gather (k_openloop_rows), the noise, the generator or the constant-velocity predictor, the resampler and the
 * scorer are enqueued on one stream (NULL = the handle's) with nothing synchronised in between; the call waits once.  A
 * window's record is byte-identical whatever max_rows, the windows beside it, the placement or the element type of a scene
 * of the same values.  Non-finite coordinates raise FOT_PRED_NONFINITE as in fot_prediction_scores.
 * Refusals, a refused call writes nothing.  FOT_ERR_INVALID: a NULL argument that is needed; negative n_frames / n_cols /
 * n_windows; obs_len, pred_len or S < 1; dt <= 0; offsets not starting at 0 or decreasing; a column outside the scene; a
 * window starting before frame 0 or reaching past n_frames; max_rows < 0 or below the largest window; an unknown method,
 * flag, dtype or noise kind (FOT_NOISE_RAW included); S != 1 with CV; no model loaded in the slot, or its obs_len / pred_len
 * differ; a negative win_id0; a misaligned device scene.  FOT_ERR_UNSUPPORTED: S > FOT_MAX_SAMPLES, pred_len >
 * FOT_MAX_PRED_LEN, obs_len > FOT_SGAN_MAX_OBS_LEN, a window of more than FOT_SGAN_MAX_PEDS rows.
 * An addition: no structure, capacity word of fot_abi_info or FOT_ABI_VERSION changes; a binding looks the symbol up. */
#define FOT_OPENLOOP_CV 0
#define FOT_OPENLOOP_SGAN 1
#define FOT_OPENLOOP_SCENE_DEVICE 1
#define FOT_OPENLOOP_NOISE_DEVICE 2
typedef struct fot_openloop_params {
    int32_t n_frames, n_cols, n_windows;
    int32_t scene_dtype;            /* FOT_F32 | FOT_F64 */
    int32_t obs_len, pred_len;
    int32_t method;                 /* FOT_OPENLOOP_CV | FOT_OPENLOOP_SGAN */
    int32_t model;                  /* slot of fot_sgan_load_model (SGAN) */
    int32_t S;
    int32_t noise_kind;             /* FOT_NOISE_GAUSSIAN | FOT_NOISE_UNIFORM | FOT_NOISE_UNIFORM_SYM (noise == NULL) */
    int32_t win_id0;                /* the noise counter's slot word of window 0 */
    int32_t max_rows;
    int32_t flags;                  /* FOT_OPENLOOP_SCENE_DEVICE | FOT_OPENLOOP_NOISE_DEVICE */
    int32_t _pad;
    double dt;
    uint64_t seed;
} fot_openloop_params;
typedef struct fot_openloop_totals {
    double sum_ade, sum_fde, sum_ade_agent, sum_fde_agent, sum_nll;
    int64_t traj_count, nll_count;
    int32_t n_windows, flags;
} fot_openloop_totals;
int fot_openloop_eval(fot_handle *h, const fot_openloop_params *p, const void *scene, const int32_t *win_frame0,
                      const int32_t *ped_off, const int32_t *row_col, const void *noise, fot_pred_score *records,
                      void *raw_out, fot_openloop_totals *totals, void *stream);

/* ---- footprint re-verification of episodes (A-4): centre, circle cover, exact rectangle -----------------------------------------
 * The reference's examples/recheck_footprint.py (recheck, reconstruct_yaw) and observational_footprint_metrics of
 * examples/run_footprint_benchmark.py.  Every step of a trajectory -- the ego pose (x, y, yaw) and that step's pedestrians
 * -- is measured against three geometries that do not depend on what the planner used:
 *   legacy  the centre distance                  min_p sqrt((px - x)^2 + (py - y)^2)
 *   multi   the n_circles cover of the rectangle  the same distance to the centres (x + off_k cos yaw, y + off_k sin yaw),
 *           off_k = -L/2 + seg/2 + seg k, seg = L / n_circles, radius hypot(seg/2, W/2) (EgoFootprint.multi_circle)
 *   rect    the exact oriented L x W rectangle    min_p hypot(max(|lx| - L/2, 0), max(|ly| - W/2, 0)), (lx, ly) the
 *           pedestrian in the vehicle frame
 * A step without pedestrians measures +inf three times.  A trajectory's record holds the minima over its steps and the
 * steps strictly below each threshold: legacy < legacy_radius (the caller adds ego_radius + ped_radius), multi < radius +
 * ped_radius, rect < ped_radius; clearance = minimum - threshold; all minima and clearances +inf without any pedestrian.
 * One record serves both reference forms, which differ in key names only.  float64 throughout, NumPy's operation order
 * (csrc/fot_footprint_obs.hpp).  Non-finite coordinates: unspecified.
 *
 * fot_footprint_recheck: n_traj ragged trajectories in ONE synchronous call (one wait).
 *   step_off [n_traj + 1] host, from 0: trajectory t owns steps step_off[t] .. step_off[t + 1] - 1 of
 *   xy [steps][2], yaw [steps] host; yaw == NULL: the heading is reconstructed on the device as reconstruct_yaw does --
 *            np.gradient of x and y (one-sided at both ends), a step moves when hypot(dx, dy) > 1e-4, its heading is
 *            atan2(dy, dx); a standing step holds the last moving heading, the steps in front of the first moving one
 *            take that first heading, a trajectory that never moves is all zeros
 *   ped_off [steps + 1] host, non-decreasing from 0;  ped_xy [ped_off[steps]][2] host: every step's pedestrians
 *   series   NULL, or [steps] records of the steps;  yaw_out  NULL, or [steps]: the heading used
 *   out      [n_traj] records
 * A trajectory's record and series are byte-identical whatever trajectories share the call.
 * Refusals (FOT_ERR_INVALID, a refused call changes nothing): geom / out / a table NULL; n_traj < 0; offsets that do not
 * start at 0 or that decrease; a trajectory of 0 steps, or of 1 step with yaw == NULL (the gradient needs two);
 * vehicle_length or vehicle_width not positive, a negative radius, n_circles outside 1 .. FOT_MAX_CIRCLES.
 *
 * fot_loop_footprint_enable: accepted after fot_loop_begin* and before the loop's first step; geom == NULL switches it off
 * again.  While on, every lock step of fot_loop_step and fot_loop_run launches the per-step kernel right behind the
 * k_safety launch of the NEW ego states, on the same poses and the same frame rows (the reference pairs the new ego state
 * with that step's pedestrians, integrated_simulator.py:707-727); the records land in pinned memory and are folded per
 * slot at the wait the step already has.  A loop that never enables it launches and allocates nothing for it; the
 * five-call form (fot_loop_plan / fot_loop_observe_*) names no slots and accumulates nothing.  fot_loop_begin* drops the
 * accumulators and switches it off.  fot_loop_footprint_obs copies the per-slot records (steps: lock steps folded so far);
 * it may be called between two fot_loop_run calls and changes nothing.
 * Refusals (FOT_ERR_INVALID, nothing changed): no loop begun; enabling after the first step; a bad geometry;
 * fot_loop_footprint_obs: not enabled, n_slots differing from the loop's, out NULL.
 * Additions: no structure, capacity word of fot_abi_info or FOT_ABI_VERSION changes; a binding looks the symbols up. */
typedef struct fot_footprint_geom {
    double vehicle_length, vehicle_width, ped_radius, legacy_radius;
    int32_t n_circles;              /* 1 .. FOT_MAX_CIRCLES */
    int32_t _pad;
} fot_footprint_geom;
typedef struct fot_footprint_step {
    double legacy, multi, rect;
} fot_footprint_step;
typedef struct fot_footprint_obs {
    double legacy_min_dist;
    double multi_min_dist, multi_clearance;
    double rect_min_surface_dist, rect_clearance;
    int32_t legacy_collision_steps, multi_violation_steps, rect_violation_steps;
    int32_t steps, steps_with_peds, _pad;
} fot_footprint_obs;
int fot_footprint_recheck(fot_handle *h, const fot_footprint_geom *geom, int32_t n_traj, const int32_t *step_off,
                          const double *xy, const double *yaw, const int32_t *ped_off, const double *ped_xy,
                          fot_footprint_step *series, double *yaw_out, fot_footprint_obs *out);
int fot_loop_footprint_enable(fot_handle *h, const fot_footprint_geom *geom);
int fot_loop_footprint_obs(fot_handle *h, int32_t n_slots, fot_footprint_obs *out);

/* ---- fidelity statistics of vehicle-pedestrian encounters (RQ2): separation, avoidance onset, roll-out error ---------------------
 * The reference's min_separation_series and avoidance_onset_distance (src/core/metrics.py) and the measuring half of
 * fidelity_report / objective_rollout_ade (src/simulation/calibration_harness.py).  An encounter is T steps of an ego
 * position and of a fixed population of N pedestrians, [T][N][2]; the caller brings the positions from wherever they were
 * recorded or simulated.  float64 throughout, NumPy's operation order (csrc/fot_fidelity.hpp):
 *   distance    sqrt(dx dx + dy dy), each product and the sum rounded apart (np.linalg.norm(axis=2))
 *   gradient    np.gradient(f, dt, axis=0): (f[t+1] - f[t-1]) / (2 dt) inside, (f[1] - f[0]) / dt and (f[T-1] - f[T-2]) / dt
 *               at the ends.  The velocity is ped_vel, or the gradient of the positions; the acceleration is always the
 *               gradient of the velocity
 *   onset       of a pedestrian: the first step t, ascending, with !(dist < 1e-9) && !(dist > max_distance) and
 *               away > accel_threshold, away = acc_x (rel_x / dist) + acc_y (rel_y / dist), rel = pedestrian - ego;
 *               onset_dist is that step's distance, the bits of its separation.  A NaN distance is not skipped and a NaN
 *               away is never an onset; dist == max_distance counts, away == accel_threshold does not; T < 2: no onset
 *   series      per step the minimum over the pedestrians as np.min forms it (a NaN stays NaN); +inf with N == 0
 *   error       against truth_xy: err[t][j] = |ped_xy - truth_xy|, step 0 excluded; with interaction_distance not NaN
 *               only the pedestrians whose truth-side distance to the ego has min_t <= interaction_distance.  err_sum adds
 *               each kept pedestrian's steps in ascending order, then the pedestrians in ascending order: one fixed order,
 *               no floating-point atomics
 * n_enc ragged encounters in ONE synchronous call: everything is enqueued on the handle's stream and waited for once.  All
 * pointers are host memory.  An encounter's outputs are byte-identical whatever encounters share the call and wherever it
 * stands in it.  No capacity on T, N or n_enc beyond the int32 offsets.
 * Refusals (FOT_ERR_INVALID, a refused call changes nothing): p, step_off, n_ped, dt, ego_xy, ped_xy or out NULL;
 * n_enc < 0; offsets that do not start at 0 or that decrease; an encounter of 0 steps; n_ped[e] < 0; a dt that is not
 * finite and positive; max_distance or accel_threshold NaN.  n_enc == 0 succeeds and writes nothing.
 * An addition: no structure, capacity word of fot_abi_info or FOT_ABI_VERSION changes; a binding looks the symbol up. */
typedef struct fot_fidelity_params {
    double accel_threshold, max_distance;   /* reference defaults 0.3, 5.0 */
    double interaction_distance;            /* NaN: keep every pedestrian in the error */
} fot_fidelity_params;
typedef struct fot_fidelity_enc {
    double  closest;                        /* min of the series; +inf if N == 0; NaN propagates */
    double  err_sum;                        /* 0 without truth */
    int64_t err_count;                      /* (T - 1) * kept pedestrians; 0 without truth */
    int32_t n_onset, closest_step;          /* first step holding `closest`; -1 if N == 0 or closest is NaN */
} fot_fidelity_enc;
int fot_fidelity_eval(fot_handle *h, const fot_fidelity_params *p, int32_t n_enc,
                      const int32_t *step_off,  /* [n_enc + 1] from 0 */
                      const int32_t *n_ped,     /* [n_enc] */
                      const double  *dt,        /* [n_enc] */
                      const double  *ego_xy,    /* [steps][2] */
                      const double  *ped_xy,    /* encounter e: [T_e][N_e][2], encounters back to back */
                      const double  *ped_vel,   /* same shape, or NULL: finite differences for every encounter */
                      const double  *truth_xy,  /* same shape, or NULL: no roll-out error */
                      double *sep_series,       /* NULL or [steps] */
                      double *onset_dist,       /* NULL or [sum N]: NaN = no onset */
                      int32_t *onset_step,      /* NULL or [sum N]: -1 = no onset */
                      fot_fidelity_enc *out);   /* [n_enc] */

/* ---- vehicle-pedestrian encounters cut out of a recorded clip (RQ2): spans, populations, closest approach, boundary conditions ---
 * The reference's _ped_velocities and extract_encounters (src/datasets/vci_encounter.py) over every vehicle of a clip
 * (_split_clip_per_vehicle), and _cruise_speeds, cruise_upper_quantile, cruise_freewalk, _floor and _far_goals
 * (src/simulation/calibration_harness.py).  The clip is a pedestrian scene ped_xy [T][A][2] (NaN where a pedestrian is
 * absent), optionally its recorded velocities ped_vel, and K vehicles ALREADY aligned onto the scene's grid: ego_xy
 * [K][T][2], ego_psi and ego_vel [K][T], NaN outside a vehicle's support (the alignment is sequential host work).  The
 * scene crosses the bus once per call, or not at all: with FOT_ENC_SCENE_DEVICE ped_xy and ped_vel are device memory,
 * aligned to one point (16 bytes), never written, and complete before the call (it is read on the handle's stream).  The
 * ego channels and every output are host memory.  float64
 * throughout, NumPy's operation order (csrc/fot_encounter.hpp):
 *   velocity    ped_vel, or with ped_vel NULL the forward difference over the WHOLE grid: vel[t] = (pos[t+1] - pos[t]) / dt,
 *               vel[T-1] = vel[T-2], all NaN with T < 2 -- a pedestrian's last present frame has a NaN velocity unless it is
 *               the grid's last frame
 *   spans       the maximal runs of frames at which x, y, psi and vel of vehicle k are all finite, by vehicle ascending, then
 *               start ascending; found on the host.  One record each.  A run shorter than min_len: FOT_ENC_SHORT
 *   population  pedestrian a is present when no position and no velocity component over the span is NaN (isnan: an infinity
 *               is not absence, and is otherwise unspecified).  None present: FOT_ENC_NO_PEDS.  The kept columns ascend
 *   closest     min_separation = min over [L][N] of sqrt(dx dx + dy dy) (fot_fidelity_eval's distance), with its first step
 *               and (compacted) column in row-major order.  min_separation > min_sep_threshold: FOT_ENC_FAR (equality keeps
 *               the span); everything else: FOT_ENC_KEPT
 *   rows        the kept spans' pedestrians back to back in span order: span s owns the rows row_base .. row_base + n_ped - 1
 *               of cols (the scene's column), cruise, goals, onset_dist and onset_step; FAR spans report n_ped but own no rows
 *   real        with FOT_ENC_MEASURE_REAL every kept span is gathered from the resident scene into fot_fidelity_eval's packed
 *               layout and measured there from its positions (no velocity, no truth; accel_threshold, max_distance):
 *               `real` is that call's record, real.closest the bits of min_separation; sep_series holds the kept spans' steps
 *               back to back
 *   cruise      per kept pedestrian, speeds[t] = sqrt(vx vx + vy vy) of the span's velocities.  FOT_ENC_CRUISE_MEDIAN: the
 *               middle order statistic, (s[n/2-1] + s[n/2]) / 2 for even n.  _QUANTILE: np.quantile's linear method at
 *               cruise_q: v = q (n-1), lo = floor(v), g = v - lo, d = s[lo+1] - s[lo]; s[lo] if d == 0, s[lo] + d g if g < 0.5,
 *               else s[lo+1] - d (1 - g).  _FREEWALK: that quantile over the steps whose speed is finite and whose distance to
 *               the ego is > free_distance; without such a step the all-step median.  Every mode ends in the floor: a value
 *               that is not finite or not > 1e-3 becomes 1e-3.  Order statistics by counting ranks, ties by step
 *   goals       first position + heading * goal_distance; heading = last - first position, or, if its norm < 1e-3, the first
 *               velocity if that norm > 1e-3, else (1, 0); divided by the chosen vector's own norm
 * ONE stateless synchronous call per clip with at most two waits: one for the spans' populations and closest approaches
 * (which size the rows), one for everything else.  A span's record and rows are byte-identical whatever vehicles share the
 * call, whether the scene is host or device memory, and whether ped_vel is given or equals the fallback's values.
 * Refusals, nothing written: FOT_ERR_INVALID for p, n_spans, n_rows, spans or cols NULL; ped_xy or an ego channel NULL where
 * T, A and K are positive; cruise or goals NULL with a cruise mode; negative T, A, K, max_spans or max_rows; dt not finite
 * and positive; min_len < 1; a NaN threshold; cruise_q outside [0, 1] (quantile and freewalk modes); an unknown mode or
 * flag; a misaligned device scene.  FOT_ERR_UNSUPPORTED when the spans exceed max_spans, the rows max_rows or, with
 * sep_series, the kept spans' steps max_steps, the need named in fot_last_error.  T, A or K of 0 succeed with zero spans.
 * An addition: no structure, capacity word of fot_abi_info or FOT_ABI_VERSION changes; a binding looks the symbol up. */
#define FOT_ENC_SHORT 0
#define FOT_ENC_NO_PEDS 1
#define FOT_ENC_FAR 2
#define FOT_ENC_KEPT 3
#define FOT_ENC_CRUISE_NONE 0
#define FOT_ENC_CRUISE_MEDIAN 1
#define FOT_ENC_CRUISE_QUANTILE 2
#define FOT_ENC_CRUISE_FREEWALK 3
#define FOT_ENC_SCENE_DEVICE 1
#define FOT_ENC_MEASURE_REAL 2
typedef struct fot_encounter_params {
    double  min_sep_threshold;              /* reference default 8.0 */
    double  dt;
    double  accel_threshold, max_distance;  /* the onset's, for `real`: 0.3, 5.0 */
    double  cruise_q;                       /* 0.85 (cruise_upper_quantile), 0.5 (cruise_freewalk) */
    double  free_distance, goal_distance;   /* 8.0, 50.0 */
    int32_t min_len;                        /* 5 */
    int32_t cruise_mode;                    /* FOT_ENC_CRUISE_* */
    int32_t flags;                          /* FOT_ENC_SCENE_DEVICE | FOT_ENC_MEASURE_REAL */
    int32_t _pad;
} fot_encounter_params;
typedef struct fot_encounter_span {
    double  min_separation;                 /* NaN for FOT_ENC_SHORT, +inf for FOT_ENC_NO_PEDS */
    fot_fidelity_enc real;                  /* KEPT with FOT_ENC_MEASURE_REAL; else closest NaN, closest_step -1, zeros */
    int64_t row_base;                       /* KEPT: its first row; else -1 */
    int32_t status, vehicle;                /* FOT_ENC_*; k */
    int32_t frame0, frame1;                 /* the frames frame0 .. frame1 - 1 */
    int32_t n_ped;                          /* 0 for SHORT */
    int32_t min_step, min_col;              /* first (step, compacted column) holding min_separation; -1 without one */
    int32_t _pad;
} fot_encounter_span;
int fot_encounters_extract(fot_handle *h, const fot_encounter_params *p, int32_t T, int32_t A, int32_t K,
                           const double *ped_xy,   /* [T][A][2] */
                           const double *ped_vel,  /* [T][A][2], or NULL: the forward-difference fallback */
                           const double *ego_xy,   /* [K][T][2] */
                           const double *ego_psi,  /* [K][T] */
                           const double *ego_vel,  /* [K][T] */
                           int32_t max_spans, int64_t max_rows,
                           int32_t *n_spans, int64_t *n_rows,
                           fot_encounter_span *spans,  /* [max_spans] */
                           int32_t *cols,          /* [max_rows] */
                           double *cruise,         /* [max_rows]; NULL allowed with FOT_ENC_CRUISE_NONE */
                           double *goals,          /* [max_rows][2]; likewise */
                           double *onset_dist,     /* NULL or [max_rows]: NaN = no onset (FOT_ENC_MEASURE_REAL) */
                           int32_t *onset_step,    /* NULL or [max_rows]: -1 = no onset */
                           double *sep_series,     /* NULL or [sum of the kept spans' lengths] */
                           int64_t max_steps);     /* capacity of sep_series (ignored when it is NULL) */

/* Host utility (no GPU): the first kmax samples of the 15 path arrays of records[index[i]], i < n, as one dense block
 * out[15][n][kmax] in fot_result array order (t .. c) -- what a history keeps of a step's records. */
int fot_gather_paths(const fot_result *records, int32_t n, const int32_t *index, int32_t kmax, double *out);

/* ---- compact wire form of the records, for the all-gather of selected paths across GPUs ------------
 * fot_result is the host view (float64, FOT_MAX_NT slots per array: 15 536 bytes).  On the wire a record is
 *   fot_wire_header (176 bytes) | float path[15][n_total] (fot_result array order t .. c) | padding to 256 bytes
 * e.g. 3 328 bytes at n_total = 51.  The header keeps cost, the state updates and the Frenet start state in float64;
 * the path samples travel as float32, s / x / y as OFFSETS from the record's own start (frenet0[0], ref0[1], ref0[2]):
 * 2^-24 of the path's length (4e-6 m at 70 m) at any world coordinate, inside the 1e-5 the north star allows; the
 * other arrays are small numbers (d, speeds, curvature).  Samples past n_keep are zero.
 * n_total = round(max_t / dt) + 1 of the planner (fot_wire_n_total).  Pack / unpack on the host are pure format
 * conversions (no GPU); fot_pack_records_device converts device-resident records on `stream`. */
typedef struct fot_wire_header {
    int32_t status, best_index, n_cand, n_keep;
    double cost;
    int32_t stats[8];
    int32_t stats_valid, n_total;
    double new_last_kappa, new_prev_s;
    double frenet0[6], ref0[6];
} fot_wire_header;
int32_t fot_wire_n_total(const fot_handle *h);
int32_t fot_wire_record_bytes(int32_t n_total);
int fot_pack_records_device(fot_handle *h, int32_t n, const fot_result *records_dev, void *wire_dev, void *stream);
int fot_pack_records_host(int32_t n_total, int32_t n, const fot_result *records, void *wire);
int fot_unpack_records(int32_t n_total, int32_t n, const void *wire, fot_result *records);

/* ---- measurement (no reference counterpart: the reference times plan() with perf_counter,
 *      integrated_simulator.py:575-585) ----
 * With profiling on, every kernel launch of a plan call is bracketed by HIP events on the
 * stream it is launched on.  fot_profile_read waits for the recorded work, then returns, per
 * kernel, the number of launches and the summed device time in ms since the last reset. */
#define FOT_PROFILE_KERNELS 3
int fot_profile_enable(fot_handle *h, int on);
/* launches / total_ms: arrays of `cap` entries (entries past cap are not written); returns FOT_PROFILE_KERNELS of the
 * library, or a negative error */
int fot_profile_read(fot_handle *h, int reset, int32_t cap, int32_t *launches, double *total_ms);
const char *fot_profile_kernel_name(int index);

#ifdef __cplusplus
}
#endif
#endif /* FOT_H */
