// fot_openloop.hpp -- what the open-loop prediction evaluation of a scene (fot_openloop_eval; the reference's
// examples/run_openloop_prediction.py: evaluate_window / evaluate_scene) shares between the kernel that gathers a chunk's
// rows (k_openloop_rows), the host (the table checks, the chunks, the fold) and tests/emu/fot_openloop_emu.cpp.  Plain C++.
//
// A scene is a tensor [n_frames][n_cols][2]; a window is obs_len + pred_len consecutive frames from win_frame0[w] on and
// the columns row_col[ped_off[w] .. ped_off[w + 1]) -- the pedestrians present throughout, in the caller's order.  Row r
// of window w observes frames f0 .. f0 + obs_len - 1 (rounded to float32, as PedestrianObserver.get_observation hands
// them over: observer.py:134), is anchored at that float32 last observation (trajectory_predictor.py:184) and is scored
// against frames f0 + obs_len - 1 + j, j = 1 .. pred_len, in float64 (the window itself: replay_source.py).
//
// The fold follows evaluate_scene (run_openloop_prediction.py:111-151) operation by operation.  Per window,
// calculate_aggregate_metrics returns m["ade"] = (0.0 + ade_scene P) / P, m["ade_per_agent"] = (0.0 + ade_agent_sum) / P
// and m["nll"] = -(0.0 + log_lik_sum) / nll_count (metrics.py:96-113, 171-176); the scene adds m[...] * count, NOT the raw
// sums: ((ade_scene P) / P) P differs from ade_scene P in the last bit for some (value, P).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FOT_OL_HD __host__ __device__ inline
#else
#define FOT_OL_HD inline
#endif

namespace fot {

constexpr int OL_TILE_ROWS = 64;                 // rows of a chunk one workgroup of k_openloop_rows gathers
constexpr int OL_DEFAULT_MAX_ROWS = 8192;        // fot_openloop_params.max_rows == 0
constexpr int OL_MAX_PRED_LEN = 32;              // FOT_MAX_PRED_LEN
constexpr int OL_MAX_OBS_LEN = 32;               // FOT_SGAN_MAX_OBS_LEN
constexpr int OL_MAX_PEDS = 256;                 // FOT_SGAN_MAX_PEDS
constexpr int OL_MAX_SAMPLES = 64;               // FOT_MAX_SAMPLES
constexpr int OL_FLAG_NLL = 1;                   // fot_pred_score.flags: FOT_PRED_NLL

// element (2-vector) of the scene that row (frame0, col) reads at frame offset t
FOT_OL_HD int64_t ol_scene_point(int32_t frame0, int t, int32_t n_cols, int32_t col)
{
    return ((int64_t)frame0 + t) * (int64_t)n_cols + col;
}

// the observer's float32 sample of a coordinate, and the anchor: that sample widened again
FOT_OL_HD float ol_observe(double v) { return (float)v; }
FOT_OL_HD double ol_anchor(double v) { return (double)(float)v; }

// ---- the table checks: 0, or OL_BAD_* with *why naming the rule (static strings) ------------------------------------------
constexpr int OL_OK = 0;
constexpr int OL_BAD_INVALID = 1;                // FOT_ERR_INVALID
constexpr int OL_BAD_UNSUPPORTED = 2;            // FOT_ERR_UNSUPPORTED

// the lengths alone (no table is read)
inline int ol_check_lengths(int64_t n_frames, int64_t n_cols, int64_t n_windows, int obs_len, int pred_len, int S, bool cv,
                            const char **why)
{
    if (n_frames < 0 || n_cols < 0 || n_windows < 0) { *why = "n_frames / n_cols / n_windows is negative"; return OL_BAD_INVALID; }
    if (obs_len < 1 || pred_len < 1) { *why = "obs_len and pred_len must be positive"; return OL_BAD_INVALID; }
    if (S < 1) { *why = "S < 1"; return OL_BAD_INVALID; }
    if (cv && S != 1) { *why = "the constant-velocity predictor gives one sample: S must be 1"; return OL_BAD_INVALID; }
    if (S > OL_MAX_SAMPLES) { *why = "S > FOT_MAX_SAMPLES"; return OL_BAD_UNSUPPORTED; }
    if (pred_len > OL_MAX_PRED_LEN) { *why = "pred_len > FOT_MAX_PRED_LEN"; return OL_BAD_UNSUPPORTED; }
    if (obs_len > OL_MAX_OBS_LEN) { *why = "obs_len > FOT_SGAN_MAX_OBS_LEN"; return OL_BAD_UNSUPPORTED; }
    return OL_OK;
}

// the window table; *widest: the largest window's rows.  Every INVALID rule is looked at before the UNSUPPORTED one.
inline int ol_check_table(int64_t n_frames, int64_t n_cols, int64_t n_windows, int obs_len, int pred_len,
                          const int32_t *win_frame0, const int32_t *ped_off, const int32_t *row_col, int *widest,
                          const char **why)
{
    *widest = 0;
    if (!ped_off) { *why = "ped_off is NULL (one offset even for no window)"; return OL_BAD_INVALID; }
    if (ped_off[0] != 0) { *why = "ped_off must start at 0 and be non-decreasing"; return OL_BAD_INVALID; }
    if (n_windows > 0 && !win_frame0) { *why = "win_frame0 is NULL"; return OL_BAD_INVALID; }
    const int64_t seq = (int64_t)obs_len + pred_len;
    int w_max = 0;
    for (int64_t w = 0; w < n_windows; ++w) {
        if (ped_off[w + 1] < ped_off[w]) { *why = "ped_off must start at 0 and be non-decreasing"; return OL_BAD_INVALID; }
        if (win_frame0[w] < 0) { *why = "a window starts before frame 0"; return OL_BAD_INVALID; }
        if ((int64_t)win_frame0[w] + seq > n_frames) { *why = "a window reaches past n_frames"; return OL_BAD_INVALID; }
        const int P = ped_off[w + 1] - ped_off[w];
        w_max = P > w_max ? P : w_max;
    }
    const int64_t rows = ped_off[n_windows];
    if (rows > 0 && !row_col) { *why = "row_col is NULL"; return OL_BAD_INVALID; }
    for (int64_t r = 0; r < rows; ++r)
        if (row_col[r] < 0 || row_col[r] >= n_cols) { *why = "a row names a column outside 0 .. n_cols - 1"; return OL_BAD_INVALID; }
    *widest = w_max;
    if (w_max > OL_MAX_PEDS) { *why = "a window of more than FOT_SGAN_MAX_PEDS rows"; return OL_BAD_UNSUPPORTED; }
    return OL_OK;
}

// A chunk is a run of whole windows whose rows fit max_rows (>= the widest window): the first window past w0's chunk.
inline int64_t ol_chunk_end(const int32_t *ped_off, int64_t n_windows, int64_t w0, int max_rows)
{
    int64_t w1 = w0 + 1;
    while (w1 < n_windows && (int64_t)ped_off[w1 + 1] - ped_off[w0] <= max_rows) ++w1;
    return w1 < n_windows ? w1 : n_windows;
}

// ---- the fold ----------------------------------------------------------------------------------------------------------------
struct OlTotals {                                // fot_openloop_totals (include/fot.h)
    double sum_ade, sum_fde, sum_ade_agent, sum_fde_agent, sum_nll;
    int64_t traj_count, nll_count;
    int32_t n_windows, flags;
};

inline OlTotals ol_totals_zero()
{
    OlTotals t;
    t.sum_ade = t.sum_fde = t.sum_ade_agent = t.sum_fde_agent = t.sum_nll = 0.0;
    t.traj_count = t.nll_count = 0;
    t.n_windows = 0; t.flags = 0;
    return t;
}

// One window's record into the scene's totals, in window order (evaluate_scene's loop body).  Every product and quotient
// is a statement of its own: none may be contracted with the addition behind it.
inline void ol_fold(OlTotals &t, double ade_scene, double fde_scene, double ade_agent_sum, double fde_agent_sum,
                    double log_lik_sum, int32_t n_peds, int32_t nll_count, int32_t flags)
{
    t.n_windows += 1;
    t.flags |= flags;
    if (n_peds > 0) {
        const double P = (double)n_peds;
        const double tot_a = ade_scene * P, tot_f = fde_scene * P;                 // total_ade += min * n_peds
        const double m_a = tot_a / P, m_f = tot_f / P;                             // m["ade"], m["fde"]
        const double m_aa = ade_agent_sum / P, m_fa = fde_agent_sum / P;           // m["ade_per_agent"], ...
        if (!(m_a != m_a)) {                                                       // `not np.isnan(m["ade"])`
            const double c_a = m_a * P, c_f = m_f * P, c_aa = m_aa * P, c_fa = m_fa * P;
            t.sum_ade += c_a; t.sum_fde += c_f; t.sum_ade_agent += c_aa; t.sum_fde_agent += c_fa;
            t.traj_count += n_peds;
        }
    }
    if ((flags & OL_FLAG_NLL) && nll_count > 0) {
        const double n = (double)nll_count;
        const double neg = -log_lik_sum;
        const double m_n = neg / n;                                                // m["nll"]
        if (!(m_n != m_n)) {
            const double c_n = m_n * n;
            t.sum_nll += c_n;
            t.nll_count += nll_count;
        }
    }
}

}  // namespace fot
