// fot_summary.hpp -- the arithmetic of the per-episode prediction-error summary (fot_loop_summary_enable /
// fot_loop_summaries): what a row of the ring contributes to the totals, when, and how a summary is read off them.
// Plain C++ shared by the kernels (k_loop_pred_error, k_loop_summary), the host and tests/emu/fot_summary_emu.cpp, which
// holds the ring against a direct evaluation of the definition (metrics.py:31-114, 225-269) on the CPU.
//
// Row i of an episode is c_i[k] = sum_p d_i[p][k], k < n_dense: the summed distance of the step-i prediction's dense
// sample k to the pedestrians' positions k + 1 steps later.  The ring keeps the last n_dense rows, row i in place
// i % n_dense with the pedestrian count beside it (0: the step had no prediction).  When step i overwrites the row of step
// i - n_dense the episode has i + 1 steps, so that row's horizon is complete (E = n_dense, and i - n_dense + stride pred_len
// < i + 1 whenever the standard metric applies at all): it is folded into the totals for good.  A summary at L steps folds
// the remaining rows, oldest first, with E = min(n_dense, L - (i + 1)) into a copy.  Rows are always folded in step order,
// by one thread: the totals are the sums of the definition in the definition's order.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FOT_SUM_HD __host__ __device__ inline
#else
#define FOT_SUM_HD inline
#endif

namespace fot {

struct SummaryTotals {
    double plan_ade, plan_fde;               // sums over origins of sum_p mean_k d, sum_p d[E - 1]
    double std_ade, std_fde;                 // the same at the predictor's cadence, complete horizons only
    int64_t plan_count, std_count;           // pedestrians of the counted origins
};

// What the prediction-error kernels need to know of the loop.
struct SummaryShape {
    int32_t n_dense;                         // dense samples of a prediction = rows of a slot's ring
    int32_t stride, pred_len;                // round(sgan_dt / sim_dt); predictor steps
    int32_t std_ok;                          // n_dense > stride * pred_len - 1: the standard metric applies
};

// round(sgan_dt / dt) if the ratio is an integer (np.isclose: |ratio - r| <= 1e-8 + 1e-5 r) and positive, else 0
// (_steps_for_interval, metrics.py:22-28; Python's round() is half-to-even, as nearbyint in the default mode)
inline int32_t summary_stride(double sgan_dt, double dt)
{
    const double ratio = sgan_dt / dt;
    const double r = std::nearbyint(ratio);
    if (!(r >= 1.0) || !(r < 1e9)) return 0;
    if (!(std::fabs(ratio - r) <= 1e-8 + 1e-5 * std::fabs(r))) return 0;
    return (int32_t)r;
}

FOT_SUM_HD SummaryShape summary_shape(int n_dense, int stride, int pred_len)
{
    SummaryShape s;
    s.n_dense = n_dense; s.stride = stride; s.pred_len = pred_len;
    s.std_ok = n_dense > stride * pred_len - 1 ? 1 : 0;
    return s;
}

// What the row of origin i (P pedestrians; P <= 0: no prediction) contributes as seen from an episode of L steps.
struct SummaryTerms {
    double plan_ade, plan_fde, std_ade, std_fde;
    int32_t plan_P, std_P;                   // 0: the origin does not count
};

FOT_SUM_HD SummaryTerms summary_row_terms(const SummaryShape &S, const double *row, int P, int i, int L)
{
    SummaryTerms t;
    t.plan_ade = t.plan_fde = t.std_ade = t.std_fde = 0.0;
    t.plan_P = t.std_P = 0;
    if (P <= 0) return t;
    const int left = L - (i + 1);
    const int E = left < S.n_dense ? left : S.n_dense;
    if (E > 0) {
        double s = 0.0;
        for (int k = 0; k < E; ++k) s += row[k];
        t.plan_ade = s / (double)E;
        t.plan_fde = row[E - 1];
        t.plan_P = P;
    }
    if (S.std_ok && i + S.stride * S.pred_len < L) {
        double s = 0.0;
        for (int j = 1; j <= S.pred_len; ++j) s += row[S.stride * j - 1];
        t.std_ade = s / (double)S.pred_len;
        t.std_fde = row[S.stride * S.pred_len - 1];
        t.std_P = P;
    }
    return t;
}

FOT_SUM_HD void summary_add_terms(SummaryTotals &T, const SummaryTerms &t)
{
    if (t.plan_P > 0) { T.plan_ade += t.plan_ade; T.plan_fde += t.plan_fde; T.plan_count += t.plan_P; }
    if (t.std_P > 0) { T.std_ade += t.std_ade; T.std_fde += t.std_fde; T.std_count += t.std_P; }
}

FOT_SUM_HD void summary_fold_row(SummaryTotals &T, const SummaryShape &S, const double *row, int P, int i, int L)
{
    summary_add_terms(T, summary_row_terms(S, row, P, i, L));
}

// The rows still in the ring of an episode of L steps, oldest first, folded into T (a copy of the running totals).
// ring: [n_dense][n_dense] rows, ring_P: [n_dense] pedestrian counts.
FOT_SUM_HD void summary_fold_tail(SummaryTotals &T, const SummaryShape &S, const double *ring, const int32_t *ring_P, int L)
{
    const int first = L > S.n_dense ? L - S.n_dense : 0;
    for (int i = first; i < L; ++i) {
        const int r = i % S.n_dense;
        summary_fold_row(T, S, ring + (int64_t)r * S.n_dense, ring_P[r], i, L);
    }
}

// the prediction-error keys of fot_loop_summary, in this order: ade, fde, planning_ade, planning_fde (NaN without a
// counted origin); the counts are T.std_count / T.plan_count
FOT_SUM_HD void summary_means(const SummaryTotals &T, double out[4])
{
    const double nan = __builtin_nan("");
    out[0] = T.std_count > 0 ? T.std_ade / (double)T.std_count : nan;
    out[1] = T.std_count > 0 ? T.std_fde / (double)T.std_count : nan;
    out[2] = T.plan_count > 0 ? T.plan_ade / (double)T.plan_count : nan;
    out[3] = T.plan_count > 0 ? T.plan_fde / (double)T.plan_count : nan;
}

// Step i of an episode writes its row over the one in place i % n_dense; before that the old row (origin i - n_dense) is
// folded as complete.  Host-side form of what k_loop_pred_error does, for the emulation.
inline void summary_push_row(SummaryTotals &T, const SummaryShape &S, double *ring, int32_t *ring_P, int i,
                             const double *row, int P)
{
    const int r = i % S.n_dense;
    double *dst = ring + (int64_t)r * S.n_dense;
    if (i >= S.n_dense) summary_fold_row(T, S, dst, ring_P[r], i - S.n_dense, i + 1);
    for (int k = 0; k < S.n_dense; ++k) dst[k] = P > 0 ? row[k] : 0.0;
    ring_P[r] = P > 0 ? P : 0;
}

}  // namespace fot
