// fot_loopscore.hpp -- what a resident sampler loop adds to score its predictor (fot_loop_scores_enable /
// fot_loop_score_summaries): the representative sample of a distribution and the per-slot fold of the per-origin records
// of fot_predscore.hpp into the episode's best-of-N and KDE keys.  Plain C++ shared by the kernel (k_loop_best_sample), the
// host and tests/emu/fot_loopscore_emu.cpp.
//
// Representative sample (predict_single_best, trajectory_predictor.py:346-351): over an episode's own pedestrians and the
// dense samples k (the prepended current position is not part of it), dev[s] = sum_{p, k} |q[s][p][k] - mean_s q[.][p][k]|;
// the FIRST minimum is chosen (np.argmin: a NaN counts as the smallest).  The mean adds the samples in index order.
//
// Fold (metrics.py:31-176 as BatchedClosedLoop.prediction_metrics folds the stepwise loop's records): the record of a
// slot's step i counts once the slot has taken step i + H, H = stride * pred_len (the reference's i + H < L).  A slot keeps
// its last H records in a ring, record i in place i % H; step i first folds the record it replaces.  Records still in the
// ring when a summary is asked for do not count.  The products ade_scene * n_peds are rounded before they are added, as
// NumPy's are: the file is compiled without contraction of a * b + c.
#pragma once

#include <cmath>
#include <cstdint>

#include "fot_predscore.hpp"

namespace fot {

// |(qx, qy) - (mx, my)|, squares and sum rounded one by one
FOT_PS_HD double bs_dev(double qx, double qy, double mx, double my)
{
#pragma clang fp contract(off)
    const double dx = qx - mx, dy = qy - my;
    const double xx = dx * dx, yy = dy * dy;
    return std::sqrt(xx + yy);
}

// np.argmin: the first minimum; the first NaN, if there is one
FOT_PS_HD int bs_first_min(int S, const double *dev)
{
    int best = 0;
    for (int s = 1; s < S; ++s) {
        const double v = dev[s], b = dev[best];
        if (v < b || (v != v && b == b)) best = s;
    }
    return best;
}

// An episode's block evaluated sequentially: at(s, p, k, axis) -> coordinate of dense sample k (the prepended entry
// already skipped), k < K.  dev[S] receives the sums in (p, k) index order.  The host-side form of k_loop_best_sample.
template <class AT>
inline int bs_choose(int S, int P, int K, const AT &at, double *dev)
{
    for (int s = 0; s < S; ++s) dev[s] = 0.0;
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < K; ++k) {
            double mx = 0.0, my = 0.0;
            for (int s = 0; s < S; ++s) { mx += at(s, p, k, 0); my += at(s, p, k, 1); }
            mx /= (double)S; my /= (double)S;
            for (int s = 0; s < S; ++s) dev[s] += bs_dev(at(s, p, k, 0), at(s, p, k, 1), mx, my);
        }
    return bs_first_min(S, dev);
}

// the running totals of a slot
struct ScoreFold {
    double ade, fde, ade_agent, fde_agent, log_lik;   // sums over the counted origins
    int64_t count, nll_count;                        // pedestrians | (pedestrian, evaluation step) pairs of them
    int32_t samples, _pad;                           // most samples of a counted origin
};

inline ScoreFold score_fold_zero()
{
    ScoreFold F;
    F.ade = F.fde = F.ade_agent = F.fde_agent = F.log_lik = 0.0;
    F.count = F.nll_count = 0; F.samples = 0; F._pad = 0;
    return F;
}

// one counted origin (a record without pedestrians contributes nothing)
inline void score_fold_add(ScoreFold &F, const PredScoreTerms &r)
{
#pragma clang fp contract(off)
    if (r.n_peds <= 0) return;
    const double a = r.ade_scene * (double)r.n_peds, f = r.fde_scene * (double)r.n_peds;
    F.ade += a; F.fde += f;
    F.ade_agent += r.ade_agent_sum; F.fde_agent += r.fde_agent_sum;
    F.count += r.n_peds;
    if (r.n_samples > F.samples) F.samples = r.n_samples;
    if (r.flags & PS_FLAG_NLL) { F.log_lik += r.log_lik_sum; F.nll_count += r.nll_count; }
}

// Step i of a slot: the record in place i % H (the one of step i - H, complete now) is folded, then replaced.
inline void score_ring_push(ScoreFold &F, PredScoreTerms *ring, int H, int i, const PredScoreTerms &r)
{
    PredScoreTerms &place = ring[i % H];
    if (i >= H) score_fold_add(F, place);
    place = r;
}

// ade, fde, ade_per_agent, fde_per_agent, nll (NaN without a counted origin / pair); pred_samples
inline void score_fold_means(const ScoreFold &F, double out[5], int32_t *pred_samples)
{
    const double nan = __builtin_nan("");
    const double c = (double)F.count;
    out[0] = F.count > 0 ? F.ade / c : nan;
    out[1] = F.count > 0 ? F.fde / c : nan;
    out[2] = F.count > 0 ? F.ade_agent / c : nan;
    out[3] = F.count > 0 ? F.fde_agent / c : nan;
    out[4] = F.nll_count > 0 ? -F.log_lik / (double)F.nll_count : nan;
    *pred_samples = F.count > 0 ? F.samples : 0;
}

}  // namespace fot
