// fot_predscore.hpp -- the arithmetic of the per-origin prediction scores (fot_prediction_scores /
// fot_loop_prediction_scores): best-of-N ADE / FDE, scene level and per agent, and the KDE log-likelihood of the truth
// under the samples (metrics.py:31-176).  Plain C++ shared by the kernel (k_pred_scores), the host (the shape rules and the
// zero record) and tests/emu/fot_predscore_emu.cpp, which evaluates an origin sequentially on the CPU.
//
// For one origin: samples q[s][p][k] (dense index k, the prepended current position skipped), evaluation indices
// k_j = stride j - 1, j = 1 .. E, truth g[p][j]; d[s][p][j] = |q[s][p][k_j] - g[p][j]|.
//   ade_scene     = min_s (sum_p (sum_j d)) / (P E)        fde_scene     = min_s (sum_p d[s][p][E]) / P
//   ade_agent_sum = sum_p min_s ((sum_j d) / E)            fde_agent_sum = sum_p min_s d[s][p][E]
//   KDE (S >= 2 and some (p, j, axis) with max_s q - min_s q > 0): per (p, j) and axis the bandwidth
//   b = max(sqrt(sum_s (q - mean)^2 / (S - 1)) S^(-1/6), 0.05) -- two passes: coordinates of tens of metres with spreads of
//   centimetres leave a sum-of-squares form without digits --, l_s = -1/2 sum_axis ((q - g) / b)^2 - log(2 pi b_x b_y),
//   log p = max(max_s l + log((sum_s exp(l_s - max_s l)) / S), -20); log_lik_sum = sum_{p, j} log p, nll_count = P E.
// Everything is float64 whatever the tensor's element type.  Every sum over s and over j runs in index order; sums over
// pedestrians and over (p, j) pairs run in an order fixed by (S, P, E) alone (the kernel: lane-strided partial sums, then
// a fixed tree; the sequential form here: index order), so the two agree to the rounding of a reordered sum.
// min / max propagate NaN as NumPy's min / maximum do.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FOT_PS_HD __host__ __device__ inline
#else
#define FOT_PS_HD inline
#endif

namespace fot {

constexpr double PS_BANDWIDTH_FLOOR = 0.05;      // KDE_BANDWIDTH_FLOOR [m] (metrics.py:14)
constexpr double PS_LOG_P_FLOOR = -20.0;         // KDE_NLL_LOG_P_FLOOR [nats] (metrics.py:19)
constexpr double PS_TWO_PI = 6.283185307179586476925286766559;
constexpr int PS_FLAG_NLL = 1;                   // fot_pred_score.flags: the KDE was evaluated
constexpr int PS_FLAG_NONFINITE = 2;             // ... a non-finite sample or truth coordinate was read

// np.min / np.maximum of two values: a NaN on either side wins
FOT_PS_HD double ps_min(double a, double b) { return (b < a || b != b) ? b : a; }
FOT_PS_HD double ps_max(double a, double b) { return (b > a || b != b) ? b : a; }
FOT_PS_HD bool ps_finite(double v) { return std::fabs(v) < __builtin_inf(); }

FOT_PS_HD double ps_dist(double qx, double qy, double gx, double gy)
{
    const double dx = qx - gx, dy = qy - gy;
    return std::sqrt(dx * dx + dy * dy);
}

// stride E - 1 < T - skip: the last evaluation index lies inside the dense track (metrics.py:78)
FOT_PS_HD bool ps_horizon_fits(int stride, int E, int T, int skip)
{
    return (int64_t)stride * E - 1 < (int64_t)T - skip;
}

// Scott's rule for two dimensions, S^(-1/6) (metrics.py:159); host side (the kernel gets it with the origin)
inline double ps_scott(int S) { return std::pow((double)S, -1.0 / 6.0); }

// One axis of one (p, j): q(s) -> coordinate of sample s.  Mean first, then the squared deviations; *varies: max - min > 0.
template <class Q>
FOT_PS_HD double ps_bandwidth(int S, double scott, const Q &q, bool *varies)
{
    double sum = 0.0, lo = q(0), hi = lo;
    for (int s = 0; s < S; ++s) {
        const double v = q(s);
        sum += v;
        lo = ps_min(lo, v); hi = ps_max(hi, v);
    }
    *varies = hi - lo > 0.0;
    const double mean = sum / (double)S;
    double ssd = 0.0;
    for (int s = 0; s < S; ++s) {
        const double dv = q(s) - mean;
        ssd += dv * dv;
    }
    return ps_max(std::sqrt(ssd / (double)(S - 1)) * scott, PS_BANDWIDTH_FLOOR);
}

// log p of the truth (gx, gy) under the S kernels of one (p, j); qx(s), qy(s) -> coordinates of sample s
template <class QX, class QY>
FOT_PS_HD double ps_log_p(int S, const QX &qx, const QY &qy, double gx, double gy, double bx, double by)
{
    const double norm = std::log(PS_TWO_PI * bx * by);
    auto l = [&](int s) {
        const double ux = (qx(s) - gx) / bx, uy = (qy(s) - gy) / by;
        return -0.5 * (ux * ux + uy * uy) - norm;
    };
    double peak = l(0);
    for (int s = 1; s < S; ++s) peak = ps_max(peak, l(s));
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += std::exp(l(s) - peak);
    return ps_max(peak + std::log(acc / (double)S), PS_LOG_P_FLOOR);
}

struct PredScoreTerms {
    double ade_scene, fde_scene, ade_agent_sum, fde_agent_sum, log_lik_sum;
    int32_t n_peds, n_samples, nll_count, flags;
};

FOT_PS_HD PredScoreTerms ps_zero(int S)
{
    PredScoreTerms t;
    t.ade_scene = t.fde_scene = t.ade_agent_sum = t.fde_agent_sum = t.log_lik_sum = 0.0;
    t.n_peds = 0; t.n_samples = S; t.nll_count = 0; t.flags = 0;
    return t;
}

// An origin evaluated sequentially: at(s, p, k, axis) -> coordinate of dense sample k (the skip already applied by the
// caller's accessor), truth [P][E][2].  The host-side form of what k_pred_scores computes, for the emulation.
template <class AT>
inline PredScoreTerms ps_origin(int S, int P, int stride, int E, const AT &at, const double *truth)
{
    PredScoreTerms t = ps_zero(S);
    if (P <= 0) return t;
    t.n_peds = P;
    bool nonfinite = false;
    for (int i = 0; i < P * E * 2; ++i) nonfinite |= !ps_finite(truth[i]);
    for (int s = 0; s < S; ++s) {
        double tot = 0.0, tot_f = 0.0;
        for (int p = 0; p < P; ++p) {
            double row = 0.0, last = 0.0;
            for (int j = 1; j <= E; ++j) {
                const int k = stride * j - 1;
                const double qx = at(s, p, k, 0), qy = at(s, p, k, 1);
                nonfinite |= !ps_finite(qx) || !ps_finite(qy);
                last = ps_dist(qx, qy, truth[(p * E + j - 1) * 2], truth[(p * E + j - 1) * 2 + 1]);
                row += last;
            }
            tot += row; tot_f += last;
        }
        const double a = tot / ((double)P * (double)E), f = tot_f / (double)P;
        t.ade_scene = s == 0 ? a : ps_min(t.ade_scene, a);
        t.fde_scene = s == 0 ? f : ps_min(t.fde_scene, f);
    }
    for (int p = 0; p < P; ++p) {
        double best_a = 0.0, best_f = 0.0;
        for (int s = 0; s < S; ++s) {
            double row = 0.0, last = 0.0;
            for (int j = 1; j <= E; ++j) {
                const int k = stride * j - 1;
                last = ps_dist(at(s, p, k, 0), at(s, p, k, 1), truth[(p * E + j - 1) * 2], truth[(p * E + j - 1) * 2 + 1]);
                row += last;
            }
            const double a = row / (double)E;
            best_a = s == 0 ? a : ps_min(best_a, a);
            best_f = s == 0 ? last : ps_min(best_f, last);
        }
        t.ade_agent_sum += best_a; t.fde_agent_sum += best_f;
    }
    if (nonfinite) t.flags |= PS_FLAG_NONFINITE;
    if (S < 2) return t;
    const double scott = ps_scott(S);
    bool any = false;
    double ll = 0.0;
    for (int p = 0; p < P; ++p)
        for (int j = 1; j <= E; ++j) {
            const int k = stride * j - 1;
            auto qx = [&](int s) { return at(s, p, k, 0); };
            auto qy = [&](int s) { return at(s, p, k, 1); };
            bool vx, vy;
            const double bx = ps_bandwidth(S, scott, qx, &vx), by = ps_bandwidth(S, scott, qy, &vy);
            any |= vx || vy;
            ll += ps_log_p(S, qx, qy, truth[(p * E + j - 1) * 2], truth[(p * E + j - 1) * 2 + 1], bx, by);
        }
    if (any) { t.log_lik_sum = ll; t.nll_count = P * E; t.flags |= PS_FLAG_NLL; }
    return t;
}

}  // namespace fot
