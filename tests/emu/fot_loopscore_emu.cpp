// fot_loopscore_emu.cpp -- test-only shim: the representative-sample rule and the per-slot ring fold of a resident sampler
// loop's prediction scores (csrc/fot_loopscore.hpp, shared by k_loop_best_sample and the host) on the CPU.  Built with g++
// by tests/test_loop_scores_cpu.py; no HIP.
#include <cstdint>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_loopscore.hpp"

using namespace fot;

static_assert(sizeof(PredScoreTerms) == 56, "the record of fot_pred_score");

extern "C" {

// blk: [S][P][T][2] float64, the first `skip` entries of every track are not part of the rule; dev[S] receives the sums
int best_sample_run(int S, int P, int T, int skip, const double *blk, double *dev)
{
    auto at = [&](int s, int p, int k, int ax) { return blk[(((int64_t)s * P + p) * T + skip + k) * 2 + ax]; };
    return bs_choose(S, P, T - skip, at, dev);
}

int first_min_of(int S, const double *dev) { return bs_first_min(S, dev); }

// n_slots slots in lock step: slot e takes steps 0 .. L[e] - 1 with the records recs[e][L_max] and then stops while the
// others go on.  Whenever `at[j]` lock steps have been taken (ascending, 0 .. L_max) a summary of every slot is read off
// its totals -- the run goes on -- into out[j][e][8] = ade, fde, ade_per_agent, fde_per_agent, nll, ade count, nll count,
// pred_samples.
int score_ring_run(int H, int n_slots, const int32_t *L, int L_max, const PredScoreTerms *recs, int n_at, const int32_t *at,
                   double *out)
{
    std::vector<PredScoreTerms> ring((size_t)n_slots * H, ps_zero(0));
    std::vector<ScoreFold> fold((size_t)n_slots, score_fold_zero());
    int j = 0;
    for (int i = 0; i <= L_max; ++i) {
        for (; j < n_at && at[j] == i; ++j)
            for (int e = 0; e < n_slots; ++e) {
                double *o = out + ((size_t)j * n_slots + e) * 8;
                int32_t samples = 0;
                score_fold_means(fold[(size_t)e], o, &samples);
                o[5] = (double)fold[(size_t)e].count; o[6] = (double)fold[(size_t)e].nll_count; o[7] = (double)samples;
            }
        if (i == L_max) break;
        for (int e = 0; e < n_slots; ++e)
            if (i < L[e]) score_ring_push(fold[(size_t)e], ring.data() + (size_t)e * H, H, i, recs[(size_t)e * L_max + i]);
    }
    return j;
}

}  // extern "C"
