// fot_summary_emu.cpp -- test-only shim: the ring / totals / truncated-tail arithmetic of the episode summaries
// (csrc/fot_summary.hpp, shared by k_loop_pred_error, k_loop_summary and the host) on the CPU.  Built with g++ by
// tests/test_loop_summary_cpu.py; no HIP.
#include <cstdint>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_summary.hpp"

using namespace fot;

extern "C" {

int summary_stride_of(double sgan_dt, double dt) { return summary_stride(sgan_dt, dt); }

// An episode of L steps whose step i has the row rows[i][n_dense] and P[i] pedestrians (0: no prediction) is pushed
// through the ring step by step; whenever the episode has at[j] steps (ascending, 0 .. L) a summary is taken -- from a
// copy of the totals, the run goes on -- into out[j][6] = ade, fde, planning_ade, planning_fde, ade count, planning count.
int summary_ring_run(int n_dense, int stride, int pred_len, int L, const double *rows, const int32_t *P, int n_at,
                     const int32_t *at, double *out)
{
    const SummaryShape S = summary_shape(n_dense, stride, pred_len);
    std::vector<double> ring((size_t)n_dense * n_dense, 0.0);
    std::vector<int32_t> ring_P((size_t)n_dense, 0);
    SummaryTotals T = SummaryTotals();
    int j = 0;
    for (int i = 0; i <= L; ++i) {
        for (; j < n_at && at[j] == i; ++j) {
            SummaryTotals C = T;
            summary_fold_tail(C, S, ring.data(), ring_P.data(), i);
            summary_means(C, out + 6 * j);
            out[6 * j + 4] = (double)C.std_count; out[6 * j + 5] = (double)C.plan_count;
        }
        if (i < L) summary_push_row(T, S, ring.data(), ring_P.data(), i, rows + (size_t)i * n_dense, P[i]);
    }
    return j;
}

}  // extern "C"
