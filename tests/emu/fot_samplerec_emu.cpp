// fot_samplerec_emu.cpp -- test-only shim: the index arithmetic of a recorded sample tensor (csrc/fot_samplerec.hpp, shared
// by k_loop_sample_rows and the host) on the CPU.  Built with g++ by tests/test_recorded_samples_cpu.py; no HIP.
#include <cstdint>

#include "../../integrated_path_planning_amd/csrc/fot_samplerec.hpp"

using namespace fot;

namespace {
SampleRecDims dims(int32_t S, int32_t pred_len, int32_t rows, int32_t n_cols, int64_t rec_row)
{
    SampleRecDims d;
    d.S = S; d.pred_len = pred_len; d.rows = rows; d.n_cols = n_cols; d.rec_row = rec_row;
    return d;
}
}  // namespace

extern "C" {

int64_t sr_step_elems_of(int32_t S, int32_t pred_len, int32_t rows) { return sr_step_elems(dims(S, pred_len, rows, 0, 0)); }

int64_t sr_rec_elems_of(int64_t n_steps, int32_t S, int32_t pred_len, int32_t n_cols) { return sr_rec_elems(n_steps, S, pred_len, n_cols); }

int sr_covers_of(int32_t first_step, int32_t n_steps, int64_t step) { return sr_covers(first_step, n_steps, step) ? 1 : 0; }

// lane t -> sjr[3] = (s, j, row)
void sr_split_of(int32_t S, int32_t pred_len, int32_t rows, int64_t t, int32_t *sjr)
{
    sr_split(dims(S, pred_len, rows, 0, 0), t, sjr[0], sjr[1], sjr[2]);
}

int64_t sr_src_of(int32_t S, int32_t pred_len, int32_t n_cols, int64_t rec_row, int32_t s, int32_t j, int32_t col)
{
    return sr_src_elem(dims(S, pred_len, 0, n_cols, rec_row), s, j, col);
}

int64_t sr_dst_of(int32_t S, int32_t pred_len, int32_t rows, int32_t s, int32_t j, int32_t row)
{
    return sr_dst_elem(dims(S, pred_len, rows, 0, 0), s, j, row);
}

int32_t sr_column_of(int32_t row, const int32_t *ped_ep, const int32_t *ep_ped0, const int32_t *ep_slot, const int32_t *slot_ped0)
{
    return sr_column(row, ped_ep, ep_ped0, ep_slot, slot_ped0);
}

void sr_fill_columns_of(int32_t n_run, const int32_t *ep_ped0, const int32_t *ep_slot, const int32_t *slot_ped0, int32_t *col)
{
    sr_fill_columns(n_run, ep_ped0, ep_slot, slot_ped0, col);
}

// k_loop_sample_rows' scheme, lane by lane: src[t] = the recording's element lane t reads, dst[t] = the one it writes
void sr_kernel_offsets(int32_t S, int32_t pred_len, int32_t rows, int32_t n_cols, int64_t rec_row, const int32_t *col,
                       int64_t *src, int64_t *dst)
{
    const SampleRecDims d = dims(S, pred_len, rows, n_cols, rec_row);
    for (int64_t t = 0; t < sr_step_elems(d); ++t) {
        int32_t s, j, q;
        sr_split(d, t, s, j, q);
        src[t] = sr_src_elem(d, s, j, col[q]);
        dst[t] = sr_dst_elem(d, s, j, q);
    }
}

}  // extern "C"
