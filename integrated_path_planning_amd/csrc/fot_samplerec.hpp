// fot_samplerec.hpp -- the index arithmetic of a recorded sample tensor (fot_loop_set_samples): from an element of a lock
// step's raw tensor [S][pred_len][rows][2] -- rows: the pedestrians of the RUNNING episodes, compacted as k_loop_frame
// leaves them -- to its place in the recording [n_steps][S][pred_len][n_cols][2], whose columns are those of all slots in
// the replay's own order.  Plain C++ shared by the kernel (k_loop_sample_rows, fot_loop_kernels.hip), the host
// (fot_host_loop.cpp) and tests/emu/fot_samplerec_emu.cpp.  Every offset into the recording is 64-bit: 256 episodes x 30
// pedestrians x 20 samples x 12 steps x 274 lock steps are 1.0e9 coordinates, and a longer run or more samples pass 2^31
// elements.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FOT_SR_HD __host__ __device__
#else
#define FOT_SR_HD
#endif

namespace fot {

// What one step's gather needs besides the tables: the recording's shape and the row the step reads.
struct SampleRecDims {
    int32_t S = 0, pred_len = 0;
    int32_t rows = 0;                        // pedestrians of the running episodes (the frame's rows)
    int32_t n_cols = 0;                      // pedestrians of all slots (the recording's columns)
    int64_t rec_row = 0;                     // lock step - first_step
};

// elements (of two coordinates) of one step's raw tensor: one lane each
FOT_SR_HD inline int64_t sr_step_elems(const SampleRecDims &d) { return (int64_t)d.S * d.pred_len * d.rows; }

// lane t -> (s, j, row), rows innermost: the lanes of a wave read and write runs of neighbouring pedestrians
FOT_SR_HD inline void sr_split(const SampleRecDims &d, int64_t t, int32_t &s, int32_t &j, int32_t &row)
{
    if (t <= (int64_t)UINT32_MAX) {          // (what every realistic step takes: 32-bit divisions, a tenth of the 64-bit ones)
        const uint32_t t32 = (uint32_t)t, sj = t32 / (uint32_t)d.rows;
        row = (int32_t)(t32 - sj * (uint32_t)d.rows);
        s = (int32_t)(sj / (uint32_t)d.pred_len);
        j = (int32_t)(sj - (uint32_t)s * (uint32_t)d.pred_len);
        return;
    }
    const int64_t sj = t / d.rows;
    row = (int32_t)(t - sj * d.rows);
    s = (int32_t)(sj / d.pred_len);
    j = (int32_t)(sj - (int64_t)s * d.pred_len);
}

// Frame row -> column of the recording.  ped_ep [rows] running episode of each row, ep_ped0 [n_run + 1] first row of each
// running episode (FrameDev::ped_ep, ped0), ep_slot [n_run] its slot, slot_ped0 [n_slots + 1] the replay's first column of
// each slot.
FOT_SR_HD inline int32_t sr_column(int32_t row, const int32_t *ped_ep, const int32_t *ep_ped0, const int32_t *ep_slot,
                                   const int32_t *slot_ped0)
{
    const int32_t i = ped_ep[row];
    return slot_ped0[ep_slot[i]] + (row - ep_ped0[i]);
}

// The same for every row of a frame, episode by episode: col [ep_ped0[n_run]].  The set of running slots changes a few
// times in a run, so the host forms this table when it does and the kernel reads it from HBM -- a lane then touches no
// table in host memory.  (The host calls fot_sweep.hpp's sweep_fill_columns: this, with first columns the caller may name.)
inline void sr_fill_columns(int32_t n_run, const int32_t *ep_ped0, const int32_t *ep_slot, const int32_t *slot_ped0,
                            int32_t *col)
{
    for (int32_t i = 0; i < n_run; ++i)
        for (int32_t row = ep_ped0[i]; row < ep_ped0[i + 1]; ++row) col[row] = slot_ped0[ep_slot[i]] + (row - ep_ped0[i]);
}

// element (s, j, col) of row d.rec_row of the recording
FOT_SR_HD inline int64_t sr_src_elem(const SampleRecDims &d, int32_t s, int32_t j, int32_t col)
{
    return (((int64_t)d.rec_row * d.S + s) * d.pred_len + j) * (int64_t)d.n_cols + col;
}

// element (s, j, row) of the step's raw tensor (= the lane's own index)
FOT_SR_HD inline int64_t sr_dst_elem(const SampleRecDims &d, int32_t s, int32_t j, int32_t row)
{
    return ((int64_t)s * d.pred_len + j) * (int64_t)d.rows + row;
}

// elements of a whole recording of n_steps rows (what fot_loop_set_samples copies for a host recording)
FOT_SR_HD inline int64_t sr_rec_elems(int64_t n_steps, int32_t S, int32_t pred_len, int32_t n_cols)
{
    return n_steps * S * (int64_t)pred_len * n_cols;
}

// Does lock step `step` lie inside a recording of n_steps rows that starts at first_step?
FOT_SR_HD inline bool sr_covers(int32_t first_step, int32_t n_steps, int64_t step)
{
    return step >= first_step && step - first_step < n_steps;
}

}  // namespace fot
