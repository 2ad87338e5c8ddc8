// fot_sweep.hpp -- the layout arithmetic of a sweep loop (fot_loop_begin_sweep): every slot on its own scenario AND in
// its own plan mode over a step's sample distributions.  The step's tensor holds every running episode's distribution
// block [S][P_e][T][2] as in any distribution loop; behind them, compacted in frame order, follow the single-sample
// planning blocks [P_e][T][2] (fot_repsample.hpp) of the episodes in FOT_LOOP_PLAN_REPRESENTATIVE mode.  A request then
// addresses its episode's distribution block with S samples or its planning block with one, on the same base pointer.
// Also the row -> column table of a recording whose columns the slots name themselves (fot_loop_set_samples_shared).
// Plain C++ shared by the kernels (k_loop_best_sample_sweep, k_loop_rep_block_sweep), the host (fot_host_loop.cpp) and
// tests/emu/fot_sweep_emu.cpp.  Every offset into the tensor counts points of two coordinates in 64 bits.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FOT_SW_HD __host__ __device__
#else
#define FOT_SW_HD
#endif

namespace fot {

constexpr int32_t SWEEP_DISTRIBUTION = 0, SWEEP_REPRESENTATIVE = 1;   // FOT_LOOP_PLAN_* (fot.h), restated for the tests

// What the step's selection and block kernels read of running episode i (pinned host memory, rewritten every step).
struct SweepEp {
    int64_t rep_off;                         // first point of its planning block in the tensor, or -1: it plans on the distribution
    int32_t select;                          // 1: its representative sample is chosen (it plans on it, or the loop scores)
    int32_t _pad;
};
static_assert(sizeof(SweepEp) == 16, "SweepEp is one 16-byte row");

FOT_SW_HD inline bool sweep_plans_on_block(const SweepEp &e) { return e.rep_off >= 0; }

// points of a planning block of P pedestrians and T time entries
FOT_SW_HD inline int64_t sweep_block_points(int32_t P, int32_t T) { return (int64_t)P * T; }

// The table of a frame of n_run running episodes.  ep_ped0 [n_run + 1] first row of each, ep_slot [n_run] its slot (or
// nullptr: episode i is slot i), slot_mode [slots] the slots' plan modes, dist_end: the points of the frame's distribution
// blocks, T: time entries of a planning block, select_all: the loop scores, so every episode's sample is chosen.
// Returns the tensor's size in points.  An episode without pedestrians keeps a block of no points.
inline int64_t sweep_layout(int32_t n_run, const int32_t *ep_ped0, const int32_t *ep_slot, const int32_t *slot_mode,
                            int64_t dist_end, int32_t T, bool select_all, SweepEp *tab)
{
    int64_t end = dist_end;
    for (int32_t i = 0; i < n_run; ++i) {
        const bool rep = slot_mode[ep_slot ? ep_slot[i] : i] == SWEEP_REPRESENTATIVE;
        tab[i].rep_off = rep ? end : -1;
        tab[i].select = rep || select_all ? 1 : 0;
        tab[i]._pad = 0;
        if (rep) end += sweep_block_points(ep_ped0[i + 1] - ep_ped0[i], T);
    }
    return end;
}

// The most points a step of a resident sweep loop can need: every slot running, S samples, n_cols pedestrians in all.
FOT_SW_HD inline int64_t sweep_capacity_points(int32_t S, int64_t n_cols, int32_t T) { return ((int64_t)S + 1) * n_cols * T; }

// Frame row -> column of a recording whose slots name their first column themselves: row r of running episode i is
// column slot_col0[ep_slot[i]] + (r - ep_ped0[i]).  Slots may share, overlap or reverse their columns.
// (fot_samplerec.hpp's sr_fill_columns is this with slot_col0 = the replay's own ped_off.)
inline void sweep_fill_columns(int32_t n_run, const int32_t *ep_ped0, const int32_t *ep_slot, const int32_t *slot_col0,
                               int32_t *col)
{
    for (int32_t i = 0; i < n_run; ++i)
        for (int32_t row = ep_ped0[i]; row < ep_ped0[i + 1]; ++row) col[row] = slot_col0[ep_slot[i]] + (row - ep_ped0[i]);
}

// Do all slots' column ranges lie inside a recording of n_rec_cols columns?  slot_ped0 [n_slots + 1]: the replay's.
inline bool sweep_columns_fit(int32_t n_slots, const int32_t *slot_ped0, const int32_t *slot_col0, int32_t n_rec_cols)
{
    for (int32_t e = 0; e < n_slots; ++e) {
        const int64_t P = (int64_t)slot_ped0[e + 1] - slot_ped0[e];
        if (slot_col0[e] < 0 || (int64_t)slot_col0[e] + P > n_rec_cols) return false;
    }
    return true;
}

}  // namespace fot
