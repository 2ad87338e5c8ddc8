// fot_sweep.hpp -- the layout arithmetic of a sweep loop (fot_loop_begin_sweep): every slot on its own scenario AND in
// its own plan mode over a step's sample distributions.  The step's tensor holds every running episode's distribution
// block [S][P_e][T][2] as in any distribution loop; behind them, compacted in frame order, follow the single-sample
// planning blocks [P_e][T][2] (fot_repsample.hpp) of the episodes in FOT_LOOP_PLAN_REPRESENTATIVE mode.  A request then
// addresses its episode's distribution block with S samples or its planning block with one, on the same base pointer.
// Also the row -> column table of a recording whose columns the slots name themselves (fot_loop_set_samples_shared), and
// the tables of a sampler step whose slots share their crowds' samples (fot_loop_set_sampler_shared) and name their
// models (fot_loop_set_sampler_models), and the ragged layout of a sweep whose slots keep sample counts of their own
// (fot_loop_set_slot_samples).
// Plain C++ shared by the kernels (k_loop_best_sample_sweep, k_loop_rep_block_sweep, k_loop_model_rows), the host (fot_host_loop.cpp) and
// tests/emu/fot_sweep_emu.cpp, tests/emu/fot_slot_samples_emu.cpp.  Every offset into the tensor counts points of two coordinates in 64 bits.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

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

// ---- a sample count per slot (fot_loop_set_slot_samples) -------------------------------------------------------------------------
// Slot e plans against the first slot_S[e] samples of what the loop's source provides.  Running episode i then keeps a
// block [S_i][P_i][T][2], the blocks packed by prefix sum; the planning blocks follow behind them as sweep_layout places
// them (dist_end = what sweep_slot_blocks returns).  The counts live in a table of their own, [n_run], beside the SweepEp
// rows: SweepEp stays as it is.

// ep_S [n_run]: the count of every running episode of the frame (ep_slot == nullptr: episode i is slot i).  Returns the
// largest of them (0 for no episode).
inline int32_t sweep_slot_counts(int32_t n_run, const int32_t *ep_slot, const int32_t *slot_S, int32_t *ep_S)
{
    int32_t most = 0;
    for (int32_t i = 0; i < n_run; ++i) {
        ep_S[i] = slot_S[ep_slot ? ep_slot[i] : i];
        most = std::max(most, ep_S[i]);
    }
    return most;
}

// points of the distribution block of an episode of S samples, P pedestrians and T time entries
FOT_SW_HD inline int64_t sweep_slot_block_points(int32_t S, int32_t P, int32_t T) { return (int64_t)S * P * T; }

// blk [n_run + 1]: first point of every running episode's distribution block, blk[n_run] (returned) the points of them all.
// With every count equal to S this is the uniform frame's table (LoopState::blk_off).
inline int64_t sweep_slot_blocks(int32_t n_run, const int32_t *ep_ped0, const int32_t *ep_S, int32_t T, int64_t *blk)
{
    blk[0] = 0;
    for (int32_t i = 0; i < n_run; ++i) blk[i + 1] = blk[i] + sweep_slot_block_points(ep_S[i], ep_ped0[i + 1] - ep_ped0[i], T);
    return blk[n_run > 0 ? n_run : 0];
}

// The most points a step of a resident sweep loop with slot counts can need: every slot running, its distribution block
// and a planning block each.  slot_ped0 [n_slots + 1]: the replay's.  Never more than sweep_capacity_points of the
// source's S, which is what the loop's tensor was sized with.
inline int64_t sweep_slot_capacity_points(int32_t n_slots, const int32_t *slot_ped0, const int32_t *slot_S, int32_t T)
{
    int64_t pts = 0;
    for (int32_t e = 0; e < n_slots; ++e) pts += ((int64_t)slot_S[e] + 1) * (slot_ped0[e + 1] - slot_ped0[e]) * T;
    return pts;
}

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

// ---- crowds: the slots of a sampler loop that share one sampling (fot_loop_set_sampler_shared) ---------------------------------
// slot_crowd [n_slots] names every slot's crowd.  A crowd is ACTIVE in a frame when one of its slots runs and has
// pedestrians; the active crowds, in ascending id, are the sampler's scenes, and a scene's pedestrians are those of the
// crowd's REPRESENTATIVE, its lowest running slot.

struct CrowdShape {
    int32_t n_scenes = 0, crowd_rows = 0;    // what the generator is handed: active crowds, the pedestrians of their representatives
    bool identity = true;                    // col[r] == r for every row and crowd_rows == the frame's rows: nothing to gather
};

// The tables of a frame of n_run running episodes (ep_ped0 [n_run + 1], ep_slot [n_run] as in sweep_fill_columns):
//   scene_off   [n_scenes + 1]  first row of each scene in the crowds' tensor
//   row_scene   [crowd_rows]    scene of each of its rows
//   scene_slot  [n_scenes]      the representative slot (the window is gathered from its columns of the recording)
//   scene_crowd [n_scenes]      the crowd's id (the noise counter's `slot` word)
//   col         [rows]          for every row of the frame its column in the crowds' tensor [S][pred_len][crowd_rows][2]
// The arrays hold n_run + 1 / rows / n_run / n_run / rows entries.  The slots of a crowd have equal pedestrian counts
// (sweep_crowds_consistent).  Runs when the set of running slots changes, on the host only.
inline CrowdShape sweep_crowd_tables(int32_t n_run, const int32_t *ep_ped0, const int32_t *ep_slot, const int32_t *slot_crowd,
                                     int32_t *scene_off, int32_t *row_scene, int32_t *scene_slot, int32_t *scene_crowd,
                                     int32_t *col)
{
    std::vector<int32_t> order, ep_scene((size_t)(n_run > 0 ? n_run : 0), -1);
    for (int32_t i = 0; i < n_run; ++i)
        if (ep_ped0[i + 1] > ep_ped0[i]) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        const int32_t ca = slot_crowd[ep_slot[a]], cb = slot_crowd[ep_slot[b]];
        return ca != cb ? ca < cb : ep_slot[a] < ep_slot[b];
    });
    CrowdShape sh;
    scene_off[0] = 0;
    for (size_t k = 0; k < order.size(); ++k) {
        const int32_t i = order[k], c = slot_crowd[ep_slot[i]];
        if (k == 0 || c != slot_crowd[ep_slot[order[k - 1]]]) {   // a new crowd: this episode is its lowest running slot
            const int32_t P = ep_ped0[i + 1] - ep_ped0[i], sc = sh.n_scenes++;
            scene_slot[sc] = ep_slot[i]; scene_crowd[sc] = c;
            for (int32_t p = 0; p < P; ++p) row_scene[sh.crowd_rows + p] = sc;
            sh.crowd_rows += P;
            scene_off[sc + 1] = sh.crowd_rows;
        }
        ep_scene[(size_t)i] = sh.n_scenes - 1;
    }
    for (int32_t i = 0; i < n_run; ++i)
        for (int32_t row = ep_ped0[i]; row < ep_ped0[i + 1]; ++row) {
            col[row] = scene_off[ep_scene[(size_t)i]] + (row - ep_ped0[i]);
            sh.identity = sh.identity && col[row] == row;
        }
    sh.identity = sh.identity && sh.crowd_rows == ep_ped0[n_run > 0 ? n_run : 0];
    return sh;
}

// ---- models: the slots of a sampler loop name their Social-GAN model (fot_loop_set_sampler_models) ----------------------------
// slot_model [n_slots] names every slot's model, in [0, n_models).  A sampling UNIT is a (crowd, model) pair, active when
// one of its running slots has pedestrians.  Model m's scenes are its active units in ascending crowd id, a scene's
// pedestrians those of the unit's lowest running slot: sweep_crowd_tables over the running episodes that name m.

struct ModelShape {
    int32_t n_scenes = 0, rows = 0;          // what model m's generator is handed: its active units, their pedestrians
};

// One frame row's place among the models' raw tensors, model m's being [S][pred_len][rows_m][2] from element `base` of
// their common pool: sample s, predictor step j of the row is element base + (s * pred_len + j) * width + col.
struct ModelRow {
    int64_t base;                            // first element (of two coordinates) of the row's model's tensor
    int32_t width, col;                      // rows_m of that model | the row's column in it
};
static_assert(sizeof(ModelRow) == 16, "ModelRow is one 16-byte row");

FOT_SW_HD inline int64_t sweep_model_src_elem(const ModelRow &r, int32_t pred_len, int32_t s, int32_t j)
{
    return r.base + ((int64_t)s * pred_len + j) * (int64_t)r.width + r.col;
}

// The tables of a frame of n_run running episodes (ep_ped0, ep_slot, slot_crowd as in sweep_crowd_tables).  Model m's
// tables are sweep_crowd_tables' of the episodes that name it, at
//   scene_off + m * (ep_stride + 1), scene_slot + m * ep_stride, scene_crowd + m * ep_stride, row_scene + m * row_stride
// (ep_stride >= n_run, row_stride >= the frame's rows); shape [n_models].  For every row of the frame: row_model [rows]
// its model and col [rows] its column in that model's tensor.  A model without an active unit has n_scenes = rows = 0.
// With n_models = 1 the tables are sweep_crowd_tables' own.  Runs when the set of running slots changes, on the host only.
inline void sweep_model_tables(int32_t n_run, const int32_t *ep_ped0, const int32_t *ep_slot, const int32_t *slot_crowd,
                               const int32_t *slot_model, int32_t n_models, int32_t ep_stride, int32_t row_stride,
                               ModelShape *shape, int32_t *scene_off, int32_t *row_scene, int32_t *scene_slot,
                               int32_t *scene_crowd, int32_t *row_model, int32_t *col)
{
    std::vector<int32_t> sub, sub_ped0, sub_slot, sub_col;
    for (int32_t m = 0; m < n_models; ++m) {
        sub.clear(); sub_ped0.assign(1, 0); sub_slot.clear();
        for (int32_t i = 0; i < n_run; ++i)
            if (slot_model[ep_slot[i]] == m) {
                sub.push_back(i);
                sub_slot.push_back(ep_slot[i]);
                sub_ped0.push_back(sub_ped0.back() + (ep_ped0[i + 1] - ep_ped0[i]));
            }
        sub_col.assign((size_t)sub_ped0.back(), 0);
        const CrowdShape sh = sweep_crowd_tables((int32_t)sub.size(), sub_ped0.data(), sub_slot.data(), slot_crowd,
                                                 scene_off + (size_t)m * ((size_t)ep_stride + 1), row_scene + (size_t)m * (size_t)row_stride,
                                                 scene_slot + (size_t)m * (size_t)ep_stride, scene_crowd + (size_t)m * (size_t)ep_stride,
                                                 sub_col.data());
        shape[m].n_scenes = sh.n_scenes; shape[m].rows = sh.crowd_rows;
        for (size_t k = 0; k < sub.size(); ++k) {
            const int32_t i = sub[k];
            for (int32_t row = ep_ped0[i]; row < ep_ped0[i + 1]; ++row) {
                row_model[row] = m;
                col[row] = sub_col[(size_t)(sub_ped0[k] + (row - ep_ped0[i]))];
            }
        }
    }
}

// The gather table of the frame's rows: model m's tensor starts at element model_base[m] of the pool.
inline void sweep_model_rows(int32_t rows, const int32_t *row_model, const int32_t *col, const ModelShape *shape,
                             const int64_t *model_base, ModelRow *tab)
{
    for (int32_t r = 0; r < rows; ++r) {
        const int32_t m = row_model[r];
        tab[r].base = model_base[m]; tab[r].width = shape[m].rows; tab[r].col = col[r];
    }
}

// Do the slots of every crowd replay the same pedestrians?  slot_ped0 [n_slots + 1], slot_frames [n_slots], pos the
// recording [n_frames_max][n_cols][2].  Every slot is held against the lowest slot of its crowd: 0 -- they agree; 1 -- the
// pedestrian counts differ; 2 -- the recorded frames; 3 -- some byte of the positions of a recorded frame.  *slot_a <
// *slot_b then name the two slots.
inline int sweep_crowds_consistent(int32_t n_slots, const int32_t *slot_ped0, const int32_t *slot_frames, const int32_t *slot_crowd,
                                   const double *pos, int32_t n_cols, int32_t *slot_a, int32_t *slot_b)
{
    for (int32_t e = 1; e < n_slots; ++e) {
        int32_t a = 0;
        while (a < e && slot_crowd[a] != slot_crowd[e]) ++a;
        if (a == e) continue;                                    // the lowest slot of its crowd
        *slot_a = a; *slot_b = e;
        const int32_t P = slot_ped0[e + 1] - slot_ped0[e];
        if (P != slot_ped0[a + 1] - slot_ped0[a]) return 1;
        if (slot_frames[a] != slot_frames[e]) return 2;
        for (int32_t f = 0; P > 0 && f < slot_frames[e]; ++f) {
            const double *row = pos + (int64_t)f * n_cols * 2;
            if (std::memcmp(row + 2 * (int64_t)slot_ped0[a], row + 2 * (int64_t)slot_ped0[e], sizeof(double) * 2 * (size_t)P) != 0) return 3;
        }
    }
    return 0;
}

}  // namespace fot
