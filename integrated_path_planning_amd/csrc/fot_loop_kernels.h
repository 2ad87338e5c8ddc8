// fot_loop_kernels.h -- host-callable launchers of the prediction and closed-loop kernels (fot_loop_kernels.hip).
#pragma once

#include <cstddef>
#include <hip/hip_runtime.h>
#include "fot_types.h"
#include "fot_summary.hpp"
#include "fot_predscore.hpp"
#include "fot_loopscore.hpp"
#include "fot_repsample.hpp"
#include "fot_samplerec.hpp"
#include "fot_sweep.hpp"
#include "fot_openloop.hpp"
#include "fot_footprint_obs.hpp"
#include "fot_fidelity.hpp"
#include "fot_encounter.hpp"

namespace fot {

// every launcher returns 0 or the hipError_t of the launch
int launch_resample(double sgan_dt, double sim_dt, double staleness, int S, int pred_len, int P, int n_dense,
                    int has_anchor, int prepend, int cv, const void *pred, int pred_dtype, const double *anchor,
                    const double *current, void *out, int out_dtype, int tmajor, hipStream_t st,
                    const int32_t *ped_ep = nullptr, const int32_t *ep_ped0 = nullptr, const int64_t *ep_blk = nullptr);
int launch_sample_dist(int S, int P, int T, int skip, const void *out, int out_dtype, int tmajor, double *dist,
                       hipStream_t st);
// ---- fot_prediction_scores (fot_predscore.hpp): one workgroup per prediction origin
// What the kernel needs of an origin: its block (first point in the tensor), the first row of its pedestrians in `truth`
// ([rows][E][2]) and Scott's factor S^(-1/6), which the host forms.
struct PredOriginDev {
    int64_t offset, truth_row;
    double scott;
    int32_t S, P, T, tmajor, skip, _pad;
};
// desc / truth / out: HBM or pinned host memory.  The host has checked every origin (1 <= S <= FOT_MAX_SAMPLES -- wide: an
// origin of the launch has more, up to FOT_MAX_PLAN_SAMPLES, and k_pred_scores_wide runs --, 1 <= E <= FOT_MAX_PRED_LEN,
// stride E - 1 < T - skip).  An origin's record is the same bits from either kernel.
int launch_pred_scores(const PredOriginDev *desc, int n, const void *tensor, int dtype, int stride, int E,
                       const double *truth, fot_pred_score *out, hipStream_t st, int wide = 0);
// What the safety metrics need of a scenario beyond its DevParams: element s of a table in HBM belongs to scenario s.
struct SafetyScen {
    double footprint_radius;
    int32_t use_fp;                                  // the loop's metrics use this scenario's multi-circle footprint
    int32_t _pad;
};
// ep_scen == nullptr: every ego on scenario P[0] with footprint_radius / use_fp as given.  Otherwise ego e is on scenario
// ep_scen[e]: its constants are P[ep_scen[e]], its footprint radius and flag scen_tab[ep_scen[e]] (the two arguments are
// then ignored).
int launch_safety(const DevParams *P, int n, const double *ego, const int32_t *ped_off, const double *ped_pos,
                  const double *ped_vel, double ego_radius, double ped_radius, double footprint_radius, int use_fp,
                  fot_safety *out, hipStream_t st, const int32_t *ep_scen = nullptr, const SafetyScen *scen_tab = nullptr);
// The static obstacle points of a scenario loop's requests: request j's points are n points from point src of `points`
// (the scenarios' point sets, each once in HBM), copied to point dst of `out` -- the static_off layout k_cull reads.
// The table lies in pinned host memory or HBM; the host has checked every range.
struct StaticGather {
    int32_t src, dst, n, _pad;
};
int launch_static_gather(const StaticGather *tab, int n_req, const double *points, double *out, hipStream_t st);
// ---- fot_loop_run: the frame of a lock step built from the HBM-resident recording, and what the host reads of a step

// The recording fot_loop_set_replay left in HBM and the per-slot tables beside it.
struct ReplayView {
    const double *pos = nullptr, *vel = nullptr;     // [n_frames_max][n_cols][2]
    const int32_t *slot_ped0 = nullptr;              // [n_slots + 1] first column of each slot
    const int32_t *slot_frames = nullptr;            // [n_slots] recorded frames (the last one is held afterwards)
    int n_cols = 0;
};

// What the host stages for a step's frame in pinned memory (one entry per RUNNING episode, slot order): k_loop_frame
// moves it into HBM with the pedestrians, so that the step's other kernels read HBM only.
struct FrameStage {
    const int32_t *slot = nullptr;                   // [n_run] slot of running episode i
    const int32_t *ped0 = nullptr;                   // [n_run + 1] first row of episode i in the compacted frame
    const int64_t *blk = nullptr;                    // [n_run + 1] first point of episode i's block of the prediction tensor
    const int32_t *prepend = nullptr;                // [n_run] 1: the current positions lead episode i's tracks
    const double *ego = nullptr;                     // [n_run][4] x, y, yaw, v
    const int32_t *scen = nullptr;                   // [n_run] scenario of running episode i, or nullptr (all on scenario 0)
};

// The compacted frame in HBM: rows [ped0[i], ped0[i + 1]) belong to running episode i.
struct FrameDev {
    double *pos = nullptr, *vel = nullptr;           // [rows][2] current positions / velocities
    double *last = nullptr, *prev = nullptr;         // [rows][2] the observer's last two samples, rounded through float32
    int32_t *ped_ep = nullptr;                       // [rows] running episode of each row
    int32_t *ped0 = nullptr;                         // [n_run + 1]
    int64_t *blk = nullptr;                          // [n_run + 1]
    int32_t *prepend = nullptr;                      // [n_run]
    double *ego = nullptr;                           // [n_run][4]
    int32_t *scen = nullptr;                         // [n_run], written when FrameStage::scen is given
};

// What the host needs of a record to replay the retry loop and move the ego: the record's first 80 bytes as they are
// (fot_result up to new_prev_s) and sample 1 of x, y, yaw, v, a.  128 bytes = eight 16-byte stores per record.
struct LoopDigest {
    int32_t status, best_index, n_cand, n_keep;
    double cost;
    int32_t stats[8];
    int32_t stats_valid, _pad;
    double new_last_kappa, new_prev_s;
    double x1, y1, yaw1, v1, a1, _zero;
};
static_assert(sizeof(LoopDigest) == 128 && offsetof(LoopDigest, x1) == offsetof(fot_result, frenet0) &&
              offsetof(LoopDigest, new_prev_s) == offsetof(fot_result, new_prev_s) && sizeof(fot_result) % 16 == 0,
              "LoopDigest starts with fot_result's header");

// f_cur / f_last / f_prev: replay frames of the current positions and of the observer's last two samples (f_last < 0:
// the observer still fills, last / prev are not written)
int launch_loop_frame(ReplayView rv, FrameStage in, FrameDev out, int n_run, int f_cur, int f_last, int f_prev,
                      hipStream_t st);
// fot_loop_set_samples: row d.rec_row of the recording rec [n_steps][S][pred_len][n_cols][2] -> the step's raw samples
// out [S][pred_len][rows][2] of the running slots, both of element type dtype (FOT_F32 | FOT_F64); row q of the frame is
// column col[q] of the recording (HBM; fot_samplerec.hpp's sr_fill_columns).  rec is only read.
struct LoopSampleRows {
    SampleRecDims d;
    const void *rec;
    const int32_t *col;                      // [rows]
    void *out;
    int32_t dtype, _pad;
};
int launch_loop_sample_rows(const LoopSampleRows &a, hipStream_t st);
// fot_loop_set_sampler_models: the models' raw tensors (float32, [S][pred_len][rows_m][2] each, in one pool) -> the step's
// raw samples out [S][pred_len][rows][2] of the running slots; tab [rows] names every frame row's tensor, its width and
// the row's column in it (HBM; fot_sweep.hpp's sweep_model_rows).  pool is only read.
struct LoopModelRows {
    int32_t S, pred_len, rows, _pad;
    const float2 *pool;
    const ModelRow *tab;                     // [rows]
    float2 *out;
};
int launch_loop_model_rows(const LoopModelRows &a, hipStream_t st);
// constant-velocity tracks of every row of the frame in ONE launch, episode i's [P_i][n_dense + prepend[i]][2] block at
// point blk[i] of `out`: k_resample's float32-observation path (cv = 2) with the prepend decided per episode
int launch_predict_cv_frame(double sgan_dt, double sim_dt, double staleness, int n_rows, int n_dense, FrameDev f,
                            double *out, hipStream_t st);
// digests of rec[0 .. n) into pinned memory, then `*done = seq` behind a system-scope release
int launch_loop_digest(const fot_result *rec, int n, LoopDigest *out, int32_t *done, int32_t seq, hipStream_t st);
// end of a step: raises `*done = seq` (everything in front of it on the stream is then in host memory) and, with hist,
// copies the first n_total samples of the 15 path arrays of rec[src[i]] (src[i] < 0: none) into
// hist[15][n_slots][n_total] at slot[i]; src / slot are pinned host memory
int launch_loop_history(const fot_result *rec, int n_run, const int32_t *src, const int32_t *slot, double *hist,
                        int n_slots, int n_total, int32_t *done, int32_t seq, hipStream_t st);
// ---- fot_loop_summaries (fot_summary.hpp): the prediction error of a resident loop
// Behind the step's prediction: running episode i (slot slot_of[i], pinned host memory) writes the row of lock step
// `step` -- sum over its pedestrians of the distance between dense sample k of its block of `dyn` (the prepended column
// skipped) and recording row min(f_cur + 1 + k, frames - 1) -- into place step % n_dense of its ring and folds the row it
// replaces into totals[slot].  have_pred == 0 (observer not ready) or no pedestrians: an empty row.  best (HBM, per slot;
// nullptr: none): episode i's block is a distribution [S][P][T][2] and its row is that of sample best[slot].
int launch_loop_pred_error(ReplayView rv, const int32_t *slot_of, FrameDev f, const double *dyn, int n_run, int have_pred,
                           int f_cur, int step, SummaryShape S, double *ring, int32_t *ring_P, SummaryTotals *totals,
                           hipStream_t st, const int32_t *best = nullptr);
// ---- fot_loop_scores_enable (fot_loopscore.hpp): a resident sampler loop scores its predictor
// The representative sample of running episode i's [S][P_i][n_dense + 1][2] block at point f.blk[i] of `dyn`:
// dev_tab[slot][best_dev_stride(S)] (HBM) receives the S deviation sums, best_tab[slot] (HBM) and best_host[slot] (pinned)
// the first minimum, -1 for an episode without pedestrians.  slot_of: pinned host memory.  S <= FOT_MAX_SAMPLES runs
// k_loop_best_sample (rows FOT_MAX_SAMPLES apart, as ever), more -- up to FOT_MAX_PLAN_SAMPLES -- k_loop_best_sample_wide,
// which takes the stride as an argument.  Whoever sizes or reads the table uses best_dev_stride of the same S.
inline int best_dev_stride(int S) { return S > FOT_MAX_SAMPLES ? S : FOT_MAX_SAMPLES; }
int launch_loop_best_sample(const int32_t *slot_of, FrameDev f, const double *dyn, int n_run, int S, int n_dense,
                            double *dev_tab, int32_t *best_tab, int32_t *best_host, hipStream_t st);
// ---- fot_loop_plan_sample (fot_repsample.hpp): behind launch_loop_best_sample, running episode i's planning block
// [P_i][n_dense + 1][2] at point f.ped0[i] * (n_dense + 1) of `rep` (HBM) from sample best_tab[slot_of[i]] of its
// distribution block and the current positions f.pos; pre_dev[i] (HBM) and pre_host[i] (pinned) receive 1 where the
// current positions lead the block.  Only f.pos, f.ped0 and f.blk are read; an episode without pedestrians writes nothing.
int launch_loop_rep_block(const int32_t *slot_of, FrameDev f, const double *dyn, const int32_t *best_tab, int n_run, int S,
                          int n_dense, double *rep, int32_t *pre_dev, int32_t *pre_host, hipStream_t st);
// ---- fot_loop_begin_sweep (fot_sweep.hpp): the two launches above with a row of tab (pinned host memory) per running
// episode.  Only episodes with tab[i].select choose a sample (the others' table entries are left alone); only episodes
// with tab[i].rep_off >= 0 write a planning block, at that point of `tensor` -- the step's own tensor, behind the
// distribution blocks `dyn` reads.  An episode's numbers are those of the uniform launches, bit for bit.
int launch_loop_best_sample_sweep(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab, int n_run, int S,
                                  int n_dense, double *dev_tab, int32_t *best_tab, int32_t *best_host, hipStream_t st);
int launch_loop_rep_block_sweep(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab,
                                const int32_t *best_tab, int n_run, int S, int n_dense, double *tensor, int32_t *pre_dev,
                                int32_t *pre_host, hipStream_t st);
// ---- fot_loop_set_slot_samples (fot_sweep.hpp): a sweep loop's step whose running episode i keeps ep_S[i] samples (pinned
// host memory, as tab).  launch_resample_slots: the first ep_S[i] samples of the raw tensor pred [S_src][pred_len][rows][2]
// into episode i's [ep_S[i]][P_i][n_dense + 1][2] block at point ep_blk[i] of `out` -- launch_resample's anchored,
// prepending float64 path; S_max / P_max: the largest count / pedestrian count among the running episodes (the grid).
// launch_loop_sample_rows_prefix: launch_loop_sample_rows moving the first a.d.S of the source's S_src samples.  The
// selection and the planning blocks as in the sweep forms, every episode on its own count; dev_tab's rows are dev_stride
// apart; a step whose counts are all <= FOT_MAX_SAMPLES (S_max) takes the narrow selection.
int launch_resample_slots(double sgan_dt, double sim_dt, double staleness, int S_max, int pred_len, int rows, int n_dense,
                          int n_run, int P_max, const void *pred, int pred_dtype, const double *anchor, const double *current,
                          double *out, const int32_t *ep_ped0, const int64_t *ep_blk, const int32_t *ep_S, hipStream_t st);
int launch_loop_sample_rows_prefix(const LoopSampleRows &a, int S_src, hipStream_t st);
int launch_loop_best_sample_slots(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab, const int32_t *ep_S,
                                  int n_run, int S_max, int n_dense, double *dev_tab, int dev_stride, int32_t *best_tab,
                                  int32_t *best_host, hipStream_t st);
int launch_loop_rep_block_slots(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab, const int32_t *ep_S,
                                const int32_t *best_tab, int n_run, int n_dense, double *tensor, int32_t *pre_dev,
                                int32_t *pre_host, hipStream_t st);
// The truth k_pred_scores reads for the step's origins, out[n_rows][E][2] (HBM): recording row min(f_cur + stride j,
// frames - 1), j = 1 .. E, of every row of the frame.
int launch_loop_score_truth(ReplayView rv, const int32_t *slot_of, FrameDev f, int n_rows, int f_cur, int stride, int E,
                            double *out, hipStream_t st);
// totals + the ring's rows under steps[slot] (pinned) -> the prediction-error keys and counts of out[slot] (pinned); the
// other fields of the record are the host's.  Changes nothing in HBM.
int launch_loop_summary(SummaryShape S, const double *ring, const int32_t *ring_P, const SummaryTotals *totals,
                        const int32_t *steps, int n_slots, int num_samples, fot_loop_summary *out, hipStream_t st);
// ---- fot_openloop_eval (fot_openloop.hpp): the rows of a chunk of windows gathered from the scene [n_frames][n_cols][2]
// (HBM, element type dtype: FOT_F32 | FOT_F64).  Row r is column row_col[r] of the window that starts at frame row_f0[r]
// (HBM tables; the host has checked every row against the scene): its observation window in float32, obs [obs_len][rows]
// [2]; its anchor, that float32 last observation widened, anchor [rows][2]; its truth, frames obs_len .. obs_len +
// pred_len - 1 of the window in float64, truth [rows][pred_len][2] -- what sgan_enqueue / launch_resample /
// launch_pred_scores read.
struct OpenLoopRows {
    const void *scene;
    const int32_t *row_col, *row_f0;         // [rows]
    int32_t dtype, n_cols, rows, obs_len, pred_len, _pad;
    float2 *obs;
    double2 *anchor, *truth;
};
int launch_openloop_rows(const OpenLoopRows &a, hipStream_t st);
// ---- fot_footprint_recheck (fot_footprint_obs.hpp).  Pose i is (xy[i xy_stride], xy[i xy_stride + 1]) with the heading
// yaw[i yaw_stride] -- xy [n][2] and yaw [n] of a recheck, or both inside the loop's [n][4] ego rows -- and its
// pedestrians are rows ped_off[i] .. ped_off[i + 1] of ped_xy; out[i] is its {legacy, multi, rect} record.  geom: HBM or
// pinned memory.
int launch_footprint_steps(const FpoGeom *geom, int n, const double *xy, int xy_stride, const double *yaw, int yaw_stride,
                           const int32_t *ped_off, const double *ped_xy, FpoStep *out, hipStream_t st);
// the headings of n_traj trajectories (steps step_off[t] .. step_off[t + 1] of xy [steps][2], each of two steps at
// least) reconstructed from their positions: yaw_out [steps]
int launch_footprint_yaw(int n_traj, const int32_t *step_off, const double *xy, double *yaw_out, hipStream_t st);
// the trajectories' records from their steps' records
int launch_footprint_fold(const FpoGeom *geom, int n_traj, const int32_t *step_off, const int32_t *ped_off,
                          const FpoStep *series, FpoRecord *out, hipStream_t st);

// ---- fot_fidelity_eval (fot_fidelity.hpp).  Encounter e owns the steps step_off[e] .. step_off[e + 1] - 1 of ego [steps][2]
// and the rows row_off[e] .. of ped_xy / ped_vel / truth ([T_e][N_e][2] each, back to back; ped_vel and truth may be NULL);
// its pedestrians are entries ped_base[e] .. ped_base[e + 1] - 1 of the per-pedestrian arrays.  One launch each: lane =
// pedestrian (onset, error sum, kept), lane = step (separation), wave = encounter (record).
struct FidelityArgs {
    int32_t n_enc;
    int64_t n_steps, n_peds;
    const int32_t *step_off, *n_ped;             // [n_enc + 1] | [n_enc]
    const double *dt;                            // [n_enc]
    const int64_t *row_off, *ped_base;           // [n_enc + 1] each
    const double *ego, *ped_xy, *ped_vel, *truth;
    FidParams p;
    double *series;                              // [steps]
    double *onset_dist, *ped_sum;                // [sum N]
    int32_t *onset_step, *ped_keep;              // [sum N]
    FidEnc *out;                                 // [n_enc]
};
int launch_fidelity(const FidelityArgs &a, hipStream_t st);

// ---- fot_encounters_extract (fot_encounter.hpp).  The clip as it lies in HBM: ped_xy / ped_vel [T][A][2] (ped_vel NULL: the
// forward-difference fallback over the whole grid), ego_xy [K][T][2].
struct EncScene {
    const double *ped_xy, *ped_vel, *ego_xy;
    int32_t T, A;
    double dt;
};
struct EncSpanOut { EncMin m; int32_t n_ped, pad_; };            // a span's closest approach and population
// the spans that are long enough, n_go of them: span [n_go][4] = vehicle, frame0, frame1, 0.  Block = 64 columns x
// ENC_STEP_WAVES shares of the steps -> col [n_go][A]; then a wave per span compacts the present columns, ascending, into
// cols [n_go][A] and joins their minima -> out [n_go]
struct EncSpansArgs {
    EncScene s;
    int32_t n_go;
    const int32_t *span;
    EncCol *col;
    int32_t *cols;
    EncSpanOut *out;
};
int launch_enc_spans(const EncSpansArgs &a, hipStream_t st);
// the kept spans, n_kept of them, in fot_fidelity_eval's tables (step_off, n_ped, row_off, ped_base as in FidelityArgs):
// kept [n_kept][4] = vehicle, frame0, index among the n_go spans, 0.  Lane = cell (step, pedestrian) of the packed layout:
// packed_xy [cells][2] (or NULL) and, per pedestrian over its steps, speeds / free_speeds [cells] (or NULL; free_speeds
// NaN where the step is not free-walking); then a wave per kept pedestrian: col_out, cruise, goals [rows]
struct EncRowsArgs {
    EncScene s;
    EncParams p;
    int32_t n_kept;
    int64_t n_rows, n_cells;
    const int32_t *kept, *step_off, *n_ped;
    const int64_t *row_off, *ped_base;
    const int32_t *cols;
    double *packed_xy, *speeds, *free_speeds;
    int32_t *col_out;
    double *cruise, *goals;
};
int launch_enc_rows(const EncRowsArgs &a, hipStream_t st);

}  // namespace fot
