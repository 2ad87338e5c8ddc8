// fot_host.hpp -- what the host units of libfot.so share (fot_host.cpp, fot_host_pred.cpp, fot_host_loop.cpp): the handle and the
// structures it owns, and the helpers that cross a unit boundary.  Internal, never installed; no launcher header is included here,
// so a unit depends only on the kernels it launches itself.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "fot_types.h"
#include "fot_setup.hpp"
#include "fot_replay.hpp"
#include "fot_summary.hpp"
#include "fot_loopscore.hpp"
#include "fot_sgan.hpp"
#include "fot_sweep.hpp"
#include "fot_footprint_obs.hpp"

// fot::host: internal to libfot.so -- hidden, so that what is declared here for the other host units is exported nowhere
namespace fot { namespace host __attribute__((visibility("hidden"))) {

// grow-only device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // the same, and a block that grew starts out all zero (record blocks: entries past n_total are never written)
    hipError_t ensure_zeroed(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        hipError_t e = ensure(bytes);
        return e != hipSuccess ? e : hipMemset(p, 0, cap);
    }
    template <class T> T *as() const { return (T *)p; }
};

struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 4 + 256;
        // fine-grained (coherent) whatever HIP_HOST_COHERENT says: kernels write records and their flags into these
        // blocks while the host polls them (wait_records)
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocCoherent | hipHostMallocMapped);
        if (e != hipSuccess) { p = nullptr; return e; }
        std::memset(p, 0, want);                                  // (record blocks: entries past n_total are never written)
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

}}  // namespace fot::host

// (the structures below stay global, beside the fot_handle of include/fot.h; the host units are written in these names)
using namespace fot;
using namespace fot::host;

// Per-lane workspace.  A large batch is split into FOT_LANES contiguous sub-batches that run on their own
// streams: the short, latency-bound kernels of one half (nearest-point search, tables, cull, select) overlap
// with the wide kernels of the other half instead of leaving the GPU idle between them.
struct Workspace {
    hipStream_t stream = nullptr;            // internal stream of this lane
    // The descriptors of a call are staged in a pinned block that the call's first kernel reads.  Two blocks take turns,
    // each with the event recorded BEHIND the last kernel of the call that used it: an event between two kernels costs
    // the second one about 6 us (profiles/r03_latency_anatomy.json: the gap behind k_frenet_state), and with two blocks
    // the host only ever waits for the call before the previous one.
    hipEvent_t staging_done[2] = { nullptr, nullptr };
    hipEvent_t done = nullptr;               // this lane's part of the current call has been enqueued up to here
    bool staging_pending[2] = { false, false };
    int staging_slot = 0;
    PinnedBuf staging[2];
    DevBuf dMeta;                            // InstDesc[]
    DevBuf dState;
    DevBuf dCost, dStatus, dKeep, dParts;
    DevBuf dEntCnt, dEnt32, dEnt64, dEntSid, dWaveRng;   // broad phase: culled entry lists + per-wave chunk ranges
    DevBuf dNanFlag;                         // one flag per pedestrian track (NanScan)
    DevBuf dDone;                            // tiles evaluated so far, per instance (tile_done)
    DevBuf dHeads;                           // GroupHead[n_inst][max_tiles / GROUP_TILES] of a grouped evaluation
    BatchLayout last;                        // layout of this lane's part of the most recent plan call
    int first_inst = 0;                      // global index of this lane's first instance
    void release()
    {
        DevBuf *bufs[] = { &dMeta, &dState, &dCost, &dParts, &dStatus, &dKeep,
                           &dWaveRng, &dEntCnt, &dEnt32, &dEnt64, &dEntSid, &dNanFlag, &dDone, &dHeads };
        for (DevBuf *b : bufs) b->release();
        for (int i = 0; i < 2; ++i) {
            staging[i].release();
            if (staging_done[i]) (void)hipEventDestroy(staging_done[i]);
        }
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// fot_loop_begin / fot_loop_step: the episodes' own state (what IntegratedSimulator, its planner and its
// FailSafeStateMachine carry from step to step), one slot per episode
struct LoopEpisodes {
    int n = 0;
    fot_loop_config cfg = fot_loop_config();  // of fot_loop_begin; of a scenario loop: the first scenario in use (dt)
    // fot_loop_begin_scenarios: every slot on a scenario of its own.  cfgs[s] / use_fp[s]: the fail-safe and simulator
    // constants and the metrics' footprint flag of scenario s (entries of scenarios no slot names are never read).
    bool scenarios = false;
    std::vector<fot_loop_config> cfgs;
    std::vector<int32_t> use_fp;
    std::vector<int32_t> scen;               // [n] scenario of each slot
    // fot_loop_begin_sweep: a scenario loop whose lock steps may carry a distribution; plan_mode[e]: FOT_LOOP_PLAN_* of slot e
    bool sweep = false;
    std::vector<int32_t> plan_mode;
    int max_lvl = 1;                         // most escalation levels of a configuration in use (sizes the record blocks)
    const fot_loop_config &cfg_of(int e) const { return scenarios ? cfgs[(size_t)scen[(size_t)e]] : cfg; }
    std::vector<double> ego;                 // [n][5] x, y, yaw, v, a
    std::vector<double> prev_s, last_kappa;  // planner.converter._prev_s (NaN: none yet), planner._last_kappa
    std::vector<double> goal_prev_s;         // the simulator's own converter (integrated_simulator.py:873)
    std::vector<double> last_clearance;      // clearance_ahead of the step's own metrics (emergency stop)
    std::vector<double> clear, clear_ahead;  // the state machine's _last_clearance / _last_clearance_ahead
    std::vector<int32_t> state, fails;       // 0 / 1 / 2 = NORMAL / CAUTION / EMERGENCY; consecutive failures
    std::vector<int32_t> stats;              // [n][8] last_check_stats, a row of -1: None
};

// fot_loop_summary_enable / fot_loop_summaries: the prediction-error ring and totals in HBM (fot_summary.hpp) and, per slot,
// what the host accumulates of every step's new ego state and metrics in step order
struct LoopSummaryAcc {
    bool on = false;
    int num_samples = 1;
    SummaryShape shape = SummaryShape();
    DevBuf dRing, dRingP, dTotals;               // [slots][n_dense][n_dense] rows | [slots][n_dense] counts | SummaryTotals[slots]
    PinnedBuf hOut, hSteps;                      // fot_loop_summary[slots] the kernel fills | steps of each slot
    std::vector<double> min_dist, min_ttc, max_jerk, sum_jerk, sum_jerk2, max_accel, sum_accel;
    std::vector<int32_t> collisions;
    void release() { dRing.release(); dRingP.release(); dTotals.release(); hOut.release(); hSteps.release(); }
};

constexpr int SGAN_MAX_MODELS = 8;           // fot_sgan_max_models(): models a handle holds (fot_sgan_load_model)

// fot_loop_set_sampler: the resident loop's Social-GAN predictor -- the window, the noise and the raw samples of a step in
// HBM, the noise kernel's row tables in pinned memory
struct LoopSampler {
    bool on = false;
    int S = 0, kind = 0;
    uint64_t seed = 0;
    DevBuf dWin, dNoise, dRaw;                   // [obs_len][rows][2] | [S][noise rows][nd] | [S][pred_len][rows][2], float32
    PinnedBuf hTab;                              // slot | step | index, n_cols + n_slots entries each
    // fot_loop_set_sampler_shared with a map other than slot e -> crowd e: one sampling per crowd (fot_sweep.hpp).  The
    // tables are rebuilt only when the set of running slots changes, as LoopSamples::sel.
    bool crowds = false;
    std::vector<int32_t> slot_crowd;             // [slots]
    std::vector<int32_t> sel;                    // the running slots the tables stand for (empty: none yet)
    std::vector<int32_t> scene_slot, scene_crowd;    // per scene: the representative slot, the crowd's id
    CrowdShape shape = CrowdShape();
    DevBuf dCrowdRaw, dCrowdTab;                 // [S][pred_len][crowd_rows][2] float32 | the tables as hCrowdTab holds them
    PinnedBuf hCrowdTab;                         // scene_off [slots + 1] | scene_slot [slots] | row_scene [cols] | col [cols]
    int last_scenes = 0, last_rows = 0;          // what the most recent lock step handed to the generator (fot_debug_loop_sampler_shape)
    // fot_loop_set_sampler_models with more than one model: one sampling per active (crowd, model) unit (fot_sweep.hpp).
    // Model m's window, noise, noise tables and raw tensor are the m-th parts of dWin, dNoise, hTab and dCrowdRaw, each
    // sized for n_cols rows; its scene tables the m-th parts of hCrowdTab / dCrowdTab.  A loop that names one model takes the
    // step above on the handle's model 0.
    int n_models = 1;
    bool models = false;
    size_t noise_stride = 0;                     // floats of a model's part of dNoise
    // the second and later active models of a step sample on side streams (side[m]: model m's), forked from and joined to
    // the loop's stream by events; FOT_LOOP_MODEL_STREAMS=0 at the set call keeps every model on the loop's stream
    bool side_on = false;
    hipStream_t side[SGAN_MAX_MODELS] = { nullptr };
    hipEvent_t fork = nullptr, join[SGAN_MAX_MODELS] = { nullptr };
    std::vector<int32_t> kinds;                  // [n_models] every model's noise kind
    std::vector<int32_t> slot_model;             // [slots]
    std::vector<ModelShape> mshape;              // [n_models] of the tables in force
    std::vector<int32_t> mscene_crowd;           // [n_models][slots] the crowd of each scene
    std::vector<int32_t> row_model, row_col;     // [cols] of the tables in force
    std::vector<int32_t> last_mscenes, last_mrows;   // [n_models] of the most recent lock step (fot_debug_loop_sampler_shapes)
    DevBuf dModelTab;                            // ModelRow[cols]
    PinnedBuf hModelTab;                         // ... as the host builds it
    void release()
    {
        dWin.release(); dNoise.release(); dRaw.release(); hTab.release();
        dCrowdRaw.release(); dCrowdTab.release(); hCrowdTab.release();
        dModelTab.release(); hModelTab.release();
        for (int m = 0; m < SGAN_MAX_MODELS; ++m) {
            if (side[m]) (void)hipStreamDestroy(side[m]);
            if (join[m]) (void)hipEventDestroy(join[m]);
            side[m] = nullptr; join[m] = nullptr;
        }
        if (fork) (void)hipEventDestroy(fork);
        fork = nullptr;
    }
};

// fot_loop_set_samples: the resident loop's recorded predictor (fot_samplerec.hpp) -- the recording in HBM (the library's
// copy of a host tensor, or the caller's device memory used in place), the raw samples of a step and the row -> column
// table of the running slots, rebuilt only when a slot drops out
struct LoopSamples {
    bool on = false;
    int S = 0, n_steps = 0, first_step = 0, dtype = FOT_F32;
    const void *rec = nullptr;                   // [n_steps][S][pred_len][n_cols][2]: dRec, or the caller's tensor
    DevBuf dRec, dRaw, dCol;                     // the copy | [S][pred_len][rows][2] of `dtype` | int32[rows]
    PinnedBuf hCol;                              // the table as the host builds it
    int n_rec_cols = 0;                          // the recording's columns (fot_loop_set_samples: the replay's n_cols)
    std::vector<int32_t> slot_col0;              // [slots] first column of each slot (fot_loop_set_samples: the replay's ped_off)
    std::vector<int32_t> sel;                    // the running slots dCol stands for (empty: none yet)
    void release() { dRec.release(); dRaw.release(); dCol.release(); hCol.release(); }
};

// fot_loop_scores_enable: a resident sampler loop scores its predictor (fot_loopscore.hpp).  The representative sample's
// error rows go through LoopSummaryAcc's ring (armed, but not `on`: fot_loop_summaries stays refused); the per-origin
// records of a step land in hRec and wait in each slot's ring of H = stride * pred_len records for their horizon.
struct LoopScores {
    bool on = false;
    int stride = 0, H = 0;
    bool std_ok = false;                         // stride * pred_len - 1 < n_dense: the standard metrics apply at all
    DevBuf dBest, dDev, dTruth;                  // int32[slots] | [slots][best_dev_stride(S)] deviation sums | [cols][pred_len][2]
    PinnedBuf hBest, hDesc, hRec;                // int32[slots] | PredOriginDev[slots] | fot_pred_score[slots] of the step
    std::vector<PredScoreTerms> ring;            // [slots][H]
    std::vector<ScoreFold> fold;                 // [slots]
    std::vector<int32_t> last_best;              // [slots] of the most recent lock step
    void release() { dBest.release(); dDev.release(); dTruth.release(); hBest.release(); hDesc.release(); hRec.release(); }
};

// fot_loop_set_replay / fot_loop_run: the recording (host copy for the prepend test, HBM copy for the frame kernel), the
// replay clock and what a resident step keeps on the device
struct LoopReplay {
    bool set = false;
    fot_loop_replay cfg = fot_loop_replay();     // the constants (its pointers are cleared)
    int n_cols = 0, n_dense = 0, max_lvl = 1;
    std::vector<int32_t> ped_off, n_frames;      // per slot
    std::vector<double> pos, vel;                // [n_frames_max][n_cols][2]
    ReplayClock clock;
    std::vector<uint8_t> alive;
    std::vector<int32_t> steps, termination;
    DevBuf dPos, dVel, dTab;                     // the recording; slot_ped0 | slot_frames
    DevBuf dFrame;                               // the step's compacted frame (FrameDev)
    DevBuf dRec, dHist;                          // the step's records; followed paths of the call's steps
    PinnedBuf hStage, hDigest, hHistTab, hWord;  // FrameStage | LoopDigest[] | followed record + slot | completion words
    int32_t seq = 0;                             // value the completion words are raised to next
    LoopSummaryAcc sum;
    LoopSampler smp;
    LoopSamples rec;                             // (sampler and recording exclude each other)
    LoopScores sc;
    int dist_S() const { return smp.on ? smp.S : rec.on ? rec.S : 0; }   // samples of a predicting step's distribution
    void release()
    {
        sum.release(); smp.release(); rec.release(); sc.release();
        dPos.release(); dVel.release(); dTab.release(); dFrame.release(); dRec.release(); dHist.release();
        hStage.release(); hDigest.release(); hHistTab.release(); hWord.release();
    }
};

// fot_loop_plan_sample: the requests plan against every episode's representative sample (fot_repsample.hpp).  Nothing
// here is allocated before the mode is switched on; the tables grow with the loop's frames as dDyn does.
struct LoopRep {
    int mode = 0;                                // FOT_LOOP_PLAN_*
    bool frame = false;                          // the most recent frame left planning blocks in dBlk (it carried a distribution)
    int T = 0;                                   // their time entries: n_dense + 1
    DevBuf dBlk, dBest, dDev, dPre;              // [rows][T][2] | int32[slots] | [slots][best_dev_stride(S)] | int32[episodes]
    PinnedBuf hBest, hPre;                       // int32[slots] | int32[episodes of the frame]
    std::vector<int32_t> last_best;              // [slots of fot_loop_begin] of the most recent lock step
    std::vector<int32_t> run_best;               // [steps][slots] of the most recent fot_loop_run call (fot_loop_run_best_samples)
    void release() { dBlk.release(); dBest.release(); dDev.release(); dPre.release(); hBest.release(); hPre.release(); }
};

// fot_loop_footprint_enable: the observational footprint metrics of a loop (fot_footprint_obs.hpp).  The geometry where
// k_footprint_steps reads it, the records of a lock step's new ego states in pinned memory (sized for the loop's slots at
// the enable call: it never grows inside a run) and the per-slot accumulators the host folds them into
struct LoopFootprintObs {
    bool on = false;
    FpoGeom geom = FpoGeom();
    PinnedBuf hGeom, hRec;                       // FpoGeom | FpoStep[slots]
    std::vector<FpoAcc> acc;                     // [slots]
    std::vector<int32_t> steps;                  // [slots] lock steps folded
    void release() { hGeom.release(); hRec.release(); }
};

// fot_loop_*: what one closed-loop step leaves behind for the step's later calls
struct LoopState {
    LoopEpisodes ep;
    LoopFootprintObs fpo;
    bool stepped = false;                    // a lock step has run since fot_loop_begin* (fot_loop_step or fot_loop_run)
    LoopReplay replay;
    LoopRep rep;
    PinnedBuf hFrame, hObserve, hOut, hRec;  // frame inputs | fot_loop_observe's inputs | small outputs | records
    DevBuf dDyn, dStatic;                    // the prediction tensor; the static points, one copy per request
    std::vector<double> static_xy;           // host copy of the static points
    int static_tiles = 0;                    // copies resident in dStatic
    // a scenario loop: every scenario's points once in HBM (dScenStatic, scenario s at point scen_static_off[s]); a
    // step's per-request blocks are gathered from them on the device (k_static_gather) into dGather
    std::vector<std::vector<double>> scen_static;    // [scenario] host copies (fot_loop_set_scenario_static)
    std::vector<int32_t> scen_static_off;    // [scenarios + 1] as resident in dScenStatic
    bool scen_static_dirty = true;
    DevBuf dScenStatic, dGather, dSafScen;   // ... ; SafetyScen[scenarios]
    PinnedBuf hGather;                       // StaticGather[requests] of the plan call being enqueued
    std::vector<int32_t> frame_scen;         // scenario of each episode of the frame (empty: all on scenario 0)
    // a sweep loop's frame that carried a distribution (fot_sweep.hpp): the planning blocks of its representative-mode
    // episodes lie in dDyn behind the distribution blocks.  Empty: no such frame.  hSweep: the table where a resident
    // step's kernels read it.
    std::vector<SweepEp> sweep_tab;
    int sweep_T = 0;
    PinnedBuf hSweep;
    // fot_loop_set_slot_samples: slot e of a sweep loop uses the first slot_S[e] samples of its source (empty: every slot
    // uses them all).  ep_S: the counts of the episodes of the most recent frame that carried a distribution (empty: it
    // carried none, or the loop has no counts), hEpS: the same where a resident step's kernels read them.
    std::vector<int32_t> slot_S, ep_S;
    PinnedBuf hEpS;
    int count_of(size_t episode) const { return ep_S.empty() ? dist_S : ep_S[episode]; }   // samples of a frame's episode
    const int32_t *p_scen = nullptr;         // the same where k_safety reads it (beside p_off), or nullptr
    std::vector<int32_t> ped_off;            // of the frame
    std::vector<int64_t> blk_off;            // first point of each episode's block in the tensor
    std::vector<int32_t> t_len;              // samples per track of each episode's block
    int dist_S = 0;                          // > 0: the blocks are [dist_S][P_e][t_len][2] distributions
    bool have_frame = false;
    const void *dyn_ptr = nullptr;           // the tensor: dDyn, or the pinned current positions (predictor not ready)
    const int32_t *p_off = nullptr;          // the frame's pedestrians in hFrame (a resident step: in HBM, LoopReplay::dFrame)
    const double *p_pos = nullptr, *p_vel = nullptr;
    double ego_radius = 0.0, ped_radius = 0.0;
    int use_footprint = 0;
    int observe_n = -1;                      // egos of a fot_loop_observe_begin not collected yet
    void release()
    {
        hFrame.release(); hObserve.release(); hOut.release(); hRec.release();
        dDyn.release(); dStatic.release(); replay.release(); rep.release();
        dScenStatic.release(); dGather.release(); dSafScen.release(); hGather.release();
        hSweep.release(); hEpS.release(); fpo.release();
    }
};

// One planner configuration + reference path of a handle (a reference FrenetPlanner object); scenario 0 is the handle's own.
struct Scenario {
    fot_params params = fot_params();
    DevParams P;                             // (element `id` of the handle's DevParams table in HBM)
    HostSpline spline;
    DevBuf dSpline;                          // its 9 coefficient arrays (element `id` of the SplineView table)
    bool has_path = false;
    bool flat_path = false;                  // the path is exactly straight (spline_is_flat): decided where it is set
    TileShapes shapes;                       // its run of the handle's tile table ...
    int32_t shape_base = 0;                  // ... starting at this entry
};

constexpr int FOT_LANES = 4;                  // lanes available; lanes_cfg of them are used (FOT_LANES env, default 1)
constexpr int FOT_SPLIT_MIN_INSTANCES = 32;  // smaller batches run as one piece on the caller's stream

struct fot_handle {
    int device = 0;
    hipStream_t stream = nullptr;            // the handle's own stream (host-pointer entry points, helpers)
    hipEvent_t fork = nullptr;               // caller's stream -> lanes
    // One handle = ONE workspace and one set of scratch buffers, so its enqueues are ordered whatever streams the
    // caller passes: an enqueue on a stream other than the previous one first waits (device side) for the event
    // recorded behind the previous enqueue.  Work of different handles still overlaps freely.
    hipEvent_t order_done = nullptr;
    hipStream_t order_stream = nullptr;
    bool order_valid = false;
    int eval_segments = 0;               // fot_debug_set_eval_segments
    // Completion of a synchronous small call without a stream synchronisation: the wave that writes a record (into
    // pinned memory) raises that record's flag to the call's sequence number behind a system-scope release; the host
    // polls the flags.  hipStreamSynchronize returns some 10 us after the last kernel ended on this platform -- a sixth
    // of a one-ego plan call.
    PinnedBuf hDone;
    int32_t done_seq = 0;
    bool done_seq_armed = false;             // the call being enqueued wants the flags
    int tile_cut = 0;                    // fot_debug_set_tile_cut (TILE_CUT_*)
    int eval_form = 0;                   // fot_debug_set_eval_form: 0 = by eligibility, 1 = the general form always
    int last_eval_forms = 0;             // forms the launches of the most recent plan call took: 1 general | 2 lean
                                         // | 4 general, wide | 8 lean, wide
    int sample_cap = FOT_MAX_SAMPLES;    // fot_set_sample_capacity: most samples of a distribution any entry accepts
    int flat_mode = 1;                   // fot_debug_set_flat: 1 = flat kernels where a launch is eligible, 0 = never
    int last_flat = 0;                   // 1: a launch of the most recent plan call took a flat kernel
    std::vector<Scenario> sc;                // scenarios; sc[0]: fot_create's params + fot_set_path_*
    std::vector<ScenarioRef> refs;           // what build_batch_layout needs of each (rebuilt with the tile table)
    DevBuf dP;                               // DevParams[sc.size()]
    DevBuf dSplineTab;                       // SplineView[sc.size()]
    int32_t n_shape_entries = 0;             // entries of the concatenated tile table ...
    DevBuf dShapes;                          // ... in HBM: cand0[] | n[] | span[]
    int head_tmpl_entries = 0;               // entries per variant of the header templates (0: no grouped cut) ...
    DevBuf dHeadTmpl;                        // ... in HBM: HeadTemplate[HEAD_VARIANTS][head_tmpl_entries]
    Workspace ws[FOT_LANES];
    int lanes_cfg = 1;                       // sub-batches a large batch is split into
    int lanes_used = 0;                      // lanes of the most recent plan call
    DevBuf dUserStatic, dUserDyn, dOut;      // device copies for the host-pointer entry point
    PinnedBuf hSmallIn, hSmallOut;           // ... and, for small calls, pinned host blocks the kernels use directly
    PinnedBuf hRecOut;                       // ... the records of a small plan call (a block of its own: zero past n_total)
    PinnedBuf hScoreIn, hScoreOut;           // fot_prediction_scores: PredOriginDev[] | truth; the records the kernel writes
    DevBuf dScoreT;                          // ... the device copy of a host tensor
    DevBuf dTmpA, dTmpB, dTmpC, dTmpD;
    // fot_openloop_eval: the scene's copy and the call's tables in HBM, the work arrays of a chunk (sized by max_rows,
    // grow-only), the tables as the host builds them and the records the scorer writes
    struct OpenLoop {
        DevBuf dScene, dTab, dNoiseAll;          // a host scene | the call's tables (hTab) | a host noise tensor
        DevBuf dObs, dAnchor, dTruth, dNoise, dRaw, dDyn;
        PinnedBuf hTab, hRec;
        void release()
        {
            for (DevBuf *b : { &dScene, &dTab, &dNoiseAll, &dObs, &dAnchor, &dTruth, &dNoise, &dRaw, &dDyn }) b->release();
            hTab.release(); hRec.release();
        }
    } ol;
    // fot_footprint_recheck: the inputs of a large call, the reconstructed headings, the steps' records and the
    // trajectories' records in HBM (grow-only)
    struct Footprint {
        DevBuf dIn, dYaw, dSeries, dOut;
        void release() { dIn.release(); dYaw.release(); dSeries.release(); dOut.release(); }
    } fp;
    // fot_fidelity_eval: the tables and the encounters' arrays, and everything the kernels write, in HBM (grow-only)
    struct Fidelity {
        DevBuf dIn, dOut;
        void release() { dIn.release(); dOut.release(); }
    } fid;
    // fot_encounters_extract: a host clip's copy, the ego rows and the tables, the columns' and spans' work arrays, the
    // packed encounters with what launch_fidelity writes, the speeds and the per-row outputs, in HBM (grow-only)
    struct Encounters {
        DevBuf dScene, dIn, dWork, dTab, dPacked, dSpeeds, dOut;
        void release() { for (DevBuf *b : { &dScene, &dIn, &dWork, &dTab, &dPacked, &dSpeeds, &dOut }) b->release(); }
    } enc;
    LoopState loop;
    // fot_sgan_*: the loaded models (descriptor, device image of the weights), each with the work arrays of its own sample
    // calls -- what model m computes never depends on what else is loaded or was sampled in between
    struct Sgan {
        bool loaded = false;
        fot_sgan_desc desc{};
        SgDev dev{};
        DevBuf dImg, dOff, dScene, dObs, dNoise, dOut, dHenc, dPool, dCtx, dH, dC, dXY;
        PinnedBuf hTab;                          // fot_sgan_noise: the row tables the kernel reads
        void release()
        {
            for (DevBuf *b : { &dImg, &dOff, &dScene, &dObs, &dNoise, &dOut, &dHenc, &dPool, &dCtx, &dH, &dC, &dXY }) b->release();
            hTab.release();
        }
    } sgan[SGAN_MAX_MODELS];
    bool last_valid = false;
    // profiling: event pairs around kernel launches
    bool prof_on = false;
    std::vector<hipEvent_t> prof_pool;       // all events ever created
    size_t prof_used = 0;                    // events handed out since the last read
    std::vector<int> prof_kernel;            // kernel id of pair i (events 2i, 2i+1)
    int32_t prof_launches[FOT_PROFILE_KERNELS] = { 0 };
    double prof_ms[FOT_PROFILE_KERNELS] = { 0 };
    std::string err;
};

namespace fot { namespace host __attribute__((visibility("hidden"))) {

// ---- defined in fot_host.cpp
int fail(fot_handle *h, int code, const std::string &msg);       // (h == nullptr: the error of fot_create / of a call without a handle)
int hip_fail(fot_handle *h, hipError_t e, const char *what);

#define HIP_TRY(h, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hip_fail((h), e_, #expr); } while (0)
#define LAUNCH_TRY(h, expr) do { int r_ = (expr); if (r_ != 0) return hip_fail((h), (hipError_t)r_, #expr); } while (0)

int order_begin(fot_handle *h, hipStream_t st);                  // see fot_handle::order_done
int order_end(fot_handle *h, hipStream_t st);
SplineView spline_view(const fot_handle *h, int scen = 0);
int check_scenarios(fot_handle *h, const fot_batch &b, const int32_t *scen);
int enqueue_plan(fot_handle *h, const fot_batch &b, const int32_t *scen, const void *d_static, const void *d_dyn,
                 fot_result *d_out, hipStream_t user, bool sync_caller = false, void *d_dyn_stage = nullptr);
bool arm_records(fot_handle *h, int n);
int wait_records(fot_handle *h, int n, hipStream_t st);

// ---- defined in fot_host_pred.cpp
int sgan_enqueue(fot_handle *h, int model, int n_scenes, int N, int S, const int32_t *d_off, const int32_t *d_scene,
                 const float *d_obs, const float *d_noise, float *d_out, hipStream_t st);

// brackets one launch with events when profiling is on
struct ProfScope {
    fot_handle *h; hipStream_t st; hipEvent_t stop = nullptr; bool active = false;
    ProfScope(fot_handle *h_, int kernel, hipStream_t st_) : h(h_), st(st_)
    {
        if (!h->prof_on) return;
        while (h->prof_pool.size() < h->prof_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            h->prof_pool.push_back(e);
        }
        hipEvent_t start = h->prof_pool[h->prof_used];
        stop = h->prof_pool[h->prof_used + 1];
        if (hipEventRecord(start, st) != hipSuccess) return;
        h->prof_used += 2;
        h->prof_kernel.push_back(kernel);
        active = true;
    }
    ~ProfScope() { if (active) (void)hipEventRecord(stop, st); }
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// The refusal of every entry that takes a sample distribution (prediction, samplers, scores, the loop's frames): S lies
// above the handle's sample capacity.  who: the entry's name with its separator.  Changes nothing but the error text.
inline int refuse_samples(fot_handle *h, const std::string &who, int S)
{
    return fail(h, FOT_ERR_UNSUPPORTED, who + "S > " + (h->sample_cap == FOT_MAX_SAMPLES ? "FOT_MAX_SAMPLES" : "the handle's raised sample capacity") +
                                        " (" + std::to_string(S) + " samples, the handle's sample capacity is " + std::to_string(h->sample_cap) +
                                        "; fot_set_sample_capacity raises it up to " + std::to_string(FOT_MAX_PLAN_SAMPLES) + ")");
}

// Calls whose inputs and outputs stay below this size skip the copy operations: the kernels read / write pinned host
// memory directly (fot_plan_batch, fot_safety_metrics_batch, fot_frenet_state_batch, the host path of the resampler).
constexpr size_t SMALL_CALL_BYTES = (size_t)1 << 20;

// The wait under wait_records (fot_host.cpp) and the resident loop's wait_word (fot_host_loop.cpp).
// Spins until the n consecutive words from `word` on have all been raised to seq (by kernels, in pinned memory); true:
// they have, and what was written ahead of them is visible.  false: 20 ms have passed without them (a kernel that
// faulted, a path that raises none) -- the caller synchronises its stream instead.
inline bool spin_words(const int32_t *word, int n, int32_t seq)
{
    volatile const int32_t *w = (volatile const int32_t *)word;
    const auto t0 = std::chrono::steady_clock::now();
    int i = 0, spins = 0;
    while (i < n) {
        if (w[i] == seq) { ++i; continue; }
        __builtin_ia32_pause();
        if ((++spins & 1023) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.02) return false;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return true;
}

}}  // namespace fot::host
