// fot_host.cpp -- the C ABI of libfot.so (include/fot.h): handle, device workspace, batch staging.
// No torch, no oracle, no CPU fallback: every entry point drives the gfx950 kernels or fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "fot_kernels.h"
#include "fot_loop_kernels.h"
#include "fot_math.hpp"
#include "fot_replay.hpp"
#include "fot_summary.hpp"
#include "fot_loopscore.hpp"
#include "fot_setup.hpp"
#include "fot_sgan.h"

using namespace fot;

namespace {

thread_local std::string g_create_error;

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

}  // namespace

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

// fot_loop_set_sampler: the resident loop's Social-GAN predictor -- the window, the noise and the raw samples of a step in
// HBM, the noise kernel's row tables in pinned memory
struct LoopSampler {
    bool on = false;
    int S = 0, kind = 0;
    uint64_t seed = 0;
    DevBuf dWin, dNoise, dRaw;                   // [obs_len][rows][2] | [S][noise rows][nd] | [S][pred_len][rows][2], float32
    PinnedBuf hTab;                              // slot | step | index, n_cols + n_slots entries each
    void release() { dWin.release(); dNoise.release(); dRaw.release(); hTab.release(); }
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
    DevBuf dBest, dDev, dTruth;                  // int32[slots] | [slots][FOT_MAX_SAMPLES] deviation sums | [cols][pred_len][2]
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
    DevBuf dBlk, dBest, dDev, dPre;              // [rows][T][2] | int32[slots] | [slots][FOT_MAX_SAMPLES] | int32[episodes]
    PinnedBuf hBest, hPre;                       // int32[slots] | int32[episodes of the frame]
    std::vector<int32_t> last_best;              // [slots of fot_loop_begin] of the most recent lock step
    std::vector<int32_t> run_best;               // [steps][slots] of the most recent fot_loop_run call (fot_loop_run_best_samples)
    void release() { dBlk.release(); dBest.release(); dDev.release(); dPre.release(); hBest.release(); hPre.release(); }
};

// fot_loop_*: what one closed-loop step leaves behind for the step's later calls
struct LoopState {
    LoopEpisodes ep;
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
    }
};

// One planner configuration + reference path of a handle (a reference FrenetPlanner object); scenario 0 is the handle's own.
struct Scenario {
    fot_params params = fot_params();
    DevParams P;                             // (element `id` of the handle's DevParams table in HBM)
    HostSpline spline;
    DevBuf dSpline;                          // its 9 coefficient arrays (element `id` of the SplineView table)
    bool has_path = false;
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
    LoopState loop;
    // fot_sgan_*: the loaded model (descriptor, device image of the weights) and the work arrays of a sample call
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
    } sgan;
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

namespace {

// Every handle fot_create returned and fot_destroy has not taken back: fot_destroy of anything else (a second destroy,
// a stale pointer) is a no-op instead of a double free, and a binding can ask how many it still owns (fot_live_handles).
std::mutex g_live_mu;
std::unordered_set<fot_handle *> &live_handles()
{
    static std::unordered_set<fot_handle *> *s = new std::unordered_set<fot_handle *>();   // (never destroyed: no static
    return *s;                                                                            //  destructor order to lose)
}

// Teardown never blocks for good.  Work the handle enqueued may sit on a CALLER's stream (fot_plan_batch_device on a
// PyTorch stream) whose owner is free to have destroyed it, and a destroy may run while the process is exiting: the
// handle's streams and its ordering event are POLLED (hipStreamQuery / hipEventQuery) for a bounded time; if they do
// not drain, or the runtime answers with an error, the device and pinned memory is left to the process teardown
// instead of being freed under work that may still touch it.
double destroy_timeout_s()
{
    if (const char *ev = std::getenv("FOT_DESTROY_TIMEOUT_MS")) { const double v = std::atof(ev); if (v >= 0.0) return v * 1e-3; }
    return 5.0;
}

void destroy_handle(fot_handle *h);           // (below fot_create: frees what a handle owns, registered or not)

template <class Query>
bool drained(const Query &query, double seconds)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = query();
        if (e == hipSuccess) return true;
        if (e != hipErrorNotReady) { (void)hipGetLastError(); return false; }   // stream / context gone: nothing to wait for, nothing to free
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

int fail(fot_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

int hip_fail(fot_handle *h, hipError_t e, const char *what)
{
    return fail(h, FOT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(h, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hip_fail((h), e_, #expr); } while (0)
#define LAUNCH_TRY(h, expr) do { int r_ = (expr); if (r_ != 0) return hip_fail((h), (hipError_t)r_, #expr); } while (0)

// see fot_handle::order_done
int order_begin(fot_handle *h, hipStream_t st)
{
    if (h->order_valid && st != h->order_stream) HIP_TRY(h, hipStreamWaitEvent(st, h->order_done, 0));
    return FOT_OK;
}

int order_end(fot_handle *h, hipStream_t st)
{
    HIP_TRY(h, hipEventRecord(h->order_done, st));
    h->order_stream = st;
    h->order_valid = true;
    return FOT_OK;
}

SplineView spline_view(const fot_handle *h, int scen = 0)
{
    SplineView v;
    const double *b = h->sc[(size_t)scen].dSpline.as<double>();
    const int n = h->sc[(size_t)scen].spline.n;
    v.s = b; v.ax = b + n; v.bx = b + 2 * n; v.cx = b + 3 * n; v.dx = b + 4 * n;
    v.ay = b + 5 * n; v.by = b + 6 * n; v.cy = b + 7 * n; v.dy = b + 8 * n;
    v.n = n; v._pad = 0;
    return v;
}

// the SplineView of every scenario, in HBM (a scenario without a path yet: an empty view no batch can reach)
int upload_spline_table(fot_handle *h)
{
    std::vector<SplineView> tab(h->sc.size());
    for (size_t s = 0; s < h->sc.size(); ++s) tab[s] = spline_view(h, (int)s);
    HIP_TRY(h, h->dSplineTab.ensure(sizeof(SplineView) * tab.size()));
    HIP_TRY(h, hipMemcpy(h->dSplineTab.p, tab.data(), sizeof(SplineView) * tab.size(), hipMemcpyHostToDevice));
    return FOT_OK;
}

// scenario `scen`'s spline into HBM (its coefficient arrays and its entry of the SplineView table)
int upload_spline(fot_handle *h, int scen = 0)
{
    Scenario &S = h->sc[(size_t)scen];
    const int n = S.spline.n;
    std::vector<double> flat((size_t)9 * n, 0.0);
    const std::vector<double> *src[9] = { &S.spline.s, &S.spline.ax, &S.spline.bx, &S.spline.cx, &S.spline.dx,
                                          &S.spline.ay, &S.spline.by, &S.spline.cy, &S.spline.dy };
    for (int f = 0; f < 9; ++f)
        std::memcpy(flat.data() + (size_t)f * n, src[f]->data(), sizeof(double) * std::min((size_t)n, src[f]->size()));
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // nothing may still be reading the old spline
    HIP_TRY(h, S.dSpline.ensure(flat.size() * sizeof(double)));
    HIP_TRY(h, hipMemcpy(S.dSpline.p, flat.data(), flat.size() * sizeof(double), hipMemcpyHostToDevice));
    { int r = upload_spline_table(h); if (r != FOT_OK) return r; }
    S.has_path = true;
    h->last_valid = false;
    return FOT_OK;
}

// the DevParams of every scenario, element s = scenario s, into HBM
int upload_params(fot_handle *h)
{
    std::vector<DevParams> tab(h->sc.size());
    for (size_t s = 0; s < h->sc.size(); ++s) tab[s] = h->sc[s].P;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // nothing may still be reading the old table
    HIP_TRY(h, h->dP.ensure(sizeof(DevParams) * tab.size()));
    HIP_TRY(h, hipMemcpy(h->dP.p, tab.data(), sizeof(DevParams) * tab.size(), hipMemcpyHostToDevice));
    h->last_valid = false;
    return FOT_OK;
}

// (re)builds the tile tables of all scenarios for the given cut (one cut per handle) and puts their concatenation into
// HBM: cand0[] | n[] | span[]; with them the group-header templates of a grouped cut, which are a function of the table
int upload_tile_shapes(fot_handle *h, int cut)
{
    const size_t n_sc = h->sc.size();
    std::vector<const DevParams *> ps(n_sc);
    std::vector<TileShapes> shapes(n_sc);
    for (size_t s = 0; s < n_sc; ++s) ps[s] = &h->sc[s].P;
    build_tile_shapes(ps.data(), (int)n_sc, shapes.data(), cut);
    std::vector<int32_t> cand0, nn, span;
    for (size_t s = 0; s < n_sc; ++s) {
        h->sc[s].shape_base = (int32_t)cand0.size();
        cand0.insert(cand0.end(), shapes[s].cand0.begin(), shapes[s].cand0.end());
        nn.insert(nn.end(), shapes[s].n.begin(), shapes[s].n.end());
        span.insert(span.end(), shapes[s].span.begin(), shapes[s].span.end());
        h->sc[s].shapes = std::move(shapes[s]);
    }
    h->refs.assign(n_sc, ScenarioRef());
    for (size_t s = 0; s < n_sc; ++s) {
        h->refs[s].hp = &h->sc[s].params; h->refs[s].P = &h->sc[s].P;
        h->refs[s].shapes = &h->sc[s].shapes; h->refs[s].shape_base = h->sc[s].shape_base;
    }
    h->tile_cut = cut;
    std::vector<HeadTemplate> tmpl;
    h->head_tmpl_entries = head_template_entries(h->refs.data(), (int)n_sc);
    if (h->head_tmpl_entries > 0)
        build_head_templates(h->refs.data(), (int)n_sc, cand0.data(), nn.data(), h->head_tmpl_entries, tmpl);
    const size_t nt = cand0.size();
    h->n_shape_entries = (int32_t)nt;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // nothing may still be reading the old table
    HIP_TRY(h, h->dShapes.ensure(sizeof(int32_t) * 3 * std::max<size_t>(nt, 1)));
    if (nt) {
        HIP_TRY(h, hipMemcpy(h->dShapes.p, cand0.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->dShapes.as<int32_t>() + nt, nn.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->dShapes.as<int32_t>() + 2 * nt, span.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
    }
    if (!tmpl.empty()) {
        HIP_TRY(h, h->dHeadTmpl.ensure(sizeof(HeadTemplate) * tmpl.size()));
        HIP_TRY(h, hipMemcpy(h->dHeadTmpl.p, tmpl.data(), sizeof(HeadTemplate) * tmpl.size(), hipMemcpyHostToDevice));
    }
    h->last_valid = false;
    return FOT_OK;
}

// The scenarios a batch's instances name: known ids with a path, chains on one scenario (scen NULL: scenario 0)
int check_scenarios(fot_handle *h, const fot_batch &b, const int32_t *scen)
{
    const int n_inst = b.n_inst;
    if (!scen) return h->sc[0].has_path ? FOT_OK : fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    for (int i = 0; i < n_inst; ++i) {
        if (scen[i] < 0 || scen[i] >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
        if (!h->sc[(size_t)scen[i]].has_path)
            return fail(h, FOT_ERR_NO_PATH_SET, "an instance's scenario has no path (fot_set_scenario_path_*)");
    }
    // (build_batch_layout refuses this too, lane by lane; checked here so that a refused call enqueues nothing)
    for (int i = 1; i < n_inst && b.ego; ++i)
        if (b.ego[i].has_prev_s == FOT_PREV_S_CHAINED && scen[i] != scen[i - 1])
            return fail(h, FOT_ERR_INVALID, "a chained instance must be on its predecessor's scenario (a chain is one planner)");
    return FOT_OK;
    return FOT_OK;
}

// the paths of a batch laid out by L: its one scenario's in the kernel arguments, or the table of a mixed batch
PathSet path_set(const fot_handle *h, const BatchLayout &L, const DevParams **P_launch)
{
    const DevParams *dP = h->dP.as<DevParams>();
    if (L.scens.size() <= 1) {
        const int s = L.scens.empty() ? 0 : L.scens[0];
        *P_launch = dP + s;
        return PathSet::single(spline_view(h, s));
    }
    PathSet ps;
    ps.table = h->dSplineTab.as<SplineView>();
    ps.mixed = 1;
    for (int s : L.scens) ps.knots[ps.n_knots++] = h->sc[(size_t)s].spline.n;
    *P_launch = dP;
    return ps;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Calls whose inputs and outputs stay below this size skip the copy operations: the kernels read / write pinned host
// memory directly (fot_plan_batch, fot_safety_metrics_batch, fot_frenet_state_batch, the host path of the resampler).
constexpr size_t SMALL_CALL_BYTES = (size_t)1 << 20;

const char *const kKernelNames[FOT_PROFILE_KERNELS] = { "k_frenet_state", "k_cull", "k_evaluate" };

// accumulate finished event pairs into the per-kernel totals (waits for them)
int prof_drain(fot_handle *h)
{
    for (size_t i = 0; i < h->prof_kernel.size(); ++i) {
        hipEvent_t a = h->prof_pool[2 * i], b = h->prof_pool[2 * i + 1];
        HIP_TRY(h, hipEventSynchronize(b));
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, a, b));
        h->prof_launches[h->prof_kernel[i]] += 1;
        h->prof_ms[h->prof_kernel[i]] += (double)ms;
    }
    h->prof_kernel.clear();
    h->prof_used = 0;
    return FOT_OK;
}

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

// Stage descriptors, size the lane's workspace and enqueue the whole pipeline for the sub-batch `b` on `st`.
// d_static / d_dyn are device pointers to the caller's obstacle coordinates (offsets in b are absolute),
// d_out the device fot_result slot of the sub-batch's first instance.
// sync_caller: see enqueue_plan.
// d_dyn_stage: HBM block the NaN-scan blocks copy the dynamic tensors into as they read them (a small call's tensors
// lie in pinned host memory: the later kernels then read the copy instead of crossing PCIe again), or nullptr.
int enqueue_lane(fot_handle *h, Workspace &w, const fot_batch &b, const int32_t *scen, const void *d_static,
                 const void *d_dyn, fot_result *d_out, hipStream_t st, bool sync_caller = false, void *d_dyn_stage = nullptr)
{
    BatchLayout &L = w.last;
    std::string err;
    int rc = build_batch_layout(h->refs.data(), (int)h->refs.size(), scen, b, L, err);
    if (rc != FOT_OK) return fail(h, rc, err);
    if (L.n_inst == 0) return FOT_OK;

    // --- staging: the descriptors in a pinned block (k_frenet_state pulls them into HBM)
    const size_t desc_bytes = align256(sizeof(InstDesc) * (size_t)L.n_inst);
    const size_t meta_bytes = desc_bytes;
    const int slot = (w.staging_slot ^= 1);
    if (w.staging_pending[slot]) { HIP_TRY(h, hipEventSynchronize(w.staging_done[slot])); w.staging_pending[slot] = false; }
    HIP_TRY(h, w.staging[slot].ensure(desc_bytes));
    char *stg = (char *)w.staging[slot].p;
    std::memcpy(stg, L.desc.data(), sizeof(InstDesc) * (size_t)L.n_inst);

    // --- workspace (grow-only; a growing hipFree/hipMalloc synchronises, steady state does not)
    const DevParams &P = h->sc[0].P;                             // (n_total: the same in every scenario)
    HIP_TRY(h, w.dMeta.ensure(meta_bytes));
    HIP_TRY(h, w.dState.ensure(sizeof(InstState) * (size_t)L.n_inst));
    const size_t slots = (size_t)std::max<int64_t>(L.n_slots, 1);
    HIP_TRY(h, w.dCost.ensure(sizeof(double) * slots));
    HIP_TRY(h, w.dParts.ensure(sizeof(TilePart) * (size_t)std::max(L.n_tiles, 1)));
    HIP_TRY(h, w.dStatus.ensure(slots));
    HIP_TRY(h, w.dKeep.ensure(sizeof(uint16_t) * slots));
    const size_t n_ent = (size_t)L.n_entries + 64;              // slack: the scalar prefetch reads one chunk ahead
    HIP_TRY(h, w.dEntCnt.ensure(sizeof(int32_t) * (size_t)P.n_total * (size_t)L.n_inst));
    HIP_TRY(h, w.dEnt32.ensure(sizeof(f2) * n_ent));
    HIP_TRY(h, w.dEnt64.ensure(sizeof(d2) * n_ent));
    HIP_TRY(h, w.dEntSid.ensure(n_ent));
    HIP_TRY(h, w.dWaveRng.ensure(sizeof(TileStep) * (size_t)P.n_total * (size_t)std::max(L.n_tiles, 1)));
    HIP_TRY(h, w.dNanFlag.ensure((size_t)std::max<int64_t>(L.n_tracks, 16)));
    HIP_TRY(h, w.dDone.ensure(sizeof(int32_t) * (size_t)L.n_inst));

    // no H2D copy in front of the kernels: k_frenet_state pulls the staging block into HBM (one dependent hop less)
    w.staging_pending[slot] = true;

    const InstDesc *d_desc = (const InstDesc *)w.dMeta.p;
    TileTable tt;
    tt.cand0 = h->dShapes.as<int32_t>();
    tt.n = h->dShapes.as<int32_t>() + h->n_shape_entries;
    tt.span = h->dShapes.as<int32_t>() + 2 * (size_t)h->n_shape_entries;
    tt.n_tiles = L.n_tiles; tt.max_tiles = L.max_tiles; tt.row_budget = L.row_budget;
    tt.eval_segments = h->eval_segments;
    tt.grouped = L.grouped;
    // The lean evaluation kernels (FusedSink<true>): at most 64 samples per candidate and the single centre circle in
    // every scenario of the handle, no chance budget on any instance of this launch.  Anything else: the general form.
    tt.lean = h->eval_form == 0 ? 1 : 0;
    for (const Scenario &S : h->sc) if (S.P.n_total > WAVE || S.P.has_footprint) tt.lean = 0;
    for (int i = 0; i < L.n_inst && tt.lean; ++i) if (L.desc[(size_t)i].max_viol != 0) tt.lean = 0;
    h->last_eval_forms |= tt.lean ? 2 : 1;
    GroupHeadOut gh;                                             // the grouped kernels' headers: k_frenet_state builds them
    if (evaluate_in_groups(tt)) {
        gh.n_pos = L.max_tiles / GROUP_TILES;
        HIP_TRY(h, w.dHeads.ensure(sizeof(GroupHead) * (size_t)L.n_inst * (size_t)gh.n_pos));
        gh.heads = tt.heads = w.dHeads.as<GroupHead>();
        gh.tmpl = h->dHeadTmpl.as<HeadTemplate>(); gh.tmpl_entries = h->head_tmpl_entries;
        if (gh.tmpl_entries < 1) return fail(h, FOT_ERR_INVALID, "plan: no header templates for this handle's tile table");
    }
    const DevParams *dP = nullptr;
    const PathSet sv = path_set(h, L, &dP);
    CandArrays ca;
    ca.cost = w.dCost.as<double>(); ca.parts = w.dParts.as<TilePart>();
    ca.status = w.dStatus.as<uint8_t>(); ca.keep = w.dKeep.as<uint16_t>();
    if (sync_caller && h->done_seq_armed) { ca.done_flag = (int32_t *)h->hDone.p; ca.done_seq = h->done_seq; }

    EntryArrays ea;
    ea.cnt = w.dEntCnt.as<int32_t>(); ea.e32 = w.dEnt32.as<f2>(); ea.e64 = w.dEnt64.as<d2>();
    ea.sid = w.dEntSid.as<uint8_t>(); ea.rng = w.dWaveRng.as<TileStep>();
    ea.nan_flag = w.dNanFlag.as<uint8_t>();
    MetaImport imp;
    imp.h_desc = (const InstDesc *)stg;
    imp.d_desc = (InstDesc *)w.dMeta.p;
    // one scan block per 256 KB of an instance's tensor (few, fat blocks: each first reads its descriptor out of the
    // pinned staging block, a PCIe round trip), at most 64 per instance
    // Only time-major tensors are scanned (k_cull finds the NaN tracks of the caller's [S][P][T] layout itself, among the
    // few its boxes touch); a small call's tensors in pinned memory take the same blocks for their one pass over PCIe.
    // (FOT_NAN_SCAN=eager: the scan blocks for every layout, as before round 4 -- the scan then doubles as a prefetch of
    // the tensor into the memory-side cache: 4 us less on the serial step of config 4, the same step with three calls in
    // flight, the tensor read twice.  A small call's staging pass leaves the flags behind anyway: k_cull uses them.)
    static const bool eager_env = getenv("FOT_NAN_SCAN") && !std::strcmp(getenv("FOT_NAN_SCAN"), "eager");
    const bool eager_nan = eager_env || d_dyn_stage != nullptr;
    ea.eager_nan = eager_nan ? 1 : 0;
    NanScan scan;
    scan.eager = ea.eager_nan;
    if (L.n_tracks > 0 && (L.any_tmajor || eager_nan)) {
        scan.dyn_xy = d_dyn; scan.dtype = b.obstacle_dtype; scan.flag = w.dNanFlag.as<uint8_t>();
        scan.blocks_per_inst = (int)std::min<int64_t>(64, std::max<int64_t>(1, (L.max_dyn_bytes + 262143) / 262144));
        if (d_dyn_stage) {                                       // (cull and the rest read the copy)
            scan.stage = d_dyn_stage; d_dyn = d_dyn_stage;
            // across PCIe a block moves 64 KB per round trip: one block per 64 KB, so that the copy is done well inside
            // the nearest-point chain it runs beside
            scan.blocks_per_inst = (int)std::min<int64_t>(64, std::max<int64_t>(1, (L.max_dyn_bytes + 65535) / 65536));
        }
    }
    {
        ProfScope ps(h, 0, st);
        LAUNCH_TRY(h, launch_frenet_state(dP, sv, d_desc, w.dState.as<InstState>(), L.n_inst, imp, scan, w.dDone.as<int32_t>(), st, gh));
    }
    if (L.any_obstacles) {
        ProfScope ps(h, 1, st);
        LAUNCH_TRY(h, launch_cull(dP, d_desc, w.dState.as<InstState>(), L.n_inst, P.n_total, L.n_ext, sv,
                                  d_static, d_dyn, b.obstacle_dtype, ea, tt, st));
    }
    {
        ProfScope ps(h, 2, st);
        LAUNCH_TRY(h, launch_evaluate(dP, sv, d_desc, w.dState.as<InstState>(), P.n_total, L.n_inst, tt, ea, ca, d_out,
                                      w.dDone.as<int32_t>(), st));
    }
    HIP_TRY(h, hipEventRecord(w.staging_done[slot], st));        // (behind the call: see Workspace::staging_done)
    return FOT_OK;
}

// sub-batch [i0, i0+n) of b: per-instance arrays shifted, obstacle offsets stay absolute
fot_batch sub_batch(const fot_batch &b, int i0, int n)
{
    fot_batch s = b;
    s.n_inst = n;
    s.ego = b.ego + i0;
    s.target_speed = b.target_speed + i0;
    s.overrides = b.overrides ? b.overrides + i0 : nullptr;
    s.max_stop_distance = b.max_stop_distance ? b.max_stop_distance + i0 : nullptr;
    s.static_off = b.static_off ? b.static_off + i0 : nullptr;
    s.dyn_off = b.dyn_off ? b.dyn_off + i0 : nullptr;
    s.dyn_dims = b.dyn_dims ? b.dyn_dims + 4 * (size_t)i0 : nullptr;
    return s;
}

// Enqueue one plan call behind everything already on `user`; small batches run on `user` itself, large ones
// fork into the lanes' streams and join `user` again.
// sync_caller: the caller waits for the records right behind this call (the synchronous entry points): the selecting
// waves then raise a flag per record in pinned memory (wait_records).
int enqueue_plan(fot_handle *h, const fot_batch &b, const int32_t *scen, const void *d_static, const void *d_dyn,
                 fot_result *d_out, hipStream_t user, bool sync_caller = false, void *d_dyn_stage = nullptr)
{
    if (b.n_inst < 0) return fail(h, FOT_ERR_INVALID, "n_inst < 0");
    { int r = check_scenarios(h, b, scen); if (r != FOT_OK) return r; }
    h->last_valid = false;
    h->last_eval_forms = 0;
    if (b.n_inst == 0) { h->lanes_used = 0; h->last_valid = true; return FOT_OK; }
    if (!d_out) return fail(h, FOT_ERR_INVALID, "out is NULL");
    if (!b.ego || !b.target_speed) return fail(h, FOT_ERR_INVALID, "ego / target_speed missing");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->prof_on && h->prof_kernel.size() > 16384) { int r = prof_drain(h); if (r != FOT_OK) return r; }
    { int r = order_begin(h, user); if (r != FOT_OK) return r; }

    if (b.n_inst < FOT_SPLIT_MIN_INSTANCES * h->lanes_cfg / 2 || h->lanes_cfg <= 1) {
        h->ws[0].first_inst = 0;
        int rc = enqueue_lane(h, h->ws[0], b, scen, d_static, d_dyn, d_out, user, sync_caller, d_dyn_stage);
        if (rc != FOT_OK) return rc;
        h->lanes_used = 1;
        h->last_valid = true;
        return order_end(h, user);
    }
    HIP_TRY(h, hipEventRecord(h->fork, user));
    int i0 = 0;
    const int lanes = h->lanes_cfg;
    for (int l = 0; l < lanes; ++l) {
        Workspace &w = h->ws[l];
        int n = b.n_inst / lanes + (l < b.n_inst % lanes ? 1 : 0);
        if (l == lanes - 1) n = b.n_inst - i0;
        while (i0 + n < b.n_inst && b.ego[i0 + n].has_prev_s == FOT_PREV_S_CHAINED) ++n;   // never cut a chain
        if (n > b.n_inst - i0) n = b.n_inst - i0;
        if (n <= 0) { w.last = BatchLayout(); w.first_inst = i0; continue; }
        HIP_TRY(h, hipStreamWaitEvent(w.stream, h->fork, 0));
        w.first_inst = i0;
        int rc = enqueue_lane(h, w, sub_batch(b, i0, n), scen ? scen + i0 : nullptr, d_static, d_dyn, d_out + i0, w.stream);
        if (rc != FOT_OK) return rc;
        HIP_TRY(h, hipEventRecord(w.done, w.stream));
        HIP_TRY(h, hipStreamWaitEvent(user, w.done, 0));
        i0 += n;
    }
    h->lanes_used = lanes;
    h->last_valid = true;
    return order_end(h, user);
}

// Arms the record flags for the next synchronous call of n records (false: this call waits on the stream instead).
bool arm_records(fot_handle *h, int n)
{
    h->done_seq_armed = false;
    static const bool off = std::getenv("FOT_NO_RECORD_FLAGS") != nullptr;       // diagnostics scripts
    if (off || h->prof_on || n <= 0 || n > 64) return false;
    // only the single-lane path hands the flags to its kernels (the predicate of enqueue_plan): a call the lanes split
    // would raise none, and wait_records would spin out its 20 ms before falling back to the stream
    if (h->lanes_cfg > 1 && n >= FOT_SPLIT_MIN_INSTANCES * h->lanes_cfg / 2) return false;
    if (h->hDone.ensure(sizeof(int32_t) * 64) != hipSuccess) return false;
    if (++h->done_seq == 0) {                                    // (wrapped: no stale flag may equal the new number)
        std::memset(h->hDone.p, 0, sizeof(int32_t) * 64);
        h->done_seq = 1;
    }
    h->done_seq_armed = true;
    return true;
}

// Waits until the n records of the call armed above are in pinned memory; after 20 ms without them (a kernel that
// faulted, a path that raises no flags) the stream is synchronised instead -- never a hang here that the stream
// synchronisation would not have been.
int wait_records(fot_handle *h, int n, hipStream_t st)
{
    const bool armed = h->done_seq_armed;
    h->done_seq_armed = false;
    if (armed) {
        volatile const int32_t *flag = (volatile const int32_t *)h->hDone.p;
        const auto t0 = std::chrono::steady_clock::now();
        int i = 0, spins = 0;
        while (i < n) {
            if (flag[i] == h->done_seq) { ++i; continue; }
            __builtin_ia32_pause();
            if ((++spins & 1023) == 0 &&
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.02) break;
        }
        if (i == n) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return FOT_OK;
        }
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

// lane and local index of global instance `inst` of the most recent plan call
Workspace *lane_of(fot_handle *h, int inst, int *local)
{
    for (int l = h->lanes_used - 1; l >= 0; --l)
        if (inst >= h->ws[l].first_inst && inst < h->ws[l].first_inst + h->ws[l].last.n_inst) {
            *local = inst - h->ws[l].first_inst;
            return &h->ws[l];
        }
    return nullptr;
}

}  // namespace

extern "C" {

const char *fot_version(void) { return "libfot 0.2 (gfx950, float64 lattice)"; }

int32_t fot_abi_info(int32_t cap, int32_t *out)
{
    const int32_t v[FOT_ABI_INFO_WORDS] = {
        FOT_ABI_VERSION,
        (int32_t)sizeof(fot_params), (int32_t)sizeof(fot_ego), (int32_t)sizeof(fot_overrides), (int32_t)sizeof(fot_result),
        (int32_t)sizeof(fot_batch), (int32_t)sizeof(fot_resample_params), (int32_t)sizeof(fot_safety),
        (int32_t)sizeof(fot_loop_frame), (int32_t)sizeof(fot_loop_request), (int32_t)sizeof(fot_wire_header),
        FOT_MAX_NT, FOT_MAX_CIRCLES, FOT_MAX_TI, FOT_MAX_TV, FOT_MAX_BRAKE, FOT_MAX_SAMPLES, FOT_MAX_PRED_LEN,
        FOT_PROFILE_KERNELS, FOT_MARGIN_GROUPS,
        (int32_t)sizeof(fot_loop_config), (int32_t)sizeof(fot_loop_step_out),
        (int32_t)sizeof(fot_loop_replay), (int32_t)sizeof(fot_loop_run_out), (int32_t)sizeof(fot_loop_summary),
        (int32_t)sizeof(fot_pred_origin), (int32_t)sizeof(fot_pred_score),
        (int32_t)sizeof(fot_sgan_desc), FOT_SGAN_MAX_EMBEDDING, FOT_SGAN_MAX_HIDDEN, FOT_SGAN_MAX_MLP, FOT_SGAN_MAX_BOTTLENECK,
        FOT_SGAN_MAX_OBS_LEN, FOT_SGAN_MAX_PEDS, FOT_SGAN_POOL_HIDDEN,
    };
    for (int i = 0; i < FOT_ABI_INFO_WORDS && i < cap && out; ++i) out[i] = v[i];
    return FOT_ABI_INFO_WORDS;
}

const char *fot_last_error(const fot_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int fot_create(const fot_params *params, int device, fot_handle **out)
{
    if (!params || !out) return fail(nullptr, FOT_ERR_INVALID, "params/out is NULL");
    *out = nullptr;
    DevParams P;
    std::string err;
    int rc = build_dev_params(*params, P, err);
    if (rc != FOT_OK) return fail(nullptr, rc, err);
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, FOT_ERR_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0) { e = hipGetDevice(&device); if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDevice"); }
    if (device >= n_dev) return fail(nullptr, FOT_ERR_INVALID, "device index out of range");
    fot_handle *h = new (std::nothrow) fot_handle();
    if (!h) return fail(nullptr, FOT_ERR_HIP, "out of host memory");
    h->device = device;
    if (const char *ev = std::getenv("FOT_LANES")) {             // tuning knob: 1 disables the split
        const int v = std::atoi(ev);
        if (v >= 1 && v <= FOT_LANES) h->lanes_cfg = v;
    }
    h->sc.reserve(FOT_MAX_SCENARIOS);
    h->sc.emplace_back();
    h->sc[0].params = *params;
    h->sc[0].P = P;
    auto bail = [&](hipError_t ee, const char *what) {
        int r = hip_fail(nullptr, ee, what);
        destroy_handle(h);
        return r;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    if ((e = hipEventCreateWithFlags(&h->fork, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&h->order_done, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    for (int l = 0; l < FOT_LANES; ++l) {
        Workspace &w = h->ws[l];
        // lane streams only when the handle splits batches; lane 0 of a single-lane handle runs on the caller's stream
        if (h->lanes_cfg > 1 && l < h->lanes_cfg &&
            (e = hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
        if (l >= h->lanes_cfg) continue;
        for (int i = 0; i < 2; ++i)
            if ((e = hipEventCreateWithFlags(&w.staging_done[i], hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&w.done, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    }
    if ((e = h->dP.ensure(sizeof(DevParams))) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemcpy(h->dP.p, &h->sc[0].P, sizeof(DevParams), hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy");
    if (upload_spline_table(h) != FOT_OK) { std::string m = h->err; destroy_handle(h); return fail(nullptr, FOT_ERR_HIP, m); }
    {
        int cut = TILE_CUT_AUTO;                                 // FOT_TILE_CUT=wave|group: diagnostics scripts
        if (const char *ev = std::getenv("FOT_TILE_CUT")) cut = ev[0] == 'g' ? TILE_CUT_GROUP : ev[0] == 'w' ? TILE_CUT_WAVE : TILE_CUT_AUTO;
        if (upload_tile_shapes(h, cut) != FOT_OK) { std::string m = h->err; destroy_handle(h); return fail(nullptr, FOT_ERR_HIP, m); }
    }
    { std::lock_guard<std::mutex> lk(g_live_mu); live_handles().insert(h); }
    *out = h;
    return FOT_OK;
}

int32_t fot_live_handles(void)
{
    std::lock_guard<std::mutex> lk(g_live_mu);
    return (int32_t)live_handles().size();
}

void fot_destroy(fot_handle *h)
{
    if (!h) return;
    {   // idempotent: only a handle fot_create handed out and nobody has destroyed yet (the pointer is not even read else)
        std::lock_guard<std::mutex> lk(g_live_mu);
        auto &live = live_handles();
        auto it = live.find(h);
        if (it == live.end()) return;
        live.erase(it);
    }
    destroy_handle(h);
}

}  // extern "C"

namespace {

void destroy_handle(fot_handle *h)
{
    const double budget = destroy_timeout_s();
    bool quiet = hipSetDevice(h->device) == hipSuccess;
    // the handle's own stream, the lanes' streams, and the event behind its last enqueue (which may be on a caller's
    // stream): polled, never waited on
    if (quiet && h->stream) quiet = drained([&] { return hipStreamQuery(h->stream); }, budget);
    if (quiet && h->order_valid) quiet = drained([&] { return hipEventQuery(h->order_done); }, budget);
    for (Workspace &w : h->ws) if (quiet && w.stream) quiet = drained([&] { return hipStreamQuery(w.stream); }, budget);
    if (!quiet) {
        // something is still running (or the runtime is already gone): the host-side struct goes, everything the device
        // may still touch stays until the process ends
        (void)hipGetLastError();
        delete h;
        return;
    }
    for (Scenario &S : h->sc) S.dSpline.release();
    DevBuf *bufs[] = { &h->dP, &h->dSplineTab, &h->dShapes, &h->dHeadTmpl, &h->dUserStatic, &h->dUserDyn, &h->dOut, &h->dTmpA, &h->dTmpB, &h->dTmpC, &h->dTmpD
                     };
    for (DevBuf *b : bufs) b->release();
    for (Workspace &w : h->ws) w.release();
    h->hSmallIn.release(); h->hSmallOut.release(); h->hRecOut.release(); h->hDone.release();
    h->hScoreIn.release(); h->hScoreOut.release(); h->dScoreT.release();
    h->sgan.release();
    h->loop.release();
    for (hipEvent_t e : h->prof_pool) (void)hipEventDestroy(e);
    if (h->fork) (void)hipEventDestroy(h->fork);
    if (h->order_done) (void)hipEventDestroy(h->order_done);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace

extern "C" {

int fot_set_scenario_path_waypoints(fot_handle *h, int32_t id, int32_t n, const double *wx, const double *wy)
{
    if (!h) return FOT_ERR_INVALID;
    if (id < 0 || id >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
    std::string err;
    HostSpline sp;
    int rc = build_spline(n, wx, wy, sp, err);
    if (rc != FOT_OK) return fail(h, rc, err);
    h->sc[(size_t)id].spline = sp;
    return upload_spline(h, id);
}

int fot_set_path_waypoints(fot_handle *h, int32_t n, const double *wx, const double *wy)
{
    return fot_set_scenario_path_waypoints(h, 0, n, wx, wy);
}

int fot_set_scenario_path_coeffs(fot_handle *h, int32_t id, int32_t n, const double *s,
                                 const double *ax, const double *bx, const double *cx, const double *dx,
                                 const double *ay, const double *by, const double *cy, const double *dy)
{
    if (!h) return FOT_ERR_INVALID;
    if (id < 0 || id >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
    if (n < 2 || !s || !ax || !bx || !cx || !dx || !ay || !by || !cy || !dy)
        return fail(h, FOT_ERR_INVALID, "spline needs >= 2 knots and all nine coefficient arrays");
    HostSpline &sp = h->sc[(size_t)id].spline;
    sp.n = n;
    sp.s.assign(s, s + n);
    sp.ax.assign(ax, ax + n); sp.bx.assign(bx, bx + n - 1); sp.cx.assign(cx, cx + n); sp.dx.assign(dx, dx + n - 1);
    sp.ay.assign(ay, ay + n); sp.by.assign(by, by + n - 1); sp.cy.assign(cy, cy + n); sp.dy.assign(dy, dy + n - 1);
    sp.bx.resize(n, 0.0); sp.dx.resize(n, 0.0); sp.by.resize(n, 0.0); sp.dy.resize(n, 0.0);
    return upload_spline(h, id);
}

int fot_set_path_coeffs(fot_handle *h, int32_t n, const double *s,
                        const double *ax, const double *bx, const double *cx, const double *dx,
                        const double *ay, const double *by, const double *cy, const double *dy)
{
    return fot_set_scenario_path_coeffs(h, 0, n, s, ax, bx, cx, dx, ay, by, cy, dy);
}

int fot_add_scenario(fot_handle *h, const fot_params *params, int32_t *id_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (!params || !id_out) return fail(h, FOT_ERR_INVALID, "params / id_out is NULL");
    const fot_params &p0 = h->sc[0].params;
    if (!(params->dt == p0.dt) || !(params->max_t == p0.max_t))
        return fail(h, FOT_ERR_INVALID, "a scenario has the handle's dt and max_t (one time grid per handle)");
    DevParams P;
    std::string err;
    int rc = build_dev_params(*params, P, err);
    if (rc != FOT_OK) return fail(h, rc, err);
    if ((int)h->sc.size() >= FOT_MAX_SCENARIOS) return fail(h, FOT_ERR_UNSUPPORTED, "more than FOT_MAX_SCENARIOS scenarios");
    h->sc.emplace_back();
    Scenario &S = h->sc.back();
    S.params = *params;
    S.P = P;
    rc = upload_params(h);
    if (rc == FOT_OK) rc = upload_spline_table(h);
    if (rc == FOT_OK) rc = upload_tile_shapes(h, h->tile_cut);
    if (rc != FOT_OK) {                                          // (a HIP failure: back to the scenarios before the call)
        h->sc.pop_back();
        (void)upload_params(h); (void)upload_spline_table(h); (void)upload_tile_shapes(h, h->tile_cut);
        return rc;
    }
    *id_out = (int32_t)h->sc.size() - 1;
    return FOT_OK;
}

int fot_get_path_coeffs(const fot_handle *h, int32_t *n_out, double *s,
                        double *ax, double *bx, double *cx, double *dx,
                        double *ay, double *by, double *cy, double *dy)
{
    return fot_get_scenario_path_coeffs(h, 0, n_out, s, ax, bx, cx, dx, ay, by, cy, dy);
}

int fot_get_scenario_path_coeffs(const fot_handle *h, int32_t id, int32_t *n_out, double *s,
                                 double *ax, double *bx, double *cx, double *dx,
                                 double *ay, double *by, double *cy, double *dy)
{
    if (!h) return FOT_ERR_NO_PATH_SET;
    if (id < 0 || id >= (int)h->sc.size()) return FOT_ERR_INVALID;
    if (!h->sc[(size_t)id].has_path) return FOT_ERR_NO_PATH_SET;
    const HostSpline &sp = h->sc[(size_t)id].spline;
    const int n = sp.n;
    if (n_out) *n_out = n;
    auto cp = [](double *dst, const std::vector<double> &src, int cnt) {
        if (dst) std::memcpy(dst, src.data(), sizeof(double) * (size_t)cnt);
    };
    cp(s, sp.s, n);
    cp(ax, sp.ax, n); cp(bx, sp.bx, n - 1); cp(cx, sp.cx, n); cp(dx, sp.dx, n - 1);
    cp(ay, sp.ay, n); cp(by, sp.by, n - 1); cp(cy, sp.cy, n); cp(dy, sp.dy, n - 1);
    return FOT_OK;
}

int fot_spline_eval(fot_handle *h, int32_t n, const double *s, double *x, double *y,
                    double *yaw, double *kappa, double *dkappa)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    if (n <= 0) return FOT_OK;
    if (!s) return fail(h, FOT_ERR_INVALID, "s is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    { int r = order_begin(h, h->stream); if (r != FOT_OK) return r; }
    HIP_TRY(h, h->dTmpA.ensure(sizeof(double) * (size_t)n));
    HIP_TRY(h, h->dTmpB.ensure(sizeof(double) * 5 * (size_t)n));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpA.p, s, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    LAUNCH_TRY(h, launch_spline_eval(spline_view(h, 0), n, h->dTmpA.as<double>(), h->dTmpB.as<double>(), h->stream));
    std::vector<double> outv((size_t)5 * n);
    HIP_TRY(h, hipMemcpyAsync(outv.data(), h->dTmpB.p, sizeof(double) * 5 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double *dst[5] = { x, y, yaw, kappa, dkappa };
    for (int f = 0; f < 5; ++f)
        if (dst[f]) std::memcpy(dst[f], outv.data() + (size_t)f * n, sizeof(double) * (size_t)n);
    return FOT_OK;
}

int fot_plan_batch_scenarios_device(fot_handle *h, const fot_batch *batch, const int32_t *scenario, fot_result *out_dev,
                                    void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (!batch) return fail(h, FOT_ERR_INVALID, "batch is NULL");
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return enqueue_plan(h, *batch, scenario, batch->static_xy, batch->dyn_xy, out_dev, st);
}

int fot_plan_batch_device(fot_handle *h, const fot_batch *batch, fot_result *out_dev, void *stream)
{
    return fot_plan_batch_scenarios_device(h, batch, nullptr, out_dev, stream);
}

int fot_resample_n_dense(const fot_resample_params *rp, int32_t pred_len)
{
    if (!rp || !(rp->sim_dt > 0.0) || !(rp->sgan_dt > 0.0) || pred_len < 1) return FOT_ERR_INVALID;
    return resample_n_dense(rp->sgan_dt, rp->sim_dt, rp->plan_horizon, pred_len);
}

namespace {

// shared body of fot_resample_predictions (cv = 0) and fot_predict_cv (cv = 1: anchor = obs_last, pred = obs_prev)
int resample_common(fot_handle *h, const fot_resample_params *rp, int cv, int32_t S, int32_t pred_len, int32_t P,
                    const void *pred, int32_t pred_dtype, const double *anchor, const double *current,
                    double staleness, void *out, int32_t out_dtype, int32_t on_device, int32_t *T_out,
                    double *sample_dist, void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (!rp || !(rp->sim_dt > 0.0) || !(rp->sgan_dt > 0.0)) return fail(h, FOT_ERR_INVALID, "sgan_dt and sim_dt must be positive");
    if (S < 0 || P < 0 || pred_len < 1) return fail(h, FOT_ERR_INVALID, "bad S / P / pred_len");
    if (pred_len > FOT_MAX_PRED_LEN) return fail(h, FOT_ERR_UNSUPPORTED, "pred_len > FOT_MAX_PRED_LEN");
    if ((pred_dtype != FOT_F32 && pred_dtype != FOT_F64) || (out_dtype != FOT_F32 && out_dtype != FOT_F64))
        return fail(h, FOT_ERR_INVALID, "dtype");
    const int n_dense = resample_n_dense(rp->sgan_dt, rp->sim_dt, rp->plan_horizon, pred_len);
    const int T = n_dense + (current ? 1 : 0);
    if (T > FOT_MAX_NT) return fail(h, FOT_ERR_UNSUPPORTED, "more than FOT_MAX_NT time steps");
    if (T_out) *T_out = T;
    const int tmajor = (on_device & FOT_OUT_TMAJOR) ? 1 : 0;
    on_device &= FOT_OUT_DEVICE;
    if (S == 0 || P == 0 || T == 0) return FOT_OK;
    if (!out || (!cv && !pred) || (cv && !anchor)) return fail(h, FOT_ERR_INVALID, "NULL tensor");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // small per-pedestrian inputs: anchor | current  (and obs_prev for cv) through the handle's scratch
    const size_t row = sizeof(double) * 2 * (size_t)P;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }  // the scratch below is shared by every entry point
    {
        const size_t in_elem_ = pred_dtype == FOT_F32 ? 4 : 8, out_elem_ = out_dtype == FOT_F32 ? 4 : 8;
        const size_t in_b = cv ? 0 : in_elem_ * 2 * (size_t)P * (size_t)S * pred_len;
        const size_t out_b = out_elem_ * 2 * (size_t)S * P * T;
        if (!on_device && 3 * align256(row) + align256(in_b) <= SMALL_CALL_BYTES &&
            out_b + sizeof(double) * (size_t)S <= SMALL_CALL_BYTES) {
            // small host call: everything through pinned memory the kernels access directly
            HIP_TRY(h, h->hSmallIn.ensure(3 * align256(row) + align256(in_b)));
            HIP_TRY(h, h->hSmallOut.ensure(align256(out_b) + sizeof(double) * (size_t)S));
            char *p = (char *)h->hSmallIn.p;
            const double *pa = nullptr, *pc = nullptr;
            const void *pp = nullptr;
            if (anchor) { std::memcpy(p, anchor, row); pa = (const double *)p; }
            if (current) { std::memcpy(p + align256(row), current, row); pc = (const double *)(p + align256(row)); }
            if (cv) { if (pred) { std::memcpy(p + 2 * align256(row), pred, row); pp = p + 2 * align256(row); } }
            else { std::memcpy(p + 3 * align256(row), pred, in_b); pp = p + 3 * align256(row); }
            char *po = (char *)h->hSmallOut.p;
            LAUNCH_TRY(h, launch_resample(rp->sgan_dt, rp->sim_dt, staleness, S, pred_len, P, n_dense, anchor ? 1 : 0,
                                          current ? 1 : 0, cv, pp, cv ? FOT_F64 : pred_dtype, pa, pc, po, out_dtype,
                                          tmajor, st));
            if (sample_dist)
                LAUNCH_TRY(h, launch_sample_dist(S, P, T, current ? 1 : 0, po, out_dtype, tmajor,
                                                 (double *)(po + align256(out_b)), st));
            { int r = order_end(h, st); if (r != FOT_OK) return r; }
            HIP_TRY(h, hipStreamSynchronize(st));
            std::memcpy(out, po, out_b);
            if (sample_dist) std::memcpy(sample_dist, po + align256(out_b), sizeof(double) * (size_t)S);
            return FOT_OK;
        }
    }
    HIP_TRY(h, h->dTmpA.ensure(3 * row + 64));
    char *scr = (char *)h->dTmpA.p;
    const double *d_anchor = nullptr, *d_current = nullptr;
    const void *d_pred = pred;
    if (anchor) { HIP_TRY(h, hipMemcpyAsync(scr, anchor, row, hipMemcpyHostToDevice, st)); d_anchor = (const double *)scr; }
    if (current) { HIP_TRY(h, hipMemcpyAsync(scr + row, current, row, hipMemcpyHostToDevice, st)); d_current = (const double *)(scr + row); }
    void *d_out = out;
    const size_t in_elem = pred_dtype == FOT_F32 ? 4 : 8, out_elem = out_dtype == FOT_F32 ? 4 : 8;
    const size_t in_bytes = in_elem * 2 * (size_t)P * (cv ? 1 : (size_t)S * pred_len);
    const size_t out_bytes = out_elem * 2 * (size_t)S * P * T;
    if (cv) {                                                      // obs_prev is a host array of doubles
        d_pred = nullptr;
        if (pred) { HIP_TRY(h, hipMemcpyAsync(scr + 2 * row, pred, row, hipMemcpyHostToDevice, st)); d_pred = scr + 2 * row; }
    } else if (!on_device) {
        HIP_TRY(h, h->dTmpB.ensure(in_bytes));
        HIP_TRY(h, hipMemcpyAsync(h->dTmpB.p, pred, in_bytes, hipMemcpyHostToDevice, st));
        d_pred = h->dTmpB.p;
    }
    if (!on_device) { HIP_TRY(h, h->dTmpC.ensure(out_bytes)); d_out = h->dTmpC.p; }
    LAUNCH_TRY(h, launch_resample(rp->sgan_dt, rp->sim_dt, staleness, S, pred_len, P, n_dense, anchor ? 1 : 0,
                                  current ? 1 : 0, cv, d_pred, cv ? FOT_F64 : pred_dtype, d_anchor, d_current, d_out,
                                  out_dtype, tmajor, st));
    if (sample_dist) {
        HIP_TRY(h, h->dTmpD.ensure(sizeof(double) * (size_t)S));
        LAUNCH_TRY(h, launch_sample_dist(S, P, T, current ? 1 : 0, d_out, out_dtype, tmajor, h->dTmpD.as<double>(), st));
        HIP_TRY(h, hipMemcpyAsync(sample_dist, h->dTmpD.p, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, st));
    }
    if (!on_device) HIP_TRY(h, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    if (!on_device || sample_dist) HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

}  // namespace

int fot_resample_predictions(fot_handle *h, const fot_resample_params *rp, int32_t S, int32_t pred_len, int32_t P,
                             const void *pred, int32_t pred_dtype, const double *anchor, const double *current,
                             double staleness, void *out, int32_t out_dtype, int32_t on_device, int32_t *T_out,
                             double *sample_dist, void *stream)
{
    return resample_common(h, rp, 0, S, pred_len, P, pred, pred_dtype, anchor, current, staleness, out, out_dtype,
                           on_device, T_out, sample_dist, stream);
}

int fot_predict_cv(fot_handle *h, const fot_resample_params *rp, int32_t pred_len, int32_t P,
                   const void *obs_last, const void *obs_prev, int32_t obs_dtype, const double *current,
                   double staleness, void *out, int32_t out_dtype, int32_t on_device, int32_t *T_out, void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (obs_dtype == FOT_F64)
        return resample_common(h, rp, 1, 1, pred_len, P, obs_prev, FOT_F64, (const double *)obs_last, current, staleness,
                               out, out_dtype, on_device, T_out, nullptr, stream);
    if (obs_dtype != FOT_F32) return fail(h, FOT_ERR_INVALID, "obs_dtype");
    // float32 observations travel widened (exact); cv mode 2 forms the velocity in float32
    const size_t n = 2 * (size_t)(P > 0 ? P : 0);
    std::vector<double> last(n), prev(n);
    for (size_t i = 0; i < n && obs_last; ++i) last[i] = (double)((const float *)obs_last)[i];
    for (size_t i = 0; i < n && obs_prev; ++i) prev[i] = (double)((const float *)obs_prev)[i];
    return resample_common(h, rp, 2, 1, pred_len, P, obs_prev ? prev.data() : nullptr, FOT_F64,
                           obs_last ? last.data() : nullptr, current, staleness, out, out_dtype, on_device, T_out,
                           nullptr, stream);
}

int fot_safety_metrics_batch(fot_handle *h, int32_t n, const double *ego, const int32_t *ped_off,
                             const double *ped_pos, const double *ped_vel, double ego_radius, double ped_radius,
                             int32_t use_footprint, fot_safety *out)
{
    if (!h) return FOT_ERR_INVALID;
    if (n <= 0) return n == 0 ? FOT_OK : fail(h, FOT_ERR_INVALID, "n < 0");
    if (!ego || !ped_off || !out) return fail(h, FOT_ERR_INVALID, "NULL array");
    for (int i = 0; i < n; ++i)
        if (ped_off[i + 1] < ped_off[i] || ped_off[0] < 0) return fail(h, FOT_ERR_INVALID, "ped_off must be non-decreasing");
    const size_t n_ped = (size_t)ped_off[n];
    if (n_ped > 0 && (!ped_pos || !ped_vel)) return fail(h, FOT_ERR_INVALID, "NULL pedestrian array");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const size_t ego_b = sizeof(double) * 4 * (size_t)n, off_b = align256(sizeof(int32_t) * ((size_t)n + 1));
    const size_t ped_b = sizeof(double) * 2 * std::max<size_t>(n_ped, 1);
    if (align256(ego_b) + off_b + 2 * align256(ped_b) <= SMALL_CALL_BYTES && sizeof(fot_safety) * (size_t)n <= SMALL_CALL_BYTES) {
        // small call: the kernel reads its inputs from, and writes its results to, pinned host memory (no copy operations)
        HIP_TRY(h, h->hSmallIn.ensure(align256(ego_b) + off_b + 2 * align256(ped_b)));
        HIP_TRY(h, h->hSmallOut.ensure(sizeof(fot_safety) * (size_t)n));
        char *p = (char *)h->hSmallIn.p;
        char *p_off = p + align256(ego_b), *p_pos = p_off + off_b, *p_vel = p_pos + align256(ped_b);
        std::memcpy(p, ego, ego_b);
        std::memcpy(p_off, ped_off, sizeof(int32_t) * ((size_t)n + 1));
        if (n_ped) { std::memcpy(p_pos, ped_pos, sizeof(double) * 2 * n_ped); std::memcpy(p_vel, ped_vel, sizeof(double) * 2 * n_ped); }
        LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, (const double *)p, (const int32_t *)p_off, (const double *)p_pos,
                                    (const double *)p_vel, ego_radius, ped_radius, h->sc[0].params.footprint_radius,
                                    use_footprint, (fot_safety *)h->hSmallOut.p, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        std::memcpy(out, h->hSmallOut.p, sizeof(fot_safety) * (size_t)n);
        return FOT_OK;
    }
    HIP_TRY(h, h->dTmpA.ensure(align256(ego_b) + off_b));
    HIP_TRY(h, h->dTmpB.ensure(2 * align256(ped_b)));
    HIP_TRY(h, h->dTmpC.ensure(sizeof(fot_safety) * (size_t)n));
    char *a = (char *)h->dTmpA.p, *b = (char *)h->dTmpB.p;
    HIP_TRY(h, hipMemcpyAsync(a, ego, ego_b, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(a + align256(ego_b), ped_off, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    if (n_ped) {
        HIP_TRY(h, hipMemcpyAsync(b, ped_pos, sizeof(double) * 2 * n_ped, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(b + align256(ped_b), ped_vel, sizeof(double) * 2 * n_ped, hipMemcpyHostToDevice, st));
    }
    LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, (const double *)a, (const int32_t *)(a + align256(ego_b)),
                                (const double *)b, (const double *)(b + align256(ped_b)), ego_radius, ped_radius,
                                h->sc[0].params.footprint_radius, use_footprint, h->dTmpC.as<fot_safety>(), st));
    HIP_TRY(h, hipMemcpyAsync(out, h->dTmpC.p, sizeof(fot_safety) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

int fot_loop_set_scenario_static(fot_handle *h, int32_t id, int32_t n_points, const double *xy)
{
    if (!h) return FOT_ERR_INVALID;
    if (id < 0 || id >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
    if (n_points < 0 || (n_points > 0 && !xy)) return fail(h, FOT_ERR_INVALID, "static points");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // nothing may still be reading the old copies
    LoopState &L = h->loop;
    if (L.scen_static.size() < h->sc.size()) L.scen_static.resize(h->sc.size());
    L.scen_static[(size_t)id].assign(xy, xy + 2 * (size_t)n_points);
    L.scen_static_dirty = true;                                  // (uploaded by the next scenario loop's step / replay)
    if (id == 0) {                                               // scenario 0 is what a fot_loop_begin loop sees
        L.static_xy = L.scen_static[0];
        L.static_tiles = 0;
    }
    return FOT_OK;
}

int fot_loop_set_static(fot_handle *h, int32_t n_points, const double *xy)
{
    return fot_loop_set_scenario_static(h, 0, n_points, xy);
}

}  // extern "C"

namespace {

// A scenario loop's static points: every scenario's set once in HBM (rebuilt after fot_loop_set_scenario_static), and
// room for the per-request blocks of n_req requests.  Synchronises only when something has to be uploaded or to grow.
int ensure_scen_static(fot_handle *h, int n_req, hipStream_t st)
{
    LoopState &L = h->loop;
    const size_t n_sc = h->sc.size();
    if (L.scen_static_dirty || L.scen_static_off.size() != n_sc + 1) {
        L.scen_static.resize(n_sc);
        std::vector<int32_t> off(n_sc + 1, 0);
        for (size_t s = 0; s < n_sc; ++s) off[s + 1] = off[s] + (int32_t)(L.scen_static[s].size() / 2);
        std::vector<double> all;
        all.reserve(2 * (size_t)off[n_sc]);
        for (size_t s = 0; s < n_sc; ++s) all.insert(all.end(), L.scen_static[s].begin(), L.scen_static[s].end());
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, L.dScenStatic.ensure(sizeof(double) * std::max<size_t>(all.size(), 2)));
        if (!all.empty()) HIP_TRY(h, hipMemcpy(L.dScenStatic.p, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice));
        L.scen_static_off = off;
        L.scen_static_dirty = false;
    }
    int32_t most = 0;
    for (size_t s = 0; s + 1 < L.scen_static_off.size(); ++s) most = std::max(most, L.scen_static_off[s + 1] - L.scen_static_off[s]);
    const size_t need = sizeof(double) * 2 * (size_t)most * (size_t)std::max(n_req, 1);
    if (need > L.dGather.cap || sizeof(StaticGather) * (size_t)std::max(n_req, 1) > L.hGather.cap) {
        HIP_TRY(h, hipStreamSynchronize(st));                    // (a block that grows moves)
        HIP_TRY(h, L.dGather.ensure(std::max<size_t>(need, 16)));
        HIP_TRY(h, L.hGather.ensure(sizeof(StaticGather) * (size_t)std::max(n_req, 1)));
    }
    return FOT_OK;
}

// FOT_LOOP_PLAN_REPRESENTATIVE: room for a frame of n_ep episodes on slots below n_slots with `rows` pedestrians and T time
// entries per track.  (A block that grows is freed first, which waits for the device: nothing still reads the old one.)
int rep_ensure(fot_handle *h, int n_slots, int n_ep, size_t rows, int T)
{
    LoopRep &Q = h->loop.rep;
    const size_t ns = (size_t)std::max(n_slots, 1), ne = (size_t)std::max(n_ep, 1);
    HIP_TRY(h, Q.dBlk.ensure(sizeof(double) * 2 * std::max<size_t>(rows, 1) * (size_t)T));
    HIP_TRY(h, Q.dBest.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, Q.dDev.ensure(sizeof(double) * ns * FOT_MAX_SAMPLES));
    HIP_TRY(h, Q.dPre.ensure(sizeof(int32_t) * ne));
    HIP_TRY(h, Q.hBest.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, Q.hPre.ensure(sizeof(int32_t) * ne));
    return FOT_OK;
}

// The planning blocks of the frame's n episodes behind their distribution blocks in dDyn (f: pos, ped0, blk): the
// selection into the given tables (the mode's own, or the scores' where a resident loop scores too), then
// k_loop_rep_block.  Enqueue only.
int rep_enqueue(fot_handle *h, const int32_t *slot_of, const FrameDev &f, int n, int S, int n_dense, double *dev_tab,
                int32_t *best_tab, int32_t *best_host, hipStream_t st)
{
    LoopState &L = h->loop;
    LoopRep &Q = L.rep;
    LAUNCH_TRY(h, launch_loop_best_sample(slot_of, f, L.dDyn.as<double>(), n, S, n_dense, dev_tab, best_tab, best_host, st));
    LAUNCH_TRY(h, launch_loop_rep_block(slot_of, f, L.dDyn.as<double>(), best_tab, n, S, n_dense, Q.dBlk.as<double>(),
                                        Q.dPre.as<int32_t>(), (int32_t *)Q.hPre.p, st));
    return FOT_OK;
}

// The requests of a loop step as one plan call against the step's tensor (LoopState: pedestrian counts, block offsets and
// lengths of the frame's episodes), records to rec_out: enqueued on st, not waited for.
int loop_enqueue_requests(fot_handle *h, int32_t n_req, const fot_loop_request *req, fot_result *rec_out, hipStream_t st,
                          bool sync_caller)
{
    LoopState &L = h->loop;
    const int n_ep = (int)L.ped_off.size() - 1;
    const bool by_scen = !L.frame_scen.empty();                  // a scenario loop: request j is on its episode's scenario
    const int n_static = by_scen ? 0 : (int)(L.static_xy.size() / 2);
    std::vector<int32_t> scen;
    if (by_scen) {
        scen.resize((size_t)n_req);
        for (int j = 0; j < n_req; ++j) {
            const int e = req[j].episode;
            if (e < 0 || e >= n_ep || e >= (int)L.frame_scen.size()) return fail(h, FOT_ERR_INVALID, "request: episode out of range");
            scen[(size_t)j] = L.frame_scen[(size_t)e];
        }
        int r = ensure_scen_static(h, n_req, st); if (r != FOT_OK) return r;
    }
    if (n_static > 0 && L.static_tiles < n_req) {              // (grows a few times in the life of a loop)
        const int tiles = std::max(n_req, 2 * L.static_tiles);
        std::vector<double> rep((size_t)tiles * L.static_xy.size());
        for (int t = 0; t < tiles; ++t)
            std::memcpy(rep.data() + (size_t)t * L.static_xy.size(), L.static_xy.data(), sizeof(double) * L.static_xy.size());
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, L.dStatic.ensure(sizeof(double) * rep.size()));
        HIP_TRY(h, hipMemcpy(L.dStatic.p, rep.data(), sizeof(double) * rep.size(), hipMemcpyHostToDevice));
        L.static_tiles = tiles;
    }
    std::vector<fot_ego> ego((size_t)n_req);
    std::vector<fot_overrides> ov((size_t)n_req);
    std::vector<double> tgt((size_t)n_req), stop((size_t)n_req);
    std::vector<int32_t> s_off((size_t)n_req + 1), dims(4 * (size_t)n_req);
    std::vector<int64_t> d_off((size_t)n_req);
    bool any_dyn = false;
    for (int j = 0; j < n_req; ++j) {
        const int e = req[j].episode;
        if (e < 0 || e >= n_ep) return fail(h, FOT_ERR_INVALID, "request: episode out of range");
        ego[j] = req[j].ego; ov[j] = req[j].overrides; tgt[j] = req[j].target_speed; stop[j] = req[j].max_stop_distance;
        if (!by_scen) s_off[j] = j * n_static;
        if (by_scen) {
            // its scenario's points: gathered on the device into [s_off[j], s_off[j + 1]) of dGather, the layout k_cull reads
            const int32_t sc = scen[(size_t)j], src = L.scen_static_off[(size_t)sc], cnt = L.scen_static_off[(size_t)sc + 1] - src;
            StaticGather &g = ((StaticGather *)L.hGather.p)[j];
            g.src = src; g.dst = s_off[j]; g.n = cnt; g._pad = 0;
            s_off[j + 1] = s_off[j] + cnt;
        }
        const int P_e = L.ped_off[e + 1] - L.ped_off[e];
        if (L.rep.frame) {
            // its episode's representative sample: one [P_e][T][2] block per episode, in the frame's pedestrian order
            d_off[j] = (int64_t)L.ped_off[e] * L.rep.T;
            dims[4 * j] = P_e > 0 ? FOT_DYN_SINGLE : FOT_DYN_NONE;
            dims[4 * j + 1] = 1; dims[4 * j + 2] = P_e; dims[4 * j + 3] = L.rep.T;
        } else {
            d_off[j] = L.blk_off[e];
            dims[4 * j] = P_e > 0 ? (L.dist_S > 0 ? FOT_DYN_DISTRIBUTION : FOT_DYN_SINGLE) : FOT_DYN_NONE;
            dims[4 * j + 1] = L.dist_S > 0 ? L.dist_S : 1; dims[4 * j + 2] = P_e; dims[4 * j + 3] = L.t_len[e];
        }
        any_dyn = any_dyn || P_e > 0;
    }
    if (!by_scen) s_off[n_req] = n_req * n_static;
    fot_batch b = fot_batch();
    b.n_inst = n_req; b.obstacle_dtype = FOT_F64;
    b.ego = ego.data(); b.target_speed = tgt.data(); b.overrides = ov.data(); b.max_stop_distance = stop.data();
    if (n_static > 0) { b.static_xy = L.dStatic.p; b.static_off = s_off.data(); }
    if (by_scen && s_off[n_req] > 0) {
        if (sizeof(double) * 2 * (size_t)s_off[n_req] > L.dGather.cap) return fail(h, FOT_ERR_INVALID, "internal: static block too small");
        { int r = check_scenarios(h, b, scen.data()); if (r != FOT_OK) return r; }   // (a refused call enqueues nothing)
        { int r = order_begin(h, st); if (r != FOT_OK) return r; }
        LAUNCH_TRY(h, launch_static_gather((const StaticGather *)L.hGather.p, n_req, L.dScenStatic.as<double>(),
                                           L.dGather.as<double>(), st));
        b.static_xy = L.dGather.p; b.static_off = s_off.data();
    }
    if (any_dyn) { b.dyn_xy = L.rep.frame ? L.rep.dBlk.p : L.dyn_ptr; b.dyn_off = d_off.data(); b.dyn_dims = dims.data(); }
    return enqueue_plan(h, b, by_scen ? scen.data() : nullptr, b.static_xy, b.dyn_xy, rec_out, st, sync_caller);
}

// fot_loop_plan; rec_first: the request's records start at record rec_first of the handle's pinned block (the escalation
// levels of a step land behind its level-0 records, which stay where they are)
// ep_scen: the scenario of each episode of the frame (a scenario loop's step), or nullptr: all on scenario 0
// ep_slot: the slot of each episode of the frame (fot_loop_step), or nullptr: episode i is slot i (what the representative
// sample's tables are indexed by)
int loop_plan_impl(fot_handle *h, const fot_loop_frame *frame, int32_t n_req, const fot_loop_request *req,
                   fot_safety *safety_out, const fot_result **records, int32_t rec_first, const int32_t *ep_scen = nullptr,
                   const int32_t *ep_slot = nullptr)
{
    if (!h) return FOT_ERR_INVALID;
    if (!ep_scen && (frame || h->loop.frame_scen.empty()) && !h->sc[0].has_path)
        return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    if (n_req < 0 || (n_req > 0 && (!req || !records))) return fail(h, FOT_ERR_INVALID, "requests");
    LoopState &L = h->loop;
    if (!frame && !L.have_frame) return fail(h, FOT_ERR_INVALID, "no frame: the first fot_loop_plan of a step carries one");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (L.observe_n > 0) {                                       // a fot_loop_observe_begin nobody collected: its launches
        HIP_TRY(h, hipStreamSynchronize(st));                    // still read the frame's pinned block
        L.observe_n = -1;
    }
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    bool metrics = false, rep_pending = false;
    std::vector<int32_t> rep_slots;                              // the frame's slots, where it left representative samples
    if (frame) {
        const int n = frame->n_episodes;
        if (n < 0 || !frame->ped_off) return fail(h, FOT_ERR_INVALID, "frame: n_episodes / ped_off (one offset even for no episode)");
        L.have_frame = false;
        for (int i = 0; i < n; ++i)
            if (frame->ped_off[i + 1] < frame->ped_off[i] || frame->ped_off[0] != 0)
                return fail(h, FOT_ERR_INVALID, "ped_off must start at 0 and be non-decreasing");
        const size_t n_ped = n > 0 ? (size_t)frame->ped_off[n] : 0;
        if (n_ped > 0 && (!frame->ped_pos || !frame->ped_vel)) return fail(h, FOT_ERR_INVALID, "frame: NULL pedestrian array");
        const bool ready = frame->obs_last != nullptr;
        const bool dist = ready && frame->dist_raw != nullptr;
        if (dist && (frame->dist_S < 1 || frame->dist_S > FOT_MAX_SAMPLES || (frame->dist_dtype != FOT_F32 && frame->dist_dtype != FOT_F64)))
            return fail(h, dist && frame->dist_S > FOT_MAX_SAMPLES ? FOT_ERR_UNSUPPORTED : FOT_ERR_INVALID, "frame: dist_S / dist_dtype");
        if (ready && !dist && n > 0 && !frame->prepend) return fail(h, FOT_ERR_INVALID, "frame: prepend missing");
        if (ready && (!(frame->rp.sim_dt > 0.0) || !(frame->rp.sgan_dt > 0.0) || frame->pred_len < 1 ||
                      frame->pred_len > FOT_MAX_PRED_LEN))
            return fail(h, FOT_ERR_INVALID, "frame: predictor parameters");
        const int n_dense = ready ? resample_n_dense(frame->rp.sgan_dt, frame->rp.sim_dt, frame->rp.plan_horizon, frame->pred_len) : 1;
        if (n_dense + 1 > FOT_MAX_NT) return fail(h, FOT_ERR_UNSUPPORTED, "more than FOT_MAX_NT time steps");
        // pinned block: ego[n][4] | ped_off | pos | vel | obs_last (widened) | obs_prev (widened) | block offsets | ped -> episode
        const size_t ego_b = align256(sizeof(double) * 4 * (size_t)std::max(n, 1));
        const size_t off_b = align256(sizeof(int32_t) * ((size_t)n + 1));
        const size_t ped_b = align256(sizeof(double) * 2 * std::max<size_t>(n_ped, 1));
        const size_t blk_b = align256(sizeof(int64_t) * ((size_t)n + 1)), pe_b = align256(sizeof(int32_t) * std::max<size_t>(n_ped, 1));
        const bool rep_on = L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE && dist;   // (never a scenario loop: the tail is free)
        HIP_TRY(h, L.hFrame.ensure(ego_b + off_b + 4 * ped_b + blk_b + pe_b + (ep_scen || rep_on ? off_b : 0)));
        char *p = (char *)L.hFrame.p;
        double *p_ego = (double *)p;
        int32_t *p_off = (int32_t *)(p + ego_b);
        double *p_pos = (double *)(p + ego_b + off_b), *p_vel = (double *)((char *)p_pos + ped_b);
        double *p_last = (double *)((char *)p_vel + ped_b), *p_prev = (double *)((char *)p_last + ped_b);
        if (frame->ego) std::memcpy(p_ego, frame->ego, sizeof(double) * 4 * (size_t)n);
        std::memcpy(p_off, frame->ped_off, sizeof(int32_t) * ((size_t)n + 1));
        if (n_ped) {
            std::memcpy(p_pos, frame->ped_pos, sizeof(double) * 2 * n_ped);
            std::memcpy(p_vel, frame->ped_vel, sizeof(double) * 2 * n_ped);
            if (ready) for (size_t i = 0; i < 2 * n_ped; ++i) p_last[i] = (double)frame->obs_last[i];   // (exact)
            if (ready && frame->obs_prev) for (size_t i = 0; i < 2 * n_ped; ++i) p_prev[i] = (double)frame->obs_prev[i];
        }
        L.ped_off.assign(frame->ped_off, frame->ped_off + n + 1);
        L.blk_off.assign((size_t)n + 1, 0);
        L.t_len.assign((size_t)std::max(n, 1), 1);
        L.dist_S = dist ? frame->dist_S : 0;
        L.rep.frame = false;
        for (int e = 0; e < n; ++e) {
            L.t_len[e] = dist ? n_dense + 1 : ready ? n_dense + (frame->prepend[e] ? 1 : 0) : 1;
            L.blk_off[e + 1] = L.blk_off[e] + (int64_t)(dist ? frame->dist_S : 1) * (L.ped_off[e + 1] - L.ped_off[e]) * L.t_len[e];
        }
        L.p_off = p_off; L.p_pos = p_pos; L.p_vel = p_vel;
        L.p_scen = nullptr; L.frame_scen.clear();
        if (ep_scen && n > 0) {                                    // the episodes' scenarios, behind the other tables
            int32_t *p_sc = (int32_t *)(p + ego_b + off_b + 4 * ped_b + blk_b + pe_b);
            std::memcpy(p_sc, ep_scen, sizeof(int32_t) * (size_t)n);
            L.p_scen = p_sc; L.frame_scen.assign(ep_scen, ep_scen + n);
        }
        L.ego_radius = frame->ego_radius; L.ped_radius = frame->ped_radius; L.use_footprint = frame->use_footprint;
        L.dyn_ptr = p_pos;                                         // not ready: the current positions, read in place
        if (dist && n_ped > 0) {
            // every sample of every pedestrian in one launch, each episode's samples into its own [S][P_e][T][2] block
            int64_t *p_blk = (int64_t *)((char *)p_prev + ped_b);
            int32_t *p_pe = (int32_t *)((char *)p_blk + blk_b);
            for (int e = 0; e <= n; ++e) p_blk[e] = L.blk_off[e];
            for (int e = 0; e < n; ++e) for (int q = L.ped_off[e]; q < L.ped_off[e + 1]; ++q) p_pe[q] = e;
            HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * (size_t)L.blk_off[n]));
            L.dyn_ptr = L.dDyn.p;
            LAUNCH_TRY(h, launch_resample(frame->rp.sgan_dt, frame->rp.sim_dt, frame->staleness, frame->dist_S, frame->pred_len,
                                          (int)n_ped, n_dense, 1, 1, 0, frame->dist_raw, frame->dist_dtype, p_last, p_pos,
                                          L.dDyn.p, FOT_F64, 0, st, p_pe, p_off, p_blk));
            if (rep_on) {
                // the selection and every episode's single-sample block behind the resample, on the same stream
                int32_t *p_slot = (int32_t *)(p + ego_b + off_b + 4 * ped_b + blk_b + pe_b);
                int n_tab = std::max(L.ep.n, n);
                for (int e = 0; e < n; ++e) p_slot[e] = ep_slot ? ep_slot[e] : e;
                { int r = rep_ensure(h, n_tab, n, n_ped, n_dense + 1); if (r != FOT_OK) return r; }
                FrameDev fd;
                fd.pos = p_pos; fd.ped0 = p_off; fd.blk = p_blk;
                { int r = rep_enqueue(h, p_slot, fd, n, frame->dist_S, n_dense, L.rep.dDev.as<double>(), L.rep.dBest.as<int32_t>(),
                                      (int32_t *)L.rep.hBest.p, st); if (r != FOT_OK) return r; }
            }
        } else if (ready && n_ped > 0) {
            HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * (size_t)L.blk_off[n]));
            L.dyn_ptr = L.dDyn.p;
            // one launch per run of episodes that agree on the prepend (normally one run: the whole frame)
            for (int e0 = 0; e0 < n;) {
                int e1 = e0 + 1;
                while (e1 < n && (frame->prepend[e1] != 0) == (frame->prepend[e0] != 0)) ++e1;
                const int r0 = L.ped_off[e0], cnt = L.ped_off[e1] - r0, pre = frame->prepend[e0] ? 1 : 0;
                if (cnt > 0)
                    LAUNCH_TRY(h, launch_resample(frame->rp.sgan_dt, frame->rp.sim_dt, frame->staleness, 1, frame->pred_len,
                                                  cnt, n_dense, 1, pre, 2, frame->obs_prev ? p_prev + 2 * (size_t)r0 : nullptr,
                                                  FOT_F64, p_last + 2 * (size_t)r0, pre ? p_pos + 2 * (size_t)r0 : nullptr,
                                                  L.dDyn.as<double>() + 2 * L.blk_off[e0], FOT_F64, 0, st));
                e0 = e1;
            }
        }
        if (frame->ego && safety_out && n > 0) {
            HIP_TRY(h, L.hOut.ensure(sizeof(fot_safety) * (size_t)n));
            LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, p_ego, p_off, p_pos, p_vel, L.ego_radius, L.ped_radius,
                                        h->sc[0].params.footprint_radius, L.use_footprint, (fot_safety *)L.hOut.p, st,
                                        L.p_scen, L.dSafScen.as<SafetyScen>()));
            metrics = true;
        }
        if (rep_on) {
            L.rep.frame = true; L.rep.T = n_dense + 1;
            rep_pending = n_ped > 0;
            rep_slots.assign((size_t)n, 0);
            for (int e = 0; e < n; ++e) rep_slots[(size_t)e] = ep_slot ? ep_slot[e] : e;
        }
        L.have_frame = true;
    }
    const int n_ep = (int)L.ped_off.size() - 1;
    if (n_req > 0) {
        if (rec_first > 0 && sizeof(fot_result) * ((size_t)rec_first + (size_t)n_req) > L.hRec.cap)
            return fail(h, FOT_ERR_INVALID, "internal: record block too small for the escalation levels");
        HIP_TRY(h, L.hRec.ensure(sizeof(fot_result) * ((size_t)rec_first + (size_t)n_req)));
        fot_result *rec_out = (fot_result *)L.hRec.p + rec_first;
        {
            // the records' flags instead of the stream (wait_records): the metrics' kernel ran ahead of the plan kernels on
            // this stream and wrote host memory directly, so its results are there once a record behind it is
            arm_records(h, n_req);
            int rc = loop_enqueue_requests(h, n_req, req, rec_out, st, true);
            if (rc != FOT_OK) { h->done_seq_armed = false; return rc; }
            rc = wait_records(h, n_req, st);
            if (rc != FOT_OK) return rc;
        }
    } else {
        int r = order_end(h, st); if (r != FOT_OK) return r;
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    if (metrics) std::memcpy(safety_out, L.hOut.p, sizeof(fot_safety) * (size_t)n_ep);
    if (frame && L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE)     // (a frame without a distribution chose nothing)
        std::fill(L.rep.last_best.begin(), L.rep.last_best.end(), -1);
    if (frame && L.rep.frame) {                                  // (the selection ran ahead of the plan on this stream)
        const int32_t *best = (const int32_t *)L.rep.hBest.p;
        for (size_t e = 0; e < rep_slots.size(); ++e) {
            const int slot = rep_slots[e];
            if (rep_pending && slot < (int)L.rep.last_best.size() && L.ped_off[e + 1] > L.ped_off[e]) L.rep.last_best[(size_t)slot] = best[slot];
        }
    }
    if (records) *records = n_req > 0 ? (const fot_result *)L.hRec.p + rec_first : nullptr;
    return FOT_OK;
}

}  // namespace

extern "C" {

int fot_loop_plan(fot_handle *h, const fot_loop_frame *frame, int32_t n_req, const fot_loop_request *req,
                  fot_safety *safety_out, const fot_result **records)
{
    return loop_plan_impl(h, frame, n_req, req, safety_out, records, 0);
}

}  // extern "C"

namespace {

// fot_loop_observe_begin; a scenario loop's frame (LoopState::frame_scen): ego i is measured with, and projected on the
// path of, the scenario of episode i
int observe_begin_impl(fot_handle *h, int32_t n, const double *ego5, const double *prev_s)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    const bool by_scen = !L.frame_scen.empty();
    if (!by_scen && !h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    L.observe_n = -1;
    if (!L.have_frame) return fail(h, FOT_ERR_INVALID, "no frame: fot_loop_plan of this step comes first");
    if (n != (int)L.ped_off.size() - 1) return fail(h, FOT_ERR_INVALID, "one ego per episode of the frame");
    if (n <= 0) { L.observe_n = 0; return FOT_OK; }
    if (!ego5) return fail(h, FOT_ERR_INVALID, "ego5 is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const size_t ego_b = align256(sizeof(double) * 4 * (size_t)n), desc_b = align256(sizeof(InstDesc) * (size_t)n);
    const size_t saf_b = align256(sizeof(fot_safety) * (size_t)n);
    HIP_TRY(h, L.hObserve.ensure(ego_b + desc_b));
    HIP_TRY(h, L.hOut.ensure(saf_b + sizeof(InstState) * (size_t)n));
    double *p_ego = (double *)L.hObserve.p;
    InstDesc *p_desc = (InstDesc *)((char *)L.hObserve.p + ego_b);
    for (int i = 0; i < n; ++i) {
        const double *e = ego5 + 5 * (size_t)i;
        p_ego[4 * i] = e[0]; p_ego[4 * i + 1] = e[1]; p_ego[4 * i + 2] = e[2]; p_ego[4 * i + 3] = e[3];
        InstDesc d = InstDesc();
        d.ego.x = e[0]; d.ego.y = e[1]; d.ego.yaw = e[2]; d.ego.v = e[3]; d.ego.a = e[4];
        const bool cached = prev_s && !std::isnan(prev_s[i]);
        d.ego.has_prev_s = cached ? 1 : 0;
        d.ego.prev_s = cached ? prev_s[i] : 0.0;
        d.scen = by_scen ? L.frame_scen[(size_t)i] : 0;
        p_desc[i] = d;
    }
    LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, p_ego, L.p_off, L.p_pos, L.p_vel, L.ego_radius, L.ped_radius,
                                h->sc[0].params.footprint_radius, L.use_footprint, (fot_safety *)L.hOut.p, st,
                                L.p_scen, L.dSafScen.as<SafetyScen>()));
    InstState *p_state = (InstState *)((char *)L.hOut.p + saf_b);
    PathSet ps = PathSet::single(spline_view(h, 0));
    if (by_scen) {                                               // the handle's path table, as a mixed plan batch passes it
        ps = PathSet();
        ps.table = h->dSplineTab.as<SplineView>();
        ps.mixed = 1;
        std::vector<uint8_t> used(h->sc.size(), 0);
        for (int i = 0; i < n; ++i) used[(size_t)L.frame_scen[(size_t)i]] = 1;
        for (size_t sc = 0; sc < used.size(); ++sc) if (used[sc]) ps.knots[ps.n_knots++] = h->sc[sc].spline.n;
    }
    LAUNCH_TRY(h, launch_frenet_state(h->dP.as<DevParams>(), ps, p_desc, p_state, n, MetaImport(), NanScan(), nullptr, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    L.observe_n = n;
    return FOT_OK;
}

}  // namespace

extern "C" {

int fot_loop_observe_begin(fot_handle *h, int32_t n, const double *ego5, const double *prev_s)
{
    // (the two-call form stays on scenario 0: what fot_loop_plan's frame leaves behind)
    return observe_begin_impl(h, n, ego5, prev_s);
}

int fot_loop_observe_end(fot_handle *h, fot_safety *safety_out, double *new_prev_s)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    const int n = L.observe_n;
    if (n < 0) return fail(h, FOT_ERR_INVALID, "no fot_loop_observe_begin to collect");
    L.observe_n = -1;
    if (n == 0) return FOT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (safety_out) std::memcpy(safety_out, L.hOut.p, sizeof(fot_safety) * (size_t)n);
    const InstState *p_state = (const InstState *)((const char *)L.hOut.p + align256(sizeof(fot_safety) * (size_t)n));
    if (new_prev_s) for (int i = 0; i < n; ++i) new_prev_s[i] = p_state[i].new_prev_s;
    return FOT_OK;
}

int fot_loop_observe(fot_handle *h, int32_t n, const double *ego5, const double *prev_s,
                     fot_safety *safety_out, double *new_prev_s)
{
    int rc = fot_loop_observe_begin(h, n, ego5, prev_s);
    return rc != FOT_OK ? rc : fot_loop_observe_end(h, safety_out, new_prev_s);
}

}  // extern "C"

// ---- the whole lock step of n episodes behind ONE call (SURVEY 8 f2 + f4) -------------------------------------------
namespace {

// FailSafeStateMachine._get_planner_config (state_machine.py:181-247): the planner configuration of `state` on the
// clearance ahead the machine last observed -> target speed, constraint overrides (NaN = absent), stop room (NaN = None)
void sm_config(const fot_loop_config &c, int state, double clear_ahead, double *target, fot_overrides *ov, double *stop)
{
    const bool fin = std::isfinite(clear_ahead), has_env = fin && c.envelope_decel > 0.0;
    const double v_env = std::sqrt(2.0 * c.envelope_decel * std::fmax((fin ? clear_ahead : 0.0) - c.envelope_standoff, 0.0));
    const double stop_room = fin ? std::fmax(clear_ahead - 0.2, 0.05) : NAN;
    *target = c.target_speed;
    ov->max_speed = ov->max_accel = ov->max_curvature = ov->max_lat_accel = NAN;
    *stop = NAN;
    if (state == 0) {
        if (has_env && v_env < c.target_speed) *target = v_env;
    } else if (state == 1) {
        const double t_ca = c.target_speed * c.caution_speed_mult;
        *target = has_env ? std::fmin(t_ca, v_env) : t_ca;
        if (has_env && v_env <= 0.0) *stop = stop_room;
        ov->max_accel = c.caution_accel; ov->max_speed = c.caution_speed;
    } else {
        *target = 0.0;
        ov->max_accel = c.emergency_accel; ov->max_lat_accel = c.emergency_lat_accel;
        if (c.envelope_decel > 0.0) *stop = stop_room;
    }
}

// FailSafeStateMachine.update (state_machine.py:116-179) of episode e: observe the metrics, then the transition
void sm_update(LoopEpisodes &E, int e, bool found, double clearance, double clearance_ahead, double speed)
{
    const fot_loop_config &c = E.cfg_of(e);
    E.clear[e] = clearance; E.clear_ahead[e] = clearance_ahead;
    const int st = E.state[e], fl = E.fails[e];
    const double trigger = c.trigger_clearance_caution + c.trigger_time_headway * std::fmax(speed, 0.0);
    if (st == 0) {
        if (!found) { E.state[e] = 1; E.fails[e] = fl + 1; }
        else if (trigger > 0.0 && clearance < trigger) { E.state[e] = 1; E.fails[e] = 0; }   // preventive escalation
        else E.fails[e] = 0;
    } else if (st == 1) {
        if (found && fl == 0) { if (clearance > std::fmax(c.clearance_caution, trigger)) E.state[e] = 0; }
        else if (!found) { E.state[e] = 2; E.fails[e] = fl + 1; }
        else E.fails[e] = 0;
    } else {
        if (found && clearance > c.clearance_emergency) E.state[e] = 1;
    }
}


// ---- the host side of one lock step, shared by fot_loop_step (records in pinned memory) and fot_loop_run (digests of
//      records that stay in HBM): Rec is fot_result or LoopDigest, which name the fields read here alike
void rec_sample1(const fot_result &r, double *g) { g[0] = r.x[1]; g[1] = r.y[1]; g[2] = r.yaw[1]; g[3] = r.v[1]; g[4] = r.a[1]; }
void rec_sample1(const LoopDigest &r, double *g) { g[0] = r.x1; g[1] = r.y1; g[2] = r.yaw1; g[3] = r.v1; g[4] = r.a1; }

int loop_max_levels(const fot_loop_config &c) { return 1 + c.max_replan < 3 ? 1 + c.max_replan : 3; }   // NORMAL -> CAUTION -> EMERGENCY, then no change

struct StepWork {
    std::vector<int> st0, n_lvl, next_rec, path_rec, keep;
    std::vector<double> speed, ego4, ego5n, jerk, cost;
    std::vector<fot_loop_request> req, more;
    std::vector<fot_safety> m;               // metrics of the current ego states
};

// level 0 of every episode: the configuration of its current state (issued on LAST step's clearance); request i plans
// against episode i of the frame
void step_level0(const LoopEpisodes &E, const int32_t *episode, int n, StepWork &W)
{
    W.st0.assign((size_t)n, 0); W.n_lvl.assign((size_t)n, 0);
    W.speed.assign((size_t)n, 0.0); W.ego4.assign(4 * (size_t)n, 0.0);
    W.req.assign((size_t)n, fot_loop_request());
    W.m.assign((size_t)n, fot_safety());
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);                   // (the episode's own scenario's constants)
        W.st0[i] = E.state[e];
        W.n_lvl[i] = std::min(3 - W.st0[i], loop_max_levels(c));
        const double *g = &E.ego[5 * (size_t)e];
        W.speed[i] = g[3];
        for (int k = 0; k < 4; ++k) W.ego4[4 * (size_t)i + k] = g[k];
        fot_loop_request &r = W.req[i];
        r = fot_loop_request();
        r.ego.x = g[0]; r.ego.y = g[1]; r.ego.yaw = g[2]; r.ego.v = g[3]; r.ego.a = g[4];
        r.ego.last_kappa = E.last_kappa[e];
        r.ego.has_prev_s = std::isnan(E.prev_s[e]) ? 0 : 1;
        r.ego.prev_s = std::isnan(E.prev_s[e]) ? 0.0 : E.prev_s[e];
        sm_config(c, W.st0[i], E.clear_ahead[e], &r.target_speed, &r.overrides, &r.max_stop_distance);
        r.episode = i;
    }
}

// episodes whose first attempt failed: every further escalation level they can reach, for ONE more launch (the
// configurations update(False, ...) would issue on THIS step's metrics, nearest-point cache chained); their records
// follow the n level-0 records
template <class Rec>
void step_escalations(const LoopEpisodes &E, const int32_t *episode, int n, const Rec *rec, StepWork &W)
{
    W.next_rec.assign((size_t)n, -1);
    W.more.clear();
    for (int i = 0; i < n; ++i) {
        if (rec[i].status == FOT_PLAN_OK || W.n_lvl[i] <= 1) continue;
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);
        W.next_rec[i] = n + (int)W.more.size();
        const double nps0 = rec[i].new_prev_s, p = std::isnan(nps0) ? E.prev_s[e] : nps0;
        for (int lvl = 1; lvl < W.n_lvl[i]; ++lvl) {
            fot_loop_request r = W.req[i];
            const bool chain = lvl > 1;
            r.ego.has_prev_s = chain ? FOT_PREV_S_CHAINED : (std::isnan(p) ? 0 : 1);
            r.ego.prev_s = (chain || std::isnan(p)) ? 0.0 : p;
            sm_config(c, W.st0[i] + lvl, W.m[i].clearance_ahead, &r.target_speed, &r.overrides, &r.max_stop_distance);
            W.more.push_back(r);
        }
    }
}

// replay of the retry loop (integrated_simulator.py:576-653) episode by episode, then the ego update (:655-676) or the
// emergency stop (:749-802): E moves on, W gets the followed record, its kept samples and cost, the jerk and the new egos
template <class Rec>
void step_resolve(LoopEpisodes &E, const int32_t *episode, int n, const Rec *rec, StepWork &W)
{
    W.path_rec.assign((size_t)n, -1); W.keep.assign((size_t)n, 0);
    W.jerk.assign((size_t)n, 0.0); W.cost.assign((size_t)n, 0.0); W.ego5n.assign(5 * (size_t)n, 0.0);
    auto adopt = [&](int i, int r) {                             // planner state after a plan() call
        const int e = episode[i];
        if (!std::isnan(rec[r].new_prev_s)) E.prev_s[e] = rec[r].new_prev_s;
        for (int k = 0; k < 8; ++k) E.stats[8 * (size_t)e + k] = rec[r].stats_valid ? rec[r].stats[k] : -1;
        if (rec[r].status == FOT_PLAN_OK) { E.last_kappa[e] = rec[r].new_last_kappa; W.path_rec[i] = r; }
    };
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);
        int cur = i, retries = 0;
        adopt(i, cur);
        bool found = rec[cur].status == FOT_PLAN_OK;
        int issued = W.st0[i];                                    // state of the configuration the attempt ran under
        sm_update(E, e, found, W.m[i].clearance, W.m[i].clearance_ahead, W.speed[i]);
        while (!found && E.state[e] != issued && retries < c.max_replan && retries + 1 < W.n_lvl[i]) {
            cur = retries == 0 ? W.next_rec[i] : cur + 1;
            ++retries;
            adopt(i, cur);
            const bool ok = rec[cur].status == FOT_PLAN_OK;
            found = found || ok;
            issued = E.state[e];
            if (!ok) sm_update(E, e, false, W.m[i].clearance, W.m[i].clearance_ahead, W.speed[i]);
        }
    }
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);
        double *g = &E.ego[5 * (size_t)e];
        const double old_a = g[4];
        const int r = W.path_rec[i];
        const int keep = r >= 0 ? rec[r].n_keep : 0;
        double jerk;
        if (keep >= 2) {
            rec_sample1(rec[r], g);
            jerk = (g[4] - old_a) / c.dt;
        } else {
            // the position integrates along the heading at the OLD speed; the deceleration is what stopping 0.2 m short
            // of the nearest pedestrian ahead needs, bounded to [max_accel, emergency_decel]
            const double v = g[3], clr = E.last_clearance[e];
            const double cap = std::isnan(c.emergency_decel) ? c.max_accel * 2.0 : c.emergency_decel;
            const double required = std::isfinite(clr) ? v * v / (2.0 * std::fmax(clr - 0.2, 0.05)) : cap;
            const double max_dec = std::fmin(std::fmax(required, c.max_accel), cap);
            const double nv = std::fmax(0.0, v - max_dec * c.dt), na = nv > 0.0 ? -max_dec : 0.0;
            g[0] = g[0] + v * std::cos(g[2]) * c.dt; g[1] = g[1] + v * std::sin(g[2]) * c.dt;
            g[3] = nv; g[4] = na;
            jerk = (na - old_a) / c.dt;
            E.last_kappa[e] = 0.0;                                // planner.reset_ego_curvature()
        }
        for (int k = 0; k < 5; ++k) W.ego5n[5 * (size_t)i + k] = g[k];
        W.jerk[i] = jerk; W.keep[i] = keep; W.cost[i] = rec[r >= 0 ? r : 0].cost;
    }
}

}  // namespace

extern "C" {

int fot_loop_begin(fot_handle *h, int32_t n_episodes, const fot_loop_config *cfg, const double *ego5)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_episodes < 0 || !cfg || (n_episodes > 0 && !ego5)) return fail(h, FOT_ERR_INVALID, "fot_loop_begin: arguments");
    if (!(cfg->dt > 0.0) || cfg->max_replan < 0 || cfg->max_replan > 8) return fail(h, FOT_ERR_INVALID, "fot_loop_begin: dt / max_replan");
    LoopEpisodes &E = h->loop.ep;
    const size_t n = (size_t)n_episodes;
    E.n = n_episodes; E.cfg = *cfg;
    E.scenarios = false; E.cfgs.clear(); E.use_fp.clear(); E.scen.clear();
    E.max_lvl = loop_max_levels(*cfg);
    h->loop.frame_scen.clear(); h->loop.p_scen = nullptr;
    E.ego.assign(ego5, ego5 + 5 * n);
    E.prev_s.assign(n, NAN); E.last_kappa.assign(n, 0.0); E.goal_prev_s.assign(n, NAN);
    E.last_clearance.assign(n, INFINITY); E.clear.assign(n, INFINITY); E.clear_ahead.assign(n, INFINITY);
    E.state.assign(n, 0); E.fails.assign(n, 0); E.stats.assign(8 * n, -1);
    h->loop.replay.set = false;                                  // (a new loop: the handle's clock, if it had one, is gone)
    h->loop.replay.sum.on = false;                               // ... and the summaries' accumulators with it
    h->loop.replay.smp.on = false;                               // ... and the sampler
    h->loop.replay.rec.on = false; h->loop.replay.rec.rec = nullptr;   // ... or the recorded samples
    h->loop.replay.sc.on = false;                                // ... and its scores
    h->loop.rep.mode = FOT_LOOP_PLAN_DISTRIBUTION; h->loop.rep.frame = false;
    h->loop.rep.last_best.assign(n, -1);
    return FOT_OK;
}

int fot_loop_begin_scenarios(fot_handle *h, int32_t n_episodes, int32_t n_cfg, const fot_loop_config *cfg,
                             const int32_t *use_footprint, const int32_t *slot_scenario, const double *ego5)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_episodes < 0 || n_cfg < 1 || !cfg || (n_episodes > 0 && (!ego5 || !slot_scenario)))
        return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: arguments");
    // --- everything is checked before anything changes
    int first = -1;
    for (int e = 0; e < n_episodes; ++e) {
        const int sc = slot_scenario[e];
        if (sc < 0 || sc >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: unknown scenario id");
        if (sc >= n_cfg) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: n_cfg is smaller than a slot's scenario id");
        if (!h->sc[(size_t)sc].has_path)
            return fail(h, FOT_ERR_NO_PATH_SET, "fot_loop_begin_scenarios: a slot's scenario has no path (fot_set_scenario_path_*)");
        const fot_loop_config &c = cfg[sc];
        if (!(c.dt > 0.0) || c.max_replan < 0 || c.max_replan > 8) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: dt / max_replan");
        if (first < 0) first = sc;
        if (c.dt != cfg[first].dt) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: the scenarios of a loop share dt");
    }
    if (first < 0) {                                             // no slot: nothing is in use but the first configuration
        first = 0;
        if (!(cfg[0].dt > 0.0) || cfg[0].max_replan < 0 || cfg[0].max_replan > 8) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: dt / max_replan");
    }
    const size_t n_sc = h->sc.size();
    std::vector<SafetyScen> tab(n_sc);
    for (size_t s = 0; s < n_sc; ++s) {
        tab[s].footprint_radius = h->sc[s].params.footprint_radius;
        tab[s].use_fp = ((int)s < n_cfg && use_footprint && use_footprint[s]) ? 1 : 0;
        tab[s]._pad = 0;
    }
    LoopState &L = h->loop;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // nothing may still be reading the old table
    HIP_TRY(h, L.dSafScen.ensure(sizeof(SafetyScen) * n_sc));
    HIP_TRY(h, hipMemcpy(L.dSafScen.p, tab.data(), sizeof(SafetyScen) * n_sc, hipMemcpyHostToDevice));
    // --- accepted
    LoopEpisodes &E = L.ep;
    const size_t n = (size_t)n_episodes;
    E.n = n_episodes; E.cfg = cfg[first];
    E.scenarios = true;
    E.cfgs.assign(cfg, cfg + n_cfg);
    E.use_fp.assign((size_t)n_cfg, 0);
    for (int s = 0; s < n_cfg; ++s) E.use_fp[(size_t)s] = use_footprint && use_footprint[s] ? 1 : 0;
    E.scen.assign(slot_scenario, slot_scenario + n);
    E.max_lvl = loop_max_levels(cfg[first]);
    for (size_t e = 0; e < n; ++e) E.max_lvl = std::max(E.max_lvl, loop_max_levels(cfg[E.scen[e]]));
    L.frame_scen.clear(); L.p_scen = nullptr; L.have_frame = false;
    E.ego.assign(ego5, ego5 + 5 * n);
    E.prev_s.assign(n, NAN); E.last_kappa.assign(n, 0.0); E.goal_prev_s.assign(n, NAN);
    E.last_clearance.assign(n, INFINITY); E.clear.assign(n, INFINITY); E.clear_ahead.assign(n, INFINITY);
    E.state.assign(n, 0); E.fails.assign(n, 0); E.stats.assign(8 * n, -1);
    L.replay.set = false;
    L.replay.sum.on = false;
    L.replay.smp.on = false;
    L.replay.rec.on = false; L.replay.rec.rec = nullptr;
    L.replay.sc.on = false;
    L.rep.mode = FOT_LOOP_PLAN_DISTRIBUTION; L.rep.frame = false;
    L.rep.last_best.assign(n, -1);
    return FOT_OK;
}

int fot_loop_step(fot_handle *h, const fot_loop_frame *frame, const int32_t *episode, fot_loop_step_out *out)
{
    if (!h) return FOT_ERR_INVALID;
    if (!frame || !out) return fail(h, FOT_ERR_INVALID, "fot_loop_step: frame / out");
    LoopState &L = h->loop;
    LoopEpisodes &E = L.ep;
    if (L.replay.set) return fail(h, FOT_ERR_INVALID, "fot_loop_step: a replay is set (fot_loop_run steps this handle; fot_loop_begin drops the replay)");
    const int n = frame->n_episodes;
    if (n < 0 || (n > 0 && !episode)) return fail(h, FOT_ERR_INVALID, "fot_loop_step: episode");
    out->records = nullptr; out->n_records = 0;
    if (n == 0) return FOT_OK;
    std::vector<uint8_t> seen((size_t)std::max(E.n, 1), 0);
    for (int i = 0; i < n; ++i) {
        if (episode[i] < 0 || episode[i] >= E.n || seen[(size_t)episode[i]]) return fail(h, FOT_ERR_INVALID, "fot_loop_step: episode slots must be distinct and below fot_loop_begin's count");
        seen[(size_t)episode[i]] = 1;
    }
    std::vector<int32_t> ep_scen;
    if (E.scenarios) {
        if (frame->dist_raw) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_step: a scenario loop takes the constant-velocity predictor only (no dist_raw)");
        ep_scen.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            ep_scen[(size_t)i] = E.scen[(size_t)episode[i]];
            if (ep_scen[(size_t)i] >= (int)h->sc.size() || !h->sc[(size_t)ep_scen[(size_t)i]].has_path)
                return fail(h, FOT_ERR_NO_PATH_SET, "fot_loop_step: a slot's scenario has no path");
        }
    }
    StepWork W;
    step_level0(E, episode, n, W);
    HIP_TRY(h, hipSetDevice(h->device));
    if (L.observe_n > 0) { HIP_TRY(h, hipStreamSynchronize(h->stream)); L.observe_n = -1; }
    // (all records of the step in one pinned block that must not move between the two plan calls)
    HIP_TRY(h, L.hRec.ensure(sizeof(fot_result) * (size_t)n * (size_t)E.max_lvl));
    fot_loop_frame fr = *frame;
    fr.ego = W.ego4.data();
    const fot_result *rec = nullptr;
    { int rc = loop_plan_impl(h, &fr, n, W.req.data(), W.m.data(), &rec, 0, E.scenarios ? ep_scen.data() : nullptr, episode); if (rc != FOT_OK) return rc; }
    rec = (const fot_result *)L.hRec.p;
    for (int i = 0; i < n; ++i) E.last_clearance[episode[i]] = W.m[i].clearance_ahead;
    step_escalations(E, episode, n, rec, W);
    int n_rec = n;
    if (!W.more.empty()) {
        const fot_result *unused = nullptr;
        int rc = loop_plan_impl(h, nullptr, (int)W.more.size(), W.more.data(), nullptr, &unused, n);
        if (rc != FOT_OK) return rc;
        rec = (const fot_result *)L.hRec.p;
        n_rec += (int)W.more.size();
    }
    step_resolve(E, episode, n, rec, W);
    for (int i = 0; i < n; ++i) {
        if (out->ego) for (int k = 0; k < 5; ++k) out->ego[5 * (size_t)i + k] = W.ego5n[5 * (size_t)i + k];
        if (out->jerk) out->jerk[i] = W.jerk[i];
        if (out->record) out->record[i] = W.path_rec[i];
        if (out->keep) out->keep[i] = W.keep[i];
        if (out->cost) out->cost[i] = W.cost[i];
    }
    // --- result metrics on the new ego states and the goal test's nearest point (:864-883): enqueued, the rest of the
    //     outputs filled while they run
    std::vector<double> gps((size_t)n);
    for (int i = 0; i < n; ++i) gps[i] = E.goal_prev_s[episode[i]];
    { int rc = fot_loop_observe_begin(h, n, W.ego5n.data(), gps.data()); if (rc != FOT_OK) return rc; }
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        if (out->state) out->state[i] = E.state[e];
        if (out->stats) for (int k = 0; k < 8; ++k) out->stats[8 * (size_t)i + k] = E.stats[8 * (size_t)e + k];
        if (out->before) out->before[i] = W.m[i];
    }
    std::vector<fot_safety> after((size_t)n);
    { int rc = fot_loop_observe_end(h, after.data(), gps.data()); if (rc != FOT_OK) return rc; }
    for (int i = 0; i < n; ++i) {
        E.goal_prev_s[episode[i]] = gps[i];
        if (out->after) out->after[i] = after[i];
        if (out->s_now) out->s_now[i] = gps[i];
    }
    out->records = rec;
    out->n_records = n_rec;
    return FOT_OK;
}

}  // extern "C"

// ---- whole replayed episodes: the recording resident in HBM, the lock steps run by the library ------------------------
namespace {

// Waits until the device has raised *word to seq (k_loop_digest / k_loop_history, in pinned memory); after 20 ms without
// it the stream is synchronised instead, as wait_records does.
int wait_word(fot_handle *h, const int32_t *word, int32_t seq, hipStream_t st)
{
    volatile const int32_t *w = (volatile const int32_t *)word;
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0; *w != seq;) {
        __builtin_ia32_pause();
        if ((++spins & 1023) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.02) {
            HIP_TRY(h, hipStreamSynchronize(st));
            return FOT_OK;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return FOT_OK;
}

int32_t next_seq(LoopReplay &R)
{
    if (++R.seq == 0) R.seq = 1;                                  // (0 is what a fresh word holds)
    return R.seq;
}

// the regions of LoopReplay::dFrame / hStage for up to n episodes and `rows` pedestrians
struct FrameLayout {
    size_t ped_b, ep_b, off_b, blk_b, pre_b, ego_b;
    FrameLayout(size_t n, size_t rows)
        : ped_b(align256(16 * std::max<size_t>(rows, 1))), ep_b(align256(4 * std::max<size_t>(rows, 1))),
          off_b(align256(4 * (n + 1))), blk_b(align256(8 * (n + 1))), pre_b(align256(4 * std::max<size_t>(n, 1))),
          ego_b(align256(32 * std::max<size_t>(n, 1))) {}
    size_t dev_bytes() const { return 4 * ped_b + ep_b + off_b + blk_b + pre_b + ego_b + pre_b; }
    // the stage block (hStage), which the host fills and k_loop_frame reads (FrameStage): its regions from `base` on and
    // its size; stage_bytes() is this walk's end
    struct Stage { int32_t *slot, *ped0; int64_t *blk; int32_t *prepend; double *ego; int32_t *scen; size_t bytes; };
    Stage stage(void *base) const
    {
        uintptr_t p = (uintptr_t)base;
        Stage s;
        s.slot = (int32_t *)p; p += pre_b;
        s.ped0 = (int32_t *)p; p += off_b;
        s.blk = (int64_t *)p; p += blk_b;
        s.prepend = (int32_t *)p; p += pre_b;
        s.ego = (double *)p; p += ego_b;
        s.scen = (int32_t *)p; p += pre_b;
        s.bytes = (size_t)(p - (uintptr_t)base);
        return s;
    }
    size_t stage_bytes() const { return stage(nullptr).bytes; }
    FrameDev dev(void *base) const
    {
        char *p = (char *)base;
        FrameDev f;
        f.pos = (double *)p; f.vel = (double *)(p + ped_b); f.last = (double *)(p + 2 * ped_b); f.prev = (double *)(p + 3 * ped_b);
        p += 4 * ped_b;
        f.ped_ep = (int32_t *)p; p += ep_b;
        f.ped0 = (int32_t *)p; p += off_b;
        f.blk = (int64_t *)p; p += blk_b;
        f.prepend = (int32_t *)p; p += pre_b;
        f.ego = (double *)p; p += ego_b;
        f.scen = (int32_t *)p;
        return f;
    }
};

// The launches of fot_sgan_sample behind its inputs, enqueue only (no copy from host memory, no synchronisation): all S
// samples of the N > 0 pedestrians of n_scenes scenes.  d_off [n_scenes + 1] and d_scene [N] (the scene of every pedestrian;
// nullptr unless the noise is per scene) are device memory, as are the tensors.
int sgan_enqueue(fot_handle *h, int n_scenes, int N, int S, const int32_t *d_off, const int32_t *d_scene, const float *d_obs,
                 const float *d_noise, float *d_out, hipStream_t st)
{
    fot_handle::Sgan &G = h->sgan;
    const fot_sgan_desc &d = G.desc;
    const int nd = d.noise_dim, noise_rows = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL ? n_scenes : N;
    const int E = d.embedding_dim, He = d.encoder_h_dim, Hd = d.decoder_h_dim, T = d.obs_len, L = d.pred_len;
    const bool pooled = sg_pooled(d), steps = sg_pool_steps(d), context = sg_has_context(d);
    const int nc = context ? Hd - nd : He;
    const size_t rows = (size_t)S * N;
    const float *img = G.dImg.as<float>();
    // once per pedestrian / scene: encoder, first pooling, context MLP
    HIP_TRY(h, G.dHenc.ensure(sizeof(float) * (size_t)N * He));
    LAUNCH_TRY(h, launch_sgan_encode(img, G.dev.enc, E, He, T, N, d_obs, G.dHenc.as<float>(), st));
    const int bp = pooled ? G.dev.pool.b_pad : 0;
    if (pooled) {
        HIP_TRY(h, G.dPool.ensure(sizeof(float) * (steps ? rows : (size_t)N) * bp));
        HIP_TRY(h, hipMemsetAsync(G.dPool.p, 0, sizeof(float) * (size_t)N * bp, st));
        LAUNCH_TRY(h, launch_sgan_pool(img, G.dev.pool, n_scenes, 1, N, d_off, G.dHenc.as<float>(),
                                       d_obs + 2 * (size_t)(T - 1) * N, G.dPool.as<float>(), st));
    }
    const float *d_ctx = G.dHenc.as<float>();
    if (context) {
        HIP_TRY(h, G.dCtx.ensure(sizeof(float) * (size_t)N * nc));
        LAUNCH_TRY(h, launch_sgan_mlp(img, G.dev.ctx, G.dHenc.as<float>(), He, G.dPool.as<float>(), pooled ? d.bottleneck_dim : 0, bp,
                                      N, G.dCtx.as<float>(), nc, st));
        d_ctx = G.dCtx.as<float>();
    }
    // once per sample: the decoder
    SgDecode a{};
    a.img = img; a.l = G.dev.dec; a.pos_w = G.dev.pos_w; a.pos_b = G.dev.pos_b;
    a.E = E; a.H = Hd; a.N = N; a.S = S; a.obs_len = T; a.pred_len = L;
    a.obs = d_obs; a.ctx = d_ctx; a.noise = d_noise; a.row_scene = d_scene;
    a.nc = nc; a.nd = nd; a.noise_rows = noise_rows; a.out = d_out;
    if (!steps) {
        a.t0 = 0; a.n_steps = L; a.init = 1; a.save = 0;
        LAUNCH_TRY(h, launch_sgan_decode(a, st));
    } else {
        HIP_TRY(h, G.dH.ensure(sizeof(float) * rows * Hd));
        HIP_TRY(h, G.dC.ensure(sizeof(float) * rows * Hd));
        HIP_TRY(h, G.dXY.ensure(sizeof(float) * rows * 6));
        a.h = G.dH.as<float>(); a.c = G.dC.as<float>();
        a.pos = G.dXY.as<float>(); a.rel = a.pos + rows * 2; a.cum = a.pos + rows * 4;
        a.n_steps = 1; a.save = 1;
        for (int t = 0; t < L; ++t) {
            a.t0 = t; a.init = t == 0;
            LAUNCH_TRY(h, launch_sgan_decode(a, st));
            if (t == L - 1) break;                                   // (the last step's pooled state is never read)
            HIP_TRY(h, hipMemsetAsync(G.dPool.p, 0, sizeof(float) * rows * bp, st));
            LAUNCH_TRY(h, launch_sgan_pool(img, G.dev.dpool, n_scenes, S, N, d_off, a.h, a.pos, G.dPool.as<float>(), st));
            LAUNCH_TRY(h, launch_sgan_mlp(img, G.dev.dmlp, a.h, Hd, G.dPool.as<float>(), d.bottleneck_dim, bp, (int64_t)rows, a.h, Hd, st));
        }
    }
    return FOT_OK;
}

// one lock step of the running slots `sel`; step k of the call (outputs row k)
int loop_run_step(fot_handle *h, const std::vector<int32_t> &sel, int k, fot_loop_run_out *out, double *d_hist_step)
{
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    LoopEpisodes &E = L.ep;
    const fot_loop_replay &C = R.cfg;
    hipStream_t st = h->stream;
    const int n = (int)sel.size(), n_slots = C.n_slots;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    // --- 1. pedestrians + observer
    R.clock.advance();
    const bool ready = R.clock.ready();
    const int f_cur = R.clock.frame, f_last = R.clock.last_frame(), f_prev = R.clock.prev_frame();
    const double stale = R.clock.staleness();
    if (out->frame) out->frame[k] = f_cur;
    if (out->obs_last_frame) out->obs_last_frame[k] = f_last;
    if (out->obs_prev_frame) out->obs_prev_frame[k] = f_prev;
    if (out->staleness) out->staleness[k] = stale;
    // --- 2. the frame of the running episodes: tables on the host, pedestrians on the device
    const FrameLayout FL((size_t)n_slots, (size_t)R.n_cols);
    const FrameLayout::Stage sg = FL.stage(R.hStage.p);
    StepWork W;
    step_level0(E, sel.data(), n, W);
    L.frame_scen.clear();
    if (E.scenarios) L.frame_scen.resize((size_t)n);
    L.ped_off.assign((size_t)n + 1, 0); L.blk_off.assign((size_t)n + 1, 0); L.t_len.assign((size_t)n, 1);
    L.dist_S = 0;
    L.rep.frame = false;
    const size_t row_doubles = 2 * (size_t)R.n_cols;
    int rows_run = 0;
    for (int i = 0; i < n; ++i) rows_run += R.ped_off[sel[i] + 1] - R.ped_off[sel[i]];
    const int dist_S = R.dist_S();
    const bool sampled = dist_S > 0 && ready && rows_run > 0;    // this step predicts with the sampler or the recording
    for (int i = 0; i < n; ++i) {
        const int e = sel[i], c0 = R.ped_off[e], P_e = R.ped_off[e + 1] - c0, nf = R.n_frames[e];
        int pre = 0;
        if (!sampled && ready && f_prev >= 0 && P_e > 0) {
            const double *cur = R.pos.data() + (size_t)replay_row(f_cur, nf) * row_doubles + 2 * (size_t)c0;
            const double *last = R.pos.data() + (size_t)replay_row(f_last, nf) * row_doubles + 2 * (size_t)c0;
            const double *prev = R.pos.data() + (size_t)replay_row(f_prev, nf) * row_doubles + 2 * (size_t)c0;
            pre = replay_prepend(P_e, last, prev, cur, C.rp.sgan_dt, C.rp.sim_dt, stale) ? 1 : 0;
        }
        if (sampled) pre = 1;                                    // (the current positions lead EVERY sample, :514-525)
        L.t_len[i] = ready ? R.n_dense + pre : 1;
        L.ped_off[i + 1] = L.ped_off[i] + P_e;
        L.blk_off[i + 1] = L.blk_off[i] + (int64_t)(sampled ? dist_S : 1) * P_e * L.t_len[i];
        sg.slot[i] = e; sg.ped0[i] = L.ped_off[i]; sg.blk[i] = L.blk_off[i]; sg.prepend[i] = pre;
        if (E.scenarios) sg.scen[i] = L.frame_scen[(size_t)i] = E.scen[(size_t)e];
        for (int q = 0; q < 4; ++q) sg.ego[4 * (size_t)i + q] = W.ego4[4 * (size_t)i + q];
    }
    sg.ped0[n] = L.ped_off[n]; sg.blk[n] = L.blk_off[n];
    const int rows = L.ped_off[n];
    ReplayView rv;
    rv.pos = R.dPos.as<double>(); rv.vel = R.dVel.as<double>();
    rv.slot_ped0 = R.dTab.as<int32_t>(); rv.slot_frames = R.dTab.as<int32_t>() + (n_slots + 1);
    rv.n_cols = R.n_cols;
    FrameStage fs;
    fs.slot = sg.slot; fs.ped0 = sg.ped0; fs.blk = sg.blk; fs.prepend = sg.prepend; fs.ego = sg.ego;
    fs.scen = E.scenarios ? sg.scen : nullptr;
    const FrameDev fd = FL.dev(R.dFrame.p);
    LAUNCH_TRY(h, launch_loop_frame(rv, fs, fd, n, f_cur, ready ? f_last : -1, ready ? f_prev : -1, st));
    L.p_off = fd.ped0; L.p_pos = fd.pos; L.p_vel = fd.vel;
    L.p_scen = E.scenarios ? fd.scen : nullptr;
    L.ego_radius = C.ego_radius; L.ped_radius = C.ped_radius; L.use_footprint = C.use_footprint;
    L.dyn_ptr = fd.pos;                                          // not ready: the current positions, T = 1
    if (sampled && R.rec.on) {
        // row k - first_step of the recording -> the step's raw samples of the running slots -> every episode's
        // [S][P_e][n_dense + 1][2] block, all in HBM behind k_loop_frame (fot_loop_run has checked that the row exists)
        LoopSamples &M = R.rec;
        if (M.sel != sel) {                                      // a slot dropped out (or the first step): the row -> column table
            int32_t *col = (int32_t *)M.hCol.p;                  // (no copy of an earlier step still reads it: every step ends
            sr_fill_columns(n, L.ped_off.data(), sel.data(), R.ped_off.data(), col);    //  with the host waiting for its word)
            HIP_TRY(h, hipMemcpyAsync(M.dCol.p, col, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, st));
            M.sel = sel;
        }
        LoopSampleRows a{};
        a.d.S = M.S; a.d.pred_len = C.pred_len; a.d.rows = rows; a.d.n_cols = R.n_cols;
        a.d.rec_row = (int64_t)R.steps[(size_t)sel[0]] - M.first_step;
        a.rec = M.rec; a.col = M.dCol.as<int32_t>(); a.out = M.dRaw.p; a.dtype = M.dtype;
        LAUNCH_TRY(h, launch_loop_sample_rows(a, st));
        L.dyn_ptr = L.dDyn.p;
        L.dist_S = M.S;
        LAUNCH_TRY(h, launch_resample(C.rp.sgan_dt, C.rp.sim_dt, stale, M.S, C.pred_len, rows, R.n_dense, 1, 1, 0, M.dRaw.p,
                                      M.dtype, fd.last, fd.pos, L.dDyn.p, FOT_F64, 0, st, fd.ped_ep, fd.ped0, fd.blk));
    } else if (sampled) {
        // window -> noise -> samples -> every episode's [S][P_e][n_dense + 1][2] block, all in HBM behind k_loop_frame
        LoopSampler &M = R.smp;
        const fot_sgan_desc &d = h->sgan.desc;
        const bool global_noise = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL;
        const int nd = d.noise_dim, noise_rows = global_noise ? n : rows;
        SgWindow w{};
        w.pos = rv.pos; w.slot_ped0 = rv.slot_ped0; w.slot_frames = rv.slot_frames;
        w.ped_ep = fd.ped_ep; w.ep_ped0 = fd.ped0; w.ep_slot = sg.slot;
        w.n_cols = R.n_cols; w.rows = rows; w.obs_len = d.obs_len;
        for (int j = 0; j < d.obs_len; ++j) w.frames.f[j] = R.clock.sample_frame[(size_t)j];
        w.out = M.dWin.as<float>();
        LAUNCH_TRY(h, launch_sgan_window(w, st));
        if (nd > 0) {
            const size_t cap = (size_t)R.n_cols + (size_t)n_slots;
            int32_t *t_slot = (int32_t *)M.hTab.p, *t_step = t_slot + cap, *t_idx = t_step + cap;
            int r = 0;
            for (int i = 0; i < n; ++i) {
                const int e = sel[i], P_e = R.ped_off[e + 1] - R.ped_off[e];
                for (int p = 0; p < (global_noise ? 1 : P_e); ++p, ++r) { t_slot[r] = e; t_step[r] = R.steps[(size_t)e]; t_idx[r] = p; }
            }
            SgNoise a{};
            a.seed = M.seed; a.kind = M.kind; a.S = M.S; a.rows = noise_rows; a.nd = nd; a.n_blk = (nd + 3) / 4;
            a.slot = t_slot; a.step = t_step; a.index = t_idx; a.out = (uint32_t *)M.dNoise.p;
            LAUNCH_TRY(h, launch_sgan_noise(a, st));
        }
        { int r = sgan_enqueue(h, n, rows, M.S, fd.ped0, global_noise && nd > 0 ? fd.ped_ep : nullptr, M.dWin.as<float>(),
                               M.dNoise.as<float>(), M.dRaw.as<float>(), st); if (r != FOT_OK) return r; }
        L.dyn_ptr = L.dDyn.p;
        L.dist_S = M.S;
        LAUNCH_TRY(h, launch_resample(C.rp.sgan_dt, C.rp.sim_dt, stale, M.S, C.pred_len, rows, R.n_dense, 1, 1, 0, M.dRaw.p,
                                      FOT_F32, fd.last, fd.pos, L.dDyn.p, FOT_F64, 0, st, fd.ped_ep, fd.ped0, fd.blk));
    } else if (ready && rows > 0) {
        L.dyn_ptr = L.dDyn.p;
        LAUNCH_TRY(h, launch_predict_cv_frame(C.rp.sgan_dt, C.rp.sim_dt, stale, rows, R.n_dense, fd, L.dDyn.as<double>(), st));
    }
    const bool scored = R.sc.on && sampled;                      // the step's distributions are scored where they lie
    const bool rep_on = L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE && sampled;   // ... the requests plan on one sample of each
    if (rep_on) {
        // the selection once, into the scores' tables where they are on: a scored and a planning loop read the same choice
        { int r = rep_ensure(h, n_slots, n_slots, (size_t)R.n_cols, R.n_dense + 1); if (r != FOT_OK) return r; }
        { int r = rep_enqueue(h, sg.slot, fd, n, dist_S, R.n_dense, R.sc.on ? R.sc.dDev.as<double>() : L.rep.dDev.as<double>(),
                              R.sc.on ? R.sc.dBest.as<int32_t>() : L.rep.dBest.as<int32_t>(),
                              (int32_t *)(R.sc.on ? R.sc.hBest.p : L.rep.hBest.p), st); if (r != FOT_OK) return r; }
        L.rep.frame = true; L.rep.T = R.n_dense + 1;
    } else if (scored)                                           // every episode's representative sample
        LAUNCH_TRY(h, launch_loop_best_sample(sg.slot, fd, L.dDyn.as<double>(), n, dist_S, R.n_dense, R.sc.dDev.as<double>(),
                                              R.sc.dBest.as<int32_t>(), (int32_t *)R.sc.hBest.p, st));
    if (R.sum.on || R.sc.on)                                     // this step's row of every running slot's ring
        LAUNCH_TRY(h, launch_loop_pred_error(rv, sg.slot, fd, L.dDyn.as<double>(), n, ready && rows > 0 ? 1 : 0, f_cur,
                                             R.steps[(size_t)sel[0]], R.sum.shape, R.sum.dRing.as<double>(),
                                             R.sum.dRingP.as<int32_t>(), R.sum.dTotals.as<SummaryTotals>(), st,
                                             scored ? R.sc.dBest.as<int32_t>() : nullptr));
    if (scored && R.sc.std_ok) {                                 // one origin per running episode, the truth from the recording
        PredOriginDev *pd = (PredOriginDev *)R.sc.hDesc.p;
        const double scott = ps_scott(dist_S);
        for (int i = 0; i < n; ++i)
            pd[i] = PredOriginDev{ L.blk_off[(size_t)i], (int64_t)L.ped_off[(size_t)i], scott, dist_S,
                                   L.ped_off[(size_t)i + 1] - L.ped_off[(size_t)i], R.n_dense + 1, 0, 1, 0 };
        LAUNCH_TRY(h, launch_loop_score_truth(rv, sg.slot, fd, rows, f_cur, R.sc.stride, C.pred_len, R.sc.dTruth.as<double>(), st));
        LAUNCH_TRY(h, launch_pred_scores(pd, n, L.dDyn.p, FOT_F64, R.sc.stride, C.pred_len, R.sc.dTruth.as<double>(),
                                         (fot_pred_score *)R.sc.hRec.p, st));
    }
    LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, fd.ego, fd.ped0, fd.pos, fd.vel, L.ego_radius, L.ped_radius,
                                h->sc[0].params.footprint_radius, L.use_footprint, (fot_safety *)L.hOut.p, st,
                                L.p_scen, L.dSafScen.as<SafetyScen>()));
    L.have_frame = true; L.observe_n = -1;
    // --- 3. level 0 of every episode; the records stay in HBM, the host reads their digests
    fot_result *d_rec = R.dRec.as<fot_result>();
    LoopDigest *dig = (LoopDigest *)R.hDigest.p;
    int32_t *word = (int32_t *)R.hWord.p;
    { int rc = loop_enqueue_requests(h, n, W.req.data(), d_rec, st, false); if (rc != FOT_OK) return rc; }
    int32_t seq = next_seq(R);
    LAUNCH_TRY(h, launch_loop_digest(d_rec, n, dig, word, seq, st));
    { int rc = wait_word(h, word, seq, st); if (rc != FOT_OK) return rc; }
    std::memcpy(W.m.data(), L.hOut.p, sizeof(fot_safety) * (size_t)n);   // (k_safety ran ahead of the plan on this stream)
    if (R.sc.on) {                                               // ... and so did the step's scores: into the slots' rings
        LoopScores &Q = R.sc;
        const fot_pred_score *rec = (const fot_pred_score *)Q.hRec.p;
        const int32_t *best = (const int32_t *)Q.hBest.p;
        std::fill(Q.last_best.begin(), Q.last_best.end(), -1);
        for (int i = 0; i < n; ++i) {
            const int e = sel[i];
            PredScoreTerms t = ps_zero(dist_S);                  // (no prediction, or no horizon that could ever complete)
            if (scored && Q.std_ok) {
                const fot_pred_score &r = rec[i];
                t.ade_scene = r.ade_scene; t.fde_scene = r.fde_scene; t.ade_agent_sum = r.ade_agent_sum;
                t.fde_agent_sum = r.fde_agent_sum; t.log_lik_sum = r.log_lik_sum;
                t.n_peds = r.n_peds; t.n_samples = r.n_samples; t.nll_count = r.nll_count; t.flags = r.flags;
            }
            score_ring_push(Q.fold[(size_t)e], Q.ring.data() + (size_t)e * (size_t)Q.H, Q.H, R.steps[(size_t)e], t);
            if (scored && L.ped_off[(size_t)i + 1] > L.ped_off[(size_t)i]) Q.last_best[(size_t)e] = best[e];
        }
    }
    if (L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE) {            // the choice the step planned on (fot_loop_last_best_sample)
        const int32_t *best = (const int32_t *)(R.sc.on ? R.sc.hBest.p : L.rep.hBest.p);
        std::fill(L.rep.last_best.begin(), L.rep.last_best.end(), -1);
        for (int i = 0; rep_on && i < n; ++i)
            if (L.ped_off[(size_t)i + 1] > L.ped_off[(size_t)i]) L.rep.last_best[(size_t)sel[i]] = best[sel[i]];
        L.rep.run_best.insert(L.rep.run_best.end(), L.rep.last_best.begin(), L.rep.last_best.end());
    }
    for (int i = 0; i < n; ++i) E.last_clearance[sel[i]] = W.m[i].clearance_ahead;
    step_escalations(E, sel.data(), n, dig, W);
    if (!W.more.empty()) {
        const int n_more = (int)W.more.size();
        int rc = loop_enqueue_requests(h, n_more, W.more.data(), d_rec + n, st, false);
        if (rc != FOT_OK) return rc;
        seq = next_seq(R);
        LAUNCH_TRY(h, launch_loop_digest(d_rec + n, n_more, dig + n, word, seq, st));
        rc = wait_word(h, word, seq, st);
        if (rc != FOT_OK) return rc;
    }
    // --- 4. retry loop, ego update; 5. metrics of the new states + the goal test's nearest point
    step_resolve(E, sel.data(), n, dig, W);
    std::vector<double> gps((size_t)n);
    for (int i = 0; i < n; ++i) gps[i] = E.goal_prev_s[sel[i]];
    { int rc = fot_loop_observe_begin(h, n, W.ego5n.data(), gps.data()); if (rc != FOT_OK) return rc; }
    // the followed paths into the history block, and the word that tells the host the step's results are there
    int32_t *t_src = (int32_t *)R.hHistTab.p, *t_slot = t_src + n_slots;
    for (int i = 0; i < n; ++i) { t_src[i] = W.path_rec[i]; t_slot[i] = sel[i]; }
    seq = next_seq(R);
    LAUNCH_TRY(h, launch_loop_history(d_rec, n, t_src, t_slot, d_hist_step, n_slots, h->sc[0].P.n_total, word + 16, seq, st));
    { int rc = wait_word(h, word + 16, seq, st); if (rc != FOT_OK) return rc; }
    L.observe_n = -1;
    const fot_safety *after = (const fot_safety *)L.hOut.p;
    const InstState *p_state = (const InstState *)((const char *)L.hOut.p + align256(sizeof(fot_safety) * (size_t)n));
    const size_t row = (size_t)k * (size_t)n_slots;
    if (out->followed) for (int e = 0; e < n_slots; ++e) out->followed[row + e] = -1;
    for (int i = 0; i < n; ++i) {
        const int e = sel[i];
        const size_t o = row + (size_t)e;
        const double s_now = p_state[i].new_prev_s;
        E.goal_prev_s[e] = s_now;
        if (out->ego) for (int q = 0; q < 5; ++q) out->ego[5 * o + q] = W.ego5n[5 * (size_t)i + q];
        if (out->jerk) out->jerk[o] = W.jerk[i];
        if (out->state) out->state[o] = E.state[e];
        if (out->stats) for (int q = 0; q < 8; ++q) out->stats[8 * o + q] = E.stats[8 * (size_t)e + q];
        if (out->followed) out->followed[o] = W.path_rec[i] >= 0 ? 1 : 0;
        if (out->keep) out->keep[o] = W.keep[i];
        if (out->cost) out->cost[o] = W.cost[i];
        if (out->after) out->after[o] = after[i];
        if (out->s_now) out->s_now[o] = s_now;
        R.steps[e] += 1;
        if (R.sum.on || R.sc.on) {                               // (calculate_aggregate_metrics, metrics.py:279-308)
            LoopSummaryAcc &A = R.sum;
            const double aj = std::fabs(W.jerk[i]), aa = std::fabs(W.ego5n[5 * (size_t)i + 4]), ttc = after[i].ttc;
            A.min_dist[e] = std::fmin(A.min_dist[e], after[i].min_distance);
            if (after[i].collision != 0) A.collisions[e] += 1;
            if (ttc > 0.0 && ttc != INFINITY && ttc < A.min_ttc[e]) A.min_ttc[e] = ttc;
            A.max_jerk[e] = std::fmax(A.max_jerk[e], aj); A.sum_jerk[e] += aj; A.sum_jerk2[e] += aj * aj;
            A.max_accel[e] = std::fmax(A.max_accel[e], aa); A.sum_accel[e] += aa;
        }
        // the goal of a scenario loop's slot: the end of its own scenario's path (its spline's last knot)
        const double s_end = E.scenarios ? h->sc[(size_t)E.scen[(size_t)e]].spline.s.back() : C.s_end;
        R.termination[e] = replay_termination(after[i].collision, s_end, s_now, C.goal_distance);
        if (R.termination[e] != 0) R.alive[e] = 0;
    }
    return FOT_OK;
}

int summary_arm(fot_handle *h, int num_samples, int stride);     // (below fot_loop_summary_enable)

}  // namespace

extern "C" {

int fot_loop_set_replay(fot_handle *h, const fot_loop_replay *rp)
{
    if (!h) return FOT_ERR_INVALID;
    if (!rp) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: replay is NULL");
    LoopState &L = h->loop;
    const LoopEpisodes &E = L.ep;
    if (!E.scenarios && !h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    for (int e = 0; E.scenarios && e < E.n; ++e)
        if (E.scen[(size_t)e] >= (int)h->sc.size() || !h->sc[(size_t)E.scen[(size_t)e]].has_path)
            return fail(h, FOT_ERR_NO_PATH_SET, "fot_loop_set_replay: a slot's scenario has no path");
    if (!(E.cfg.dt > 0.0)) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: fot_loop_begin comes first");
    const int n = rp->n_slots;
    if (n != E.n) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: n_slots differs from fot_loop_begin's episode count");
    if (!rp->ped_off || (n > 0 && !rp->n_frames) || rp->n_frames_max < 1 || rp->warmup_frames < 0)
        return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: ped_off / n_frames / n_frames_max / warmup_frames");
    for (int i = 0; i < n; ++i)
        if (rp->ped_off[i + 1] < rp->ped_off[i] || rp->ped_off[0] != 0)
            return fail(h, FOT_ERR_INVALID, "ped_off must start at 0 and be non-decreasing");
    for (int i = 0; i < n; ++i)
        if (rp->n_frames[i] < 1 || rp->n_frames[i] > rp->n_frames_max)
            return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: every slot needs 1 .. n_frames_max recorded frames");
    const size_t cols = n > 0 ? (size_t)rp->ped_off[n] : 0;
    if (cols > 0 && (!rp->pos || !rp->vel)) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: NULL recording");
    if (rp->obs_len < 2) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: obs_len < 2 (the predictor needs two samples)");
    if (!(rp->rp.sim_dt > 0.0) || !(rp->rp.sgan_dt > 0.0) || rp->pred_len < 1)
        return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: predictor parameters");
    if (rp->pred_len > FOT_MAX_PRED_LEN) return fail(h, FOT_ERR_UNSUPPORTED, "pred_len > FOT_MAX_PRED_LEN");
    const int n_dense = resample_n_dense(rp->rp.sgan_dt, rp->rp.sim_dt, rp->rp.plan_horizon, rp->pred_len);
    if (n_dense + 1 > FOT_MAX_NT) return fail(h, FOT_ERR_UNSUPPORTED, "more than FOT_MAX_NT time steps");
    // --- accepted: everything the steps need is allocated here, so that no block grows (and moves) inside a run
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // nothing may still read what is replaced below
    LoopReplay &R = L.replay;
    R.set = false;
    R.sum.on = false;                                            // (a new recording: summaries are enabled again, if wanted)
    R.smp.on = false;                                            // ... and so is a sampler
    R.rec.on = false; R.rec.rec = nullptr;                       // ... or recorded samples
    R.sc.on = false;                                             // ... and its scores
    const size_t rec_doubles = (size_t)rp->n_frames_max * cols * 2;
    const int max_lvl = E.max_lvl;
    const size_t n_rec = (size_t)std::max(n, 1) * (size_t)max_lvl;
    const FrameLayout FL((size_t)n, cols);
    HIP_TRY(h, R.dPos.ensure(sizeof(double) * std::max<size_t>(rec_doubles, 2)));
    HIP_TRY(h, R.dVel.ensure(sizeof(double) * std::max<size_t>(rec_doubles, 2)));
    HIP_TRY(h, R.dTab.ensure(sizeof(int32_t) * (2 * (size_t)n + 1)));
    HIP_TRY(h, R.dFrame.ensure(FL.dev_bytes()));
    HIP_TRY(h, R.dRec.ensure_zeroed(sizeof(fot_result) * n_rec));
    HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * std::max<size_t>(cols, 1) * (size_t)(n_dense + 1)));
    HIP_TRY(h, R.hStage.ensure(FL.stage_bytes()));
    HIP_TRY(h, R.hDigest.ensure(sizeof(LoopDigest) * n_rec));
    HIP_TRY(h, R.hHistTab.ensure(sizeof(int32_t) * 2 * (size_t)std::max(n, 1)));
    HIP_TRY(h, R.hWord.ensure(sizeof(int32_t) * 32));
    HIP_TRY(h, L.hOut.ensure(align256(sizeof(fot_safety) * (size_t)std::max(n, 1)) + sizeof(InstState) * (size_t)std::max(n, 1)));
    HIP_TRY(h, L.hObserve.ensure(align256(sizeof(double) * 4 * (size_t)std::max(n, 1)) + align256(sizeof(InstDesc) * (size_t)std::max(n, 1))));
    if (E.scenarios) { int r = ensure_scen_static(h, (int)n_rec, h->stream); if (r != FOT_OK) return r; }
    if (rec_doubles) {
        HIP_TRY(h, hipMemcpy(R.dPos.p, rp->pos, sizeof(double) * rec_doubles, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(R.dVel.p, rp->vel, sizeof(double) * rec_doubles, hipMemcpyHostToDevice));
    }
    std::vector<int32_t> tab(2 * (size_t)n + 1);
    for (int i = 0; i <= n; ++i) tab[(size_t)i] = rp->ped_off[i];
    for (int i = 0; i < n; ++i) tab[(size_t)n + 1 + (size_t)i] = rp->n_frames[i];
    HIP_TRY(h, hipMemcpy(R.dTab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice));
    R.cfg = *rp;
    R.cfg.ped_off = nullptr; R.cfg.n_frames = nullptr; R.cfg.pos = nullptr; R.cfg.vel = nullptr;
    R.n_cols = (int)cols; R.n_dense = n_dense; R.max_lvl = max_lvl;
    R.ped_off.assign(rp->ped_off, rp->ped_off + n + 1);
    R.n_frames.assign(rp->n_frames, rp->n_frames + n);
    R.pos.assign(rp->pos, rp->pos + rec_doubles);
    R.vel.clear();                                               // (the host needs the positions only: the prepend test)
    R.alive.assign((size_t)n, 1); R.steps.assign((size_t)n, 0); R.termination.assign((size_t)n, 0);
    R.clock.reset(rp->obs_len, rp->rp.sim_dt, rp->rp.sgan_dt);
    for (int i = 0; i < rp->warmup_frames; ++i) R.clock.advance();   // fills the observer (integrated_simulator.py:406-422)
    L.have_frame = false; L.observe_n = -1;
    R.set = true;
    return FOT_OK;
}

int fot_loop_summary_enable(fot_handle *h, int32_t on, int32_t num_samples)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: fot_loop_set_replay comes first");
    const int n = R.cfg.n_slots;
    for (int e = 0; e < n; ++e)
        if (R.steps[(size_t)e] != 0) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: the run has begun (enable between fot_loop_set_replay and the first step)");
    if (R.clock.frame != R.cfg.warmup_frames) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: the run has begun (enable between fot_loop_set_replay and the first step)");
    LoopSummaryAcc &A = R.sum;
    if (!on) { A.on = false; return FOT_OK; }
    if (R.smp.on) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_summary_enable: a sampler is set (fot_loop_set_sampler): the prediction-error ring reads the constant-velocity tensor");
    if (R.rec.on) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_summary_enable: recorded samples are set (fot_loop_set_samples): the prediction-error ring reads the constant-velocity tensor");
    if (num_samples < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: num_samples < 1");
    const int stride = summary_stride(R.cfg.rp.sgan_dt, R.cfg.rp.sim_dt);
    if (stride < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: sgan_dt must be a multiple of sim_dt");
    { int r = summary_arm(h, num_samples, stride); if (r != FOT_OK) return r; }
    A.on = true;
    return FOT_OK;
}

}  // extern "C"

namespace {

// The prediction-error ring, its totals and the host's accumulators of a run that has not begun: allocated and zeroed
// (a row with count 0 contributes nothing).  Leaves LoopSummaryAcc::on as it is.
int summary_arm(fot_handle *h, int num_samples, int stride)
{
    LoopReplay &R = h->loop.replay;
    LoopSummaryAcc &A = R.sum;
    const size_t ns = (size_t)std::max(R.cfg.n_slots, 1), nd = (size_t)R.n_dense;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, A.dRing.ensure(sizeof(double) * ns * nd * nd));
    HIP_TRY(h, A.dRingP.ensure(sizeof(int32_t) * ns * nd));
    HIP_TRY(h, A.dTotals.ensure(sizeof(SummaryTotals) * ns));
    HIP_TRY(h, A.hOut.ensure(sizeof(fot_loop_summary) * ns));
    HIP_TRY(h, A.hSteps.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, hipMemsetAsync(A.dRing.p, 0, sizeof(double) * ns * nd * nd, h->stream));
    HIP_TRY(h, hipMemsetAsync(A.dRingP.p, 0, sizeof(int32_t) * ns * nd, h->stream));
    HIP_TRY(h, hipMemsetAsync(A.dTotals.p, 0, sizeof(SummaryTotals) * ns, h->stream));
    A.shape = summary_shape(R.n_dense, stride, R.cfg.pred_len);
    A.num_samples = num_samples;
    A.min_dist.assign(ns, INFINITY); A.min_ttc.assign(ns, INFINITY);
    A.max_jerk.assign(ns, 0.0); A.sum_jerk.assign(ns, 0.0); A.sum_jerk2.assign(ns, 0.0);
    A.max_accel.assign(ns, 0.0); A.sum_accel.assign(ns, 0.0); A.collisions.assign(ns, 0);
    return FOT_OK;
}

// one record per slot from the ring, its totals and the host's accumulators (n_slots > 0, checked by the caller)
int summaries_fill(fot_handle *h, int32_t n_slots, fot_loop_summary *out)
{
    LoopReplay &R = h->loop.replay;
    LoopSummaryAcc &A = R.sum;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int32_t *steps = (int32_t *)A.hSteps.p;
    fot_loop_summary *rec = (fot_loop_summary *)A.hOut.p;
    for (int e = 0; e < n_slots; ++e) steps[e] = R.steps[(size_t)e];
    // totals + the ring's rows with their truncated horizons -> the prediction-error keys; nothing in HBM changes
    LAUNCH_TRY(h, launch_loop_summary(A.shape, A.dRing.as<double>(), A.dRingP.as<int32_t>(), A.dTotals.as<SummaryTotals>(),
                                      steps, n_slots, A.num_samples, rec, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const double dt = R.cfg.rp.sim_dt;
    for (int e = 0; e < n_slots; ++e) {
        fot_loop_summary s = rec[e];
        const int L = R.steps[(size_t)e];
        // an empty history: the reference's values (metrics.py:301-308)
        s.min_dist = L > 0 ? A.min_dist[e] : 0.0;
        s.min_ttc = A.min_ttc[e];
        s.collision_count = A.collisions[e];
        s.max_jerk = A.max_jerk[e]; s.max_accel = A.max_accel[e];
        s.mean_jerk = L > 0 ? A.sum_jerk[e] / (double)L : 0.0;
        s.rms_jerk = L > 0 ? std::sqrt(A.sum_jerk2[e] / (double)L) : 0.0;
        s.mean_accel = L > 0 ? A.sum_accel[e] / (double)L : 0.0;
        s.steps = L; s.termination = R.termination[(size_t)e]; s._pad = 0;
        s.total_time = (double)L * dt;
        out[e] = s;
    }
    return FOT_OK;
}

}  // namespace

extern "C" {

int fot_loop_summaries(fot_handle *h, int32_t n_slots, fot_loop_summary *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: fot_loop_set_replay comes first");
    if (!R.sum.on) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: summaries are not enabled (fot_loop_summary_enable)");
    if (n_slots != R.cfg.n_slots) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: n_slots differs from the loop's");
    if (n_slots > 0 && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: out is NULL");
    if (n_slots == 0) return FOT_OK;
    return summaries_fill(h, n_slots, out);
}

int fot_loop_scores_enable(fot_handle *h, int32_t on)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: fot_loop_set_replay comes first");
    if (!R.smp.on && !R.rec.on)
        return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: no sampler or recording is set (fot_loop_set_sampler / fot_loop_set_samples comes first)");
    const int n = R.cfg.n_slots;
    bool begun = R.clock.frame != R.cfg.warmup_frames;
    for (int e = 0; e < n; ++e) begun = begun || R.steps[(size_t)e] != 0;
    if (begun) return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: the run has begun (enable between fot_loop_set_sampler / fot_loop_set_samples and the first step)");
    LoopScores &Q = R.sc;
    if (!on) { Q.on = false; return FOT_OK; }
    const int stride = summary_stride(R.cfg.rp.sgan_dt, R.cfg.rp.sim_dt);
    if (stride < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: sgan_dt must be a multiple of sim_dt");
    // --- accepted: everything the mode needs is allocated here
    Q.on = false;
    { int r = summary_arm(h, R.dist_S(), stride); if (r != FOT_OK) return r; }
    const size_t ns = (size_t)std::max(n, 1), cols = (size_t)std::max(R.n_cols, 1), E = (size_t)R.cfg.pred_len;
    HIP_TRY(h, Q.dBest.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, Q.dDev.ensure(sizeof(double) * ns * FOT_MAX_SAMPLES));
    HIP_TRY(h, Q.dTruth.ensure(sizeof(double) * 2 * cols * E));
    HIP_TRY(h, Q.hBest.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, Q.hDesc.ensure(sizeof(PredOriginDev) * ns));
    HIP_TRY(h, Q.hRec.ensure(sizeof(fot_pred_score) * ns));
    HIP_TRY(h, hipMemsetAsync(Q.dBest.p, 0xFF, sizeof(int32_t) * ns, h->stream));
    HIP_TRY(h, hipMemsetAsync(Q.dDev.p, 0, sizeof(double) * ns * FOT_MAX_SAMPLES, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::memset(Q.hBest.p, 0xFF, sizeof(int32_t) * ns);
    std::memset(Q.hRec.p, 0, sizeof(fot_pred_score) * ns);
    Q.stride = stride; Q.H = stride * R.cfg.pred_len;
    Q.std_ok = ps_horizon_fits(stride, R.cfg.pred_len, R.n_dense + 1, 1);
    Q.ring.assign(ns * (size_t)Q.H, ps_zero(R.dist_S()));
    Q.fold.assign(ns, score_fold_zero());
    Q.last_best.assign(ns, -1);
    Q.on = true;
    return FOT_OK;
}

int fot_loop_score_summaries(fot_handle *h, int32_t n_slots, fot_loop_summary *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set || !R.sc.on) return fail(h, FOT_ERR_INVALID, "fot_loop_score_summaries: scores are not enabled (fot_loop_scores_enable)");
    if (n_slots != R.cfg.n_slots) return fail(h, FOT_ERR_INVALID, "fot_loop_score_summaries: n_slots differs from the loop's");
    if (n_slots > 0 && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_score_summaries: out is NULL");
    if (n_slots == 0) return FOT_OK;
    { int r = summaries_fill(h, n_slots, out); if (r != FOT_OK) return r; }
    // the ring's standard-cadence totals are the representative sample's: the best-of-N and KDE keys are the fold's
    for (int e = 0; e < n_slots; ++e) {
        double m[5];
        int32_t samples = 0;
        const ScoreFold &F = R.sc.fold[(size_t)e];
        score_fold_means(F, m, &samples);
        fot_loop_summary &s = out[e];
        s.ade = m[0]; s.fde = m[1]; s.ade_per_agent = m[2]; s.fde_per_agent = m[3]; s.nll = m[4];
        s.ade_eval_count = (int32_t)F.count; s.nll_eval_count = (int32_t)F.nll_count; s.pred_samples = samples;
    }
    return FOT_OK;
}

int fot_loop_last_best_sample(fot_handle *h, int32_t n_slots, int32_t *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    const LoopRep &Q = h->loop.rep;
    const bool scores = R.set && R.sc.on, planned = Q.mode == FOT_LOOP_PLAN_REPRESENTATIVE;
    if (!scores && !planned)
        return fail(h, FOT_ERR_INVALID, "fot_loop_last_best_sample: scores are not enabled (fot_loop_scores_enable)");
    // (a stepwise loop planning on the representative sample: the slots of fot_loop_begin)
    if (n_slots != (scores ? R.cfg.n_slots : h->loop.ep.n)) return fail(h, FOT_ERR_INVALID, "fot_loop_last_best_sample: n_slots differs from the loop's");
    if (n_slots > 0 && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_last_best_sample: out is NULL");
    for (int e = 0; e < n_slots; ++e) out[e] = scores ? R.sc.last_best[(size_t)e] : Q.last_best[(size_t)e];
    return FOT_OK;
}

int fot_loop_plan_sample(fot_handle *h, int32_t mode)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    if (mode != FOT_LOOP_PLAN_DISTRIBUTION && mode != FOT_LOOP_PLAN_REPRESENTATIVE)
        return fail(h, FOT_ERR_INVALID, "fot_loop_plan_sample: mode is FOT_LOOP_PLAN_DISTRIBUTION or FOT_LOOP_PLAN_REPRESENTATIVE");
    if (!(L.ep.cfg.dt > 0.0)) return fail(h, FOT_ERR_INVALID, "fot_loop_plan_sample: fot_loop_begin comes first");
    if (L.ep.scenarios) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_plan_sample: a scenario loop plans against no distribution");
    if (R.set) {
        bool begun = R.clock.frame != R.cfg.warmup_frames;
        for (int e = 0; e < R.cfg.n_slots; ++e) begun = begun || R.steps[(size_t)e] != 0;
        if (begun) return fail(h, FOT_ERR_INVALID, "fot_loop_plan_sample: the run has begun (choose between fot_loop_set_replay and the first step)");
    }
    if (mode == FOT_LOOP_PLAN_REPRESENTATIVE && R.set) {
        // a resident run: everything its steps need is allocated here, so that no block grows (and moves) inside the run
        HIP_TRY(h, hipSetDevice(h->device));
        int r = rep_ensure(h, R.cfg.n_slots, R.cfg.n_slots, (size_t)R.n_cols, R.n_dense + 1);
        if (r != FOT_OK) return r;
    }
    L.rep.mode = mode;
    L.rep.frame = false;                                         // (the next frame decides what its requests plan against)
    L.rep.last_best.assign((size_t)L.ep.n, -1);
    L.rep.run_best.clear();
    return FOT_OK;
}

int fot_loop_run_best_samples(fot_handle *h, int32_t n_steps, int32_t n_slots, int32_t *out)
{
    if (!h) return FOT_ERR_INVALID;
    const LoopState &L = h->loop;
    if (!L.replay.set || L.rep.mode != FOT_LOOP_PLAN_REPRESENTATIVE)
        return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: no resident run plans on the representative sample (fot_loop_plan_sample)");
    if (n_slots != L.replay.cfg.n_slots) return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: n_slots differs from the loop's");
    if (n_steps < 0 || (size_t)n_steps * (size_t)n_slots != L.rep.run_best.size())
        return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: n_steps differs from the steps of the most recent fot_loop_run");
    if (!L.rep.run_best.empty() && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: out is NULL");
    if (!L.rep.run_best.empty()) std::memcpy(out, L.rep.run_best.data(), sizeof(int32_t) * L.rep.run_best.size());
    return FOT_OK;
}

int fot_debug_loop_block(fot_handle *h, int32_t episode, int32_t cap_points, double *xy, int32_t *P, int32_t *T,
                         int32_t *prepended)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    if (!L.have_frame) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: no frame");
    const int n_ep = (int)L.ped_off.size() - 1;
    if (episode < 0 || episode >= n_ep) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: episode out of range");
    if (cap_points < 0 || (cap_points > 0 && !xy)) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: cap_points / xy");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t e = (size_t)episode;
    const int P_e = L.ped_off[e + 1] - L.ped_off[e];
    int t_len = 0, pre = -1;
    int64_t first = 0, n_pts = 0;
    const void *base = nullptr;
    if (L.rep.frame) {
        t_len = L.rep.T; first = (int64_t)L.ped_off[e] * t_len; n_pts = (int64_t)P_e * t_len; base = L.rep.dBlk.p;
        if (P_e > 0) pre = ((const int32_t *)L.rep.hPre.p)[e];
    } else {
        t_len = L.t_len[e]; first = L.blk_off[e]; n_pts = (int64_t)std::max(L.dist_S, 1) * P_e * t_len; base = L.dyn_ptr;
    }
    if (P) *P = P_e;
    if (T) *T = t_len;
    if (prepended) *prepended = pre;
    if (n_pts > cap_points) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: the block holds more than cap_points points");
    if (n_pts > 0 && base)
        HIP_TRY(h, hipMemcpy(xy, (const double *)base + 2 * first, sizeof(double) * 2 * (size_t)n_pts, hipMemcpyDefault));
    return FOT_OK;
}

// Shared body of fot_prediction_scores and fot_loop_prediction_scores: `tensor` is device memory, or host memory of
// tensor_bytes bytes to be copied first (tensor_bytes > 0).  Checks every origin before anything is enqueued or written.
static int prediction_scores_impl(fot_handle *h, const char *who, int32_t n, const fot_pred_origin *desc, const void *tensor,
                                  size_t tensor_bytes, int32_t dtype, int32_t stride, int32_t E, const double *truth,
                                  fot_pred_score *out, hipStream_t st)
{
    const std::string w(who);
    if (stride < 1 || E < 1) return fail(h, FOT_ERR_INVALID, w + ": stride and E must be positive");
    if (E > FOT_MAX_PRED_LEN) return fail(h, FOT_ERR_UNSUPPORTED, w + ": E > FOT_MAX_PRED_LEN");
    size_t rows = 0;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const fot_pred_origin &d = desc[i];
        if (d.S < 1 || d.P < 0 || d.T < 1 || d.offset < 0 || (d.skip != 0 && d.skip != 1) ||
            (d.layout != 0 && d.layout != FOT_DYN_LAYOUT_TSP))
            return fail(h, FOT_ERR_INVALID, w + ": an origin's S / P / T / offset / skip / layout");
        if (!ps_horizon_fits(stride, E, d.T, d.skip))
            return fail(h, FOT_ERR_INVALID, w + ": stride E - 1 reaches past an origin's dense track (T - skip)");
        if (d.S > FOT_MAX_SAMPLES) return fail(h, FOT_ERR_UNSUPPORTED, w + ": S > FOT_MAX_SAMPLES");
        rows += (size_t)d.P;
        any |= d.P > 0;
    }
    if (!out || (any && (!truth || !tensor))) return fail(h, FOT_ERR_INVALID, w + ": NULL tensor / truth / out");
    if (!any) {                                                    // nothing for the device to do
        for (int i = 0; i < n; ++i) {
            const PredScoreTerms z = ps_zero(desc[i].S);
            out[i] = fot_pred_score{ 0.0, 0.0, 0.0, 0.0, 0.0, z.n_peds, z.n_samples, z.nll_count, z.flags };
        }
        return FOT_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const size_t desc_b = align256(sizeof(PredOriginDev) * (size_t)n), truth_b = sizeof(double) * 2 * rows * (size_t)E;
    HIP_TRY(h, h->hScoreIn.ensure(desc_b + truth_b));
    HIP_TRY(h, h->hScoreOut.ensure(sizeof(fot_pred_score) * (size_t)n));
    PredOriginDev *pd = (PredOriginDev *)h->hScoreIn.p;
    double *pt = (double *)((char *)h->hScoreIn.p + desc_b);
    size_t row = 0;
    for (int i = 0; i < n; ++i) {
        const fot_pred_origin &d = desc[i];
        pd[i] = PredOriginDev{ d.offset, (int64_t)row, ps_scott(d.S), d.S, d.P, d.T, d.layout == FOT_DYN_LAYOUT_TSP ? 1 : 0,
                               d.skip, 0 };
        row += (size_t)d.P;
    }
    std::memcpy(pt, truth, truth_b);
    const void *d_tensor = tensor;
    if (tensor_bytes > 0) {
        HIP_TRY(h, h->dScoreT.ensure(tensor_bytes));
        HIP_TRY(h, hipMemcpyAsync(h->dScoreT.p, tensor, tensor_bytes, hipMemcpyHostToDevice, st));
        d_tensor = h->dScoreT.p;
    }
    LAUNCH_TRY(h, launch_pred_scores(pd, n, d_tensor, dtype, stride, E, pt, (fot_pred_score *)h->hScoreOut.p, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));
    std::memcpy(out, h->hScoreOut.p, sizeof(fot_pred_score) * (size_t)n);
    return FOT_OK;
}

int fot_prediction_scores(fot_handle *h, int32_t n_origins, const fot_pred_origin *desc, const void *tensor, int32_t dtype,
                          int32_t on_device, int32_t stride, int32_t E, const double *truth, fot_pred_score *out,
                          void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_origins < 0 || (n_origins > 0 && !desc)) return fail(h, FOT_ERR_INVALID, "fot_prediction_scores: n_origins / desc");
    if (dtype != FOT_F32 && dtype != FOT_F64) return fail(h, FOT_ERR_INVALID, "fot_prediction_scores: dtype");
    if (n_origins == 0) return FOT_OK;
    size_t bytes = 0;
    if (!on_device) {                                              // the host tensor up to the end of the last block
        int64_t end = 0;
        for (int i = 0; i < n_origins; ++i)
            if (desc[i].offset >= 0 && desc[i].S > 0 && desc[i].P > 0 && desc[i].T > 0)
                end = std::max(end, desc[i].offset + (int64_t)desc[i].S * desc[i].P * desc[i].T);
        bytes = (dtype == FOT_F32 ? 4 : 8) * 2 * (size_t)end;
    }
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return prediction_scores_impl(h, "fot_prediction_scores", n_origins, desc, tensor, bytes, dtype, stride, E, truth, out, st);
}

int fot_loop_prediction_scores(fot_handle *h, int32_t n_episodes, int32_t stride, int32_t E, const double *truth,
                               fot_pred_score *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    if (L.replay.set) return fail(h, FOT_ERR_INVALID, "fot_loop_prediction_scores: a replay is set (fot_loop_run owns the handle's tensor)");
    if (!L.have_frame || L.dist_S < 1)
        return fail(h, FOT_ERR_INVALID, "fot_loop_prediction_scores: the last frame carried no distribution (fot_loop_frame.dist_raw)");
    if (n_episodes != (int)L.ped_off.size() - 1) return fail(h, FOT_ERR_INVALID, "fot_loop_prediction_scores: n_episodes differs from the frame's");
    if (n_episodes == 0) return FOT_OK;
    std::vector<fot_pred_origin> desc((size_t)n_episodes);
    for (int e = 0; e < n_episodes; ++e)
        desc[(size_t)e] = fot_pred_origin{ L.blk_off[(size_t)e], L.dist_S, L.ped_off[(size_t)e + 1] - L.ped_off[(size_t)e],
                                           L.t_len[(size_t)e], 0, 1, 0 };
    // (a frame without pedestrians left no tensor: every P is 0 and none is read)
    return prediction_scores_impl(h, "fot_loop_prediction_scores", n_episodes, desc.data(), L.dDyn.p, 0, FOT_F64, stride, E,
                                  truth, out, h->stream);
}

// ---- Social-GAN sample generation (include/fot.h; kernels: fot_sgan.hip, arithmetic: fot_sgan.hpp) ------------------------
int fot_sgan_weight_count(const fot_sgan_desc *desc, int64_t *n)
{
    if (!desc || !n) return fail(nullptr, FOT_ERR_INVALID, "fot_sgan_weight_count: desc / n is NULL");
    std::string why;
    const int rc = sg_check_desc(*desc, why);
    if (rc != FOT_OK) return fail(nullptr, rc, why);
    *n = sg_blob_layout(*desc).total;
    return FOT_OK;
}

int fot_sgan_load(fot_handle *h, const fot_sgan_desc *desc, int64_t n, const float *weights)
{
    if (!h) return FOT_ERR_INVALID;
    if (!desc || !weights) return fail(h, FOT_ERR_INVALID, "fot_sgan_load: desc / weights is NULL");
    if (h->loop.replay.set && h->loop.replay.smp.on) return fail(h, FOT_ERR_INVALID, "fot_sgan_load: the resident loop's sampler uses the model (fot_loop_set_sampler)");
    std::string why;
    const int rc = sg_check_desc(*desc, why);
    if (rc != FOT_OK) return fail(h, rc, why);
    if (n != sg_blob_layout(*desc).total) return fail(h, FOT_ERR_INVALID, "fot_sgan_load: n is not fot_sgan_weight_count of the descriptor");
    std::vector<float> img;
    const SgDev dev = sg_dev_image(*desc, weights, img);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                   // (a sample call of the model before this one is synchronous anyway)
    fot_handle::Sgan &G = h->sgan;
    G.loaded = false;
    HIP_TRY(h, G.dImg.ensure(sizeof(float) * img.size()));
    HIP_TRY(h, hipMemcpy(G.dImg.p, img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice));
    G.desc = *desc;
    G.dev = dev;
    G.loaded = true;
    return FOT_OK;
}

int fot_sgan_unload(fot_handle *h)
{
    if (!h) return FOT_ERR_INVALID;
    if (h->loop.replay.set && h->loop.replay.smp.on) return fail(h, FOT_ERR_INVALID, "fot_sgan_unload: the resident loop's sampler uses the model (fot_loop_set_sampler)");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->sgan.loaded = false;
    h->sgan.release();
    return FOT_OK;
}

int fot_sgan_sample(fot_handle *h, int32_t n_scenes, const int32_t *ped_off, const void *obs, int32_t S, const void *noise,
                    int32_t flags, void *out, void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    fot_handle::Sgan &G = h->sgan;
    if (!G.loaded) return fail(h, FOT_ERR_INVALID, "fot_sgan_sample: no model loaded (fot_sgan_load)");
    if (n_scenes < 0 || !ped_off) return fail(h, FOT_ERR_INVALID, "fot_sgan_sample: n_scenes / ped_off (one offset even for no scene)");
    if (S < 1) return fail(h, FOT_ERR_INVALID, "fot_sgan_sample: S < 1");
    if (flags & ~(FOT_OUT_DEVICE | FOT_SGAN_OBS_DEVICE | FOT_SGAN_NOISE_DEVICE)) return fail(h, FOT_ERR_INVALID, "fot_sgan_sample: flags");
    if (ped_off[0] != 0) return fail(h, FOT_ERR_INVALID, "fot_sgan_sample: ped_off must start at 0 and be non-decreasing");
    int widest = 0;
    for (int i = 0; i < n_scenes; ++i) {
        if (ped_off[i + 1] < ped_off[i]) return fail(h, FOT_ERR_INVALID, "fot_sgan_sample: ped_off must start at 0 and be non-decreasing");
        widest = std::max(widest, ped_off[i + 1] - ped_off[i]);
    }
    if (S > FOT_MAX_SAMPLES) return fail(h, FOT_ERR_UNSUPPORTED, "fot_sgan_sample: S > FOT_MAX_SAMPLES");
    if (widest > FOT_SGAN_MAX_PEDS) return fail(h, FOT_ERR_UNSUPPORTED, "fot_sgan_sample: a scene of more than FOT_SGAN_MAX_PEDS pedestrians");
    const fot_sgan_desc &d = G.desc;
    const int N = ped_off[n_scenes];
    const bool global_noise = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL;
    const int nd = d.noise_dim, noise_rows = global_noise ? n_scenes : N;
    if (N == 0) return FOT_OK;
    if (!obs || !out || (nd > 0 && !noise)) return fail(h, FOT_ERR_INVALID, "fot_sgan_sample: NULL tensor");
    const int T = d.obs_len, L = d.pred_len;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const size_t obs_bytes = sizeof(float) * 2 * (size_t)T * N, noise_bytes = sizeof(float) * (size_t)S * noise_rows * nd;
    const size_t out_bytes = sizeof(float) * 2 * (size_t)S * L * N;
    // the offsets and, for noise per scene, every pedestrian's scene
    std::vector<int32_t> scene_of;
    HIP_TRY(h, G.dOff.ensure(sizeof(int32_t) * ((size_t)n_scenes + 1)));
    HIP_TRY(h, hipMemcpyAsync(G.dOff.p, ped_off, sizeof(int32_t) * ((size_t)n_scenes + 1), hipMemcpyHostToDevice, st));
    if (global_noise && nd > 0) {
        scene_of.resize((size_t)N);
        for (int i = 0; i < n_scenes; ++i) std::fill(scene_of.begin() + ped_off[i], scene_of.begin() + ped_off[i + 1], i);
        HIP_TRY(h, G.dScene.ensure(sizeof(int32_t) * (size_t)N));
        HIP_TRY(h, hipMemcpyAsync(G.dScene.p, scene_of.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, st));
    }
    const float *d_obs = (const float *)obs, *d_noise = (const float *)noise;
    if (!(flags & FOT_SGAN_OBS_DEVICE)) {
        HIP_TRY(h, G.dObs.ensure(obs_bytes));
        HIP_TRY(h, hipMemcpyAsync(G.dObs.p, obs, obs_bytes, hipMemcpyHostToDevice, st));
        d_obs = G.dObs.as<float>();
    }
    if (nd > 0 && !(flags & FOT_SGAN_NOISE_DEVICE)) {
        HIP_TRY(h, G.dNoise.ensure(noise_bytes));
        HIP_TRY(h, hipMemcpyAsync(G.dNoise.p, noise, noise_bytes, hipMemcpyHostToDevice, st));
        d_noise = G.dNoise.as<float>();
    }
    float *d_out = (float *)out;
    if (!(flags & FOT_OUT_DEVICE)) { HIP_TRY(h, G.dOut.ensure(out_bytes)); d_out = G.dOut.as<float>(); }
    { int r = sgan_enqueue(h, n_scenes, N, S, G.dOff.as<int32_t>(), global_noise && nd > 0 ? G.dScene.as<int32_t>() : nullptr, d_obs,
                           d_noise, d_out, st); if (r != FOT_OK) return r; }
    if (!(flags & FOT_OUT_DEVICE)) HIP_TRY(h, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

int fot_sgan_noise(fot_handle *h, uint64_t seed, int32_t kind, int32_t S, int32_t rows, int32_t noise_dim,
                   const int32_t *row_slot, const int32_t *row_step, const int32_t *row_index, int32_t flags, void *out,
                   void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (kind < 0 || kind >= FOT_NOISE_KINDS) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: kind");
    if (flags & ~FOT_OUT_DEVICE) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: flags");
    if (S < 1 || rows < 0 || noise_dim < 0) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: S < 1 / rows < 0 / noise_dim < 0");
    if (S > FOT_MAX_SAMPLES) return fail(h, FOT_ERR_UNSUPPORTED, "fot_sgan_noise: S > FOT_MAX_SAMPLES");
    if (rows == 0 || noise_dim == 0) return FOT_OK;
    if (!row_slot || !row_step || !row_index || !out) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: NULL table / out");
    for (int r = 0; r < rows; ++r)
        if (row_slot[r] < 0 || row_step[r] < 0 || row_index[r] < 0 || row_index[r] > 0xFFFF)
            return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: a negative table entry, or a row_index above 65535");
    fot_handle::Sgan &G = h->sgan;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const size_t n_out = (size_t)S * (size_t)rows * (size_t)noise_dim;
    HIP_TRY(h, hipStreamSynchronize(h->stream));                  // (the tables' block: nothing of an earlier call reads it)
    HIP_TRY(h, G.hTab.ensure(sizeof(int32_t) * 3 * (size_t)rows));
    uint32_t *d_out = (uint32_t *)out;
    if (!(flags & FOT_OUT_DEVICE)) { HIP_TRY(h, G.dNoise.ensure(sizeof(uint32_t) * n_out)); d_out = (uint32_t *)G.dNoise.p; }
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    int32_t *t = (int32_t *)G.hTab.p;
    std::memcpy(t, row_slot, sizeof(int32_t) * (size_t)rows);
    std::memcpy(t + rows, row_step, sizeof(int32_t) * (size_t)rows);
    std::memcpy(t + 2 * (size_t)rows, row_index, sizeof(int32_t) * (size_t)rows);
    SgNoise a{};
    a.seed = seed; a.kind = kind; a.S = S; a.rows = rows; a.nd = noise_dim; a.n_blk = (noise_dim + 3) / 4;
    a.slot = t; a.step = t + rows; a.index = t + 2 * (size_t)rows; a.out = d_out;
    LAUNCH_TRY(h, launch_sgan_noise(a, st));
    if (!(flags & FOT_OUT_DEVICE)) HIP_TRY(h, hipMemcpyAsync(out, d_out, sizeof(uint32_t) * n_out, hipMemcpyDeviceToHost, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

int fot_loop_set_sampler(fot_handle *h, int32_t S, uint64_t seed, int32_t kind)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    fot_handle::Sgan &G = h->sgan;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_set_sampler: fot_loop_set_replay comes first");
    if (!G.loaded) return fail(h, FOT_ERR_INVALID, "fot_loop_set_sampler: no model loaded (fot_sgan_load)");
    if (R.rec.on) return fail(h, FOT_ERR_INVALID, "fot_loop_set_sampler: recorded samples are set (fot_loop_set_samples): one predictor per run");
    const int n = R.cfg.n_slots;
    bool begun = R.clock.frame != R.cfg.warmup_frames;
    for (int e = 0; e < n; ++e) begun = begun || R.steps[(size_t)e] != 0;
    if (begun) return fail(h, FOT_ERR_INVALID, "fot_loop_set_sampler: the run has begun (set it between fot_loop_set_replay and the first step)");
    if (S < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_set_sampler: S < 1");
    if (kind != FOT_NOISE_GAUSSIAN && kind != FOT_NOISE_UNIFORM_SYM)
        return fail(h, FOT_ERR_INVALID, "fot_loop_set_sampler: kind is FOT_NOISE_GAUSSIAN or FOT_NOISE_UNIFORM_SYM");
    const fot_sgan_desc &d = G.desc;
    if (d.obs_len != R.cfg.obs_len || d.pred_len != R.cfg.pred_len)
        return fail(h, FOT_ERR_INVALID, "fot_loop_set_sampler: the model's obs_len / pred_len differ from the replay's");
    if (S > FOT_MAX_SAMPLES) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_set_sampler: S > FOT_MAX_SAMPLES");
    for (int e = 0; e < n; ++e)
        if (R.ped_off[(size_t)e + 1] - R.ped_off[(size_t)e] > FOT_SGAN_MAX_PEDS)
            return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_set_sampler: a slot of more than FOT_SGAN_MAX_PEDS pedestrians");
    if (L.ep.scenarios) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_set_sampler: a scenario loop plans against no distribution");
    if (R.sum.on) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_set_sampler: summaries are enabled (their prediction-error ring reads the constant-velocity tensor)");
    // --- accepted: everything a step needs is allocated here, so that no block grows (and moves) inside a run
    LoopSampler &M = R.smp;
    const size_t N = std::max<size_t>((size_t)R.n_cols, 1), rows = (size_t)S * N, ns = (size_t)std::max(n, 1);
    const int bp = sg_pooled(d) ? G.dev.pool.b_pad : 0;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    M.on = false;
    HIP_TRY(h, M.dWin.ensure(sizeof(float) * 2 * (size_t)d.obs_len * N));
    HIP_TRY(h, M.dNoise.ensure(sizeof(float) * (size_t)S * std::max(N, ns) * (size_t)std::max(d.noise_dim, 1)));
    HIP_TRY(h, M.dRaw.ensure(sizeof(float) * 2 * (size_t)S * (size_t)d.pred_len * N));
    HIP_TRY(h, M.hTab.ensure(sizeof(int32_t) * 3 * (N + ns)));
    HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * rows * (size_t)(R.n_dense + 1)));
    HIP_TRY(h, G.dHenc.ensure(sizeof(float) * N * (size_t)d.encoder_h_dim));
    if (bp > 0) HIP_TRY(h, G.dPool.ensure(sizeof(float) * (sg_pool_steps(d) ? rows : N) * (size_t)bp));
    if (sg_has_context(d)) HIP_TRY(h, G.dCtx.ensure(sizeof(float) * N * (size_t)std::max(d.decoder_h_dim - d.noise_dim, 1)));
    if (sg_pool_steps(d)) {
        HIP_TRY(h, G.dH.ensure(sizeof(float) * rows * (size_t)d.decoder_h_dim));
        HIP_TRY(h, G.dC.ensure(sizeof(float) * rows * (size_t)d.decoder_h_dim));
        HIP_TRY(h, G.dXY.ensure(sizeof(float) * rows * 6));
    }
    M.S = S; M.seed = seed; M.kind = kind;
    M.on = true;
    R.sc.on = false;                                             // (a new sampler: its scores are enabled again, if wanted)
    return FOT_OK;
}

int fot_loop_set_samples(fot_handle *h, int32_t S, int32_t n_steps, int32_t first_step, const void *samples, int32_t dtype,
                         int32_t flags)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: fot_loop_set_replay comes first");
    if (R.smp.on) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: a sampler is set (fot_loop_set_sampler): one predictor per run");
    const int n = R.cfg.n_slots;
    bool begun = R.clock.frame != R.cfg.warmup_frames;
    for (int e = 0; e < n; ++e) begun = begun || R.steps[(size_t)e] != 0;
    if (begun) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: the run has begun (set it between fot_loop_set_replay and the first step)");
    if (S < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: S < 1");
    if (n_steps < 1 || first_step < 0) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: n_steps < 1 / first_step < 0");
    if (!samples) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: samples is NULL");
    if (dtype != FOT_F32 && dtype != FOT_F64) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: dtype is FOT_F32 or FOT_F64");
    if (flags & ~FOT_OUT_DEVICE) return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: flags");
    const size_t elem = dtype == FOT_F32 ? 2 * sizeof(float) : 2 * sizeof(double);
    // (the gather moves whole elements of two coordinates; hipMalloc allocations and their slices along any axis
    //  but the last are aligned to one)
    if ((flags & FOT_OUT_DEVICE) && (uintptr_t)samples % elem != 0)
        return fail(h, FOT_ERR_INVALID, "fot_loop_set_samples: device samples must be aligned to one [x, y] element");
    if (S > FOT_MAX_SAMPLES) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_set_samples: S > FOT_MAX_SAMPLES");
    if (L.ep.scenarios) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_set_samples: a scenario loop plans against no distribution");
    if (R.sum.on) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_set_samples: summaries are enabled (their prediction-error ring reads the constant-velocity tensor)");
    // --- accepted: everything a step needs is allocated here, so that no block grows (and moves) inside a run
    LoopSamples &M = R.rec;
    const size_t N = std::max<size_t>((size_t)R.n_cols, 1), rows = (size_t)S * N;
    const size_t rec_bytes = (size_t)sr_rec_elems(n_steps, S, R.cfg.pred_len, R.n_cols) * elem;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    M.on = false; M.rec = nullptr;
    HIP_TRY(h, M.dRaw.ensure(elem * (size_t)S * (size_t)R.cfg.pred_len * N));
    HIP_TRY(h, M.dCol.ensure(sizeof(int32_t) * N));
    HIP_TRY(h, M.hCol.ensure(sizeof(int32_t) * N));
    HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * rows * (size_t)(R.n_dense + 1)));
    if (flags & FOT_OUT_DEVICE) {
        M.rec = samples;                                         // used in place, never written
    } else {
        HIP_TRY(h, M.dRec.ensure(std::max<size_t>(rec_bytes, elem)));
        if (rec_bytes) HIP_TRY(h, hipMemcpy(M.dRec.p, samples, rec_bytes, hipMemcpyHostToDevice));
        M.rec = M.dRec.p;
    }
    M.S = S; M.n_steps = n_steps; M.first_step = first_step; M.dtype = dtype;
    M.sel.clear();
    M.on = true;
    R.sc.on = false;                                             // (a new recording: its scores are enabled again, if wanted)
    return FOT_OK;
}

int fot_loop_run(fot_handle *h, int32_t max_steps, fot_loop_run_out *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_run: fot_loop_set_replay comes first");
    if (max_steps < 0 || !out) return fail(h, FOT_ERR_INVALID, "fot_loop_run: max_steps / out");
    const int n_slots = R.cfg.n_slots;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const size_t step_doubles = 15 * (size_t)n_slots * (size_t)h->sc[0].P.n_total;
    const bool keep_paths = out->paths != nullptr && step_doubles > 0 && max_steps > 0;
    if (keep_paths) {
        HIP_TRY(h, R.dHist.ensure(sizeof(double) * step_doubles * (size_t)max_steps));
        HIP_TRY(h, hipMemsetAsync(R.dHist.p, 0, sizeof(double) * step_doubles * (size_t)max_steps, st));
    }
    int done = 0;
    std::vector<int32_t> sel;
    L.rep.run_best.clear();
    for (; done < max_steps; ++done) {
        sel.clear();
        for (int e = 0; e < n_slots; ++e) if (R.alive[(size_t)e]) sel.push_back(e);
        if (sel.empty()) break;
        if (R.rec.on) {
            // Would this step predict, and is its row recorded?  The clock does not depend on the ego, so the host knows
            // before anything of the step is enqueued: a step outside the recording is not run.
            ReplayClock next = R.clock;
            next.advance();
            int rows_run = 0;
            for (int32_t e : sel) rows_run += R.ped_off[(size_t)e + 1] - R.ped_off[(size_t)e];
            const int step = R.steps[(size_t)sel[0]];
            if (next.ready() && rows_run > 0 && !sr_covers(R.rec.first_step, R.rec.n_steps, step)) {
                if (done > 0) break;
                return fail(h, FOT_ERR_INVALID, "fot_loop_run: lock step " + std::to_string(step) + " predicts, but the recorded samples (fot_loop_set_samples) cover steps " +
                                                std::to_string(R.rec.first_step) + " .. " + std::to_string((int64_t)R.rec.first_step + R.rec.n_steps - 1));
            }
        }
        int rc = loop_run_step(h, sel, done, out, keep_paths ? R.dHist.as<double>() + step_doubles * (size_t)done : nullptr);
        if (rc != FOT_OK) return rc;
    }
    if (done > 0) { int r = order_end(h, st); if (r != FOT_OK) return r; }
    if (keep_paths && done > 0) {                                // the call's history block, in one copy
        HIP_TRY(h, hipMemcpyAsync(out->paths, R.dHist.p, sizeof(double) * step_doubles * (size_t)done, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    for (int e = 0; e < n_slots; ++e) {
        if (out->steps) out->steps[e] = R.steps[(size_t)e];
        if (out->termination) out->termination[e] = R.termination[(size_t)e];
    }
    return done;
}

}  // extern "C"

extern "C" {

int fot_gather_paths(const fot_result *records, int32_t n, const int32_t *index, int32_t kmax, double *out)
{
    if (n < 0 || kmax < 0 || kmax > FOT_MAX_NT) return FOT_ERR_INVALID;
    if (n == 0 || kmax == 0) return FOT_OK;
    if (!records || !index || !out) return FOT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        if (index[i] < 0) return FOT_ERR_INVALID;
        const double *src = records[index[i]].t;                 // the 15 arrays lie back to back (static_assert below)
        for (int f = 0; f < 15; ++f)
            std::memcpy(out + ((size_t)f * n + i) * kmax, src + (size_t)f * FOT_MAX_NT, sizeof(double) * (size_t)kmax);
    }
    return FOT_OK;
}

int fot_profile_enable(fot_handle *h, int on)
{
    if (!h) return FOT_ERR_INVALID;
    if (!on && h->prof_on) { int r = prof_drain(h); if (r != FOT_OK) return r; }
    h->prof_on = on != 0;
    return FOT_OK;
}

int fot_profile_read(fot_handle *h, int reset, int32_t cap, int32_t *launches, double *total_ms)
{
    if (!h) return FOT_ERR_INVALID;
    if (cap < 0) return fail(h, FOT_ERR_INVALID, "fot_profile_read: cap < 0");
    HIP_TRY(h, hipSetDevice(h->device));
    int r = prof_drain(h);
    if (r != FOT_OK) return r;
    for (int k = 0; k < FOT_PROFILE_KERNELS; ++k) {
        if (k < cap) {                                           // (never past the caller's arrays, whatever header it was built with)
            if (launches) launches[k] = h->prof_launches[k];
            if (total_ms) total_ms[k] = h->prof_ms[k];
        }
        if (reset) { h->prof_launches[k] = 0; h->prof_ms[k] = 0.0; }
    }
    return FOT_PROFILE_KERNELS;
}

const char *fot_profile_kernel_name(int index)
{
    return index >= 0 && index < FOT_PROFILE_KERNELS ? kKernelNames[index] : "";
}

int fot_synchronize(fot_handle *h)
{
    if (!h) return FOT_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FOT_OK;
}

int fot_plan_batch(fot_handle *h, const fot_batch *batch, fot_result *out)
{
    return fot_plan_batch_scenarios(h, batch, nullptr, out);
}

int fot_plan_batch_scenarios(fot_handle *h, const fot_batch *batch, const int32_t *scenario, fot_result *out)
{
    if (!h) return FOT_ERR_INVALID;
    if (!batch) return fail(h, FOT_ERR_INVALID, "batch is NULL");
    if (batch->n_inst > 0 && !out) return fail(h, FOT_ERR_INVALID, "out is NULL");
    if (batch->n_inst <= 0) return batch->n_inst == 0 ? FOT_OK : fail(h, FOT_ERR_INVALID, "n_inst < 0");
    { int r = check_scenarios(h, *batch, scenario); if (r != FOT_OK) return r; }
    // extents of the caller's obstacle arrays
    BatchLayout probe;
    std::string err;
    int rc = build_batch_layout(h->refs.data(), (int)h->refs.size(), scenario, *batch, probe, err);
    if (rc != FOT_OK) return fail(h, rc, err);
    const size_t elem = batch->obstacle_dtype == FOT_F32 ? sizeof(float) : sizeof(double);
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t st_bytes = (size_t)probe.n_static * 2 * elem, dy_bytes = (size_t)probe.dyn_src_points * 2 * elem;
    const size_t out_bytes = sizeof(fot_result) * (size_t)batch->n_inst;
    // A plan step for one or a few egos is latency, not bandwidth: its obstacle points and its records (written once,
    // by the selecting wave) then travel straight between the kernels and pinned host memory -- two copy operations and
    // their synchronisation less per call.  The dynamic tensors cross the bus ONCE: the NaN-scan blocks of the first
    // launch read them out of the pinned block and leave a copy in HBM for k_cull (NanScan::stage); the few static points
    // are read in place.  Up to the 2 MiB below that beats a staging copy plus its wait (scripts/size_sweep.py), beyond
    // it the tensors are staged in HBM with copy operations.
    if (st_bytes + dy_bytes <= 2 * SMALL_CALL_BYTES && out_bytes <= 8 * SMALL_CALL_BYTES) {   // (records stream out as instances finish)
        const size_t dy_off = align256(st_bytes);
        HIP_TRY(h, h->hSmallIn.ensure(dy_off + dy_bytes + 256));
        HIP_TRY(h, h->hRecOut.ensure(out_bytes));
        char *in = (char *)h->hSmallIn.p;
        if (st_bytes) std::memcpy(in, batch->static_xy, st_bytes);
        if (dy_bytes) std::memcpy(in + dy_off, batch->dyn_xy, dy_bytes);
        // the dynamic tensors cross PCIe once: the scan blocks of the first launch leave a copy in HBM for the others
        static const bool no_stage = std::getenv("FOT_NO_SCAN_STAGE") != nullptr;        // diagnostics scripts
        void *stage = nullptr;
        if (dy_bytes && !no_stage) { HIP_TRY(h, h->dUserDyn.ensure(dy_bytes + 256)); stage = h->dUserDyn.p; }
        arm_records(h, batch->n_inst);
        rc = enqueue_plan(h, *batch, scenario, in, in + dy_off, (fot_result *)h->hRecOut.p, h->stream, true, stage);
        if (rc != FOT_OK) { h->done_seq_armed = false; return rc; }
        rc = wait_records(h, batch->n_inst, h->stream);
        if (rc != FOT_OK) return rc;
        // what the device wrote of each record: the header and the first n_total entries of the 15 path arrays (a fifth of
        // the record at 51 samples -- the whole-record copy cost a one-ego call 2 us); the caller's entries past n_total stay
        // as they are
        const size_t head = offsetof(fot_result, t), used = sizeof(double) * (size_t)h->sc[0].P.n_total;
        for (int i = 0; i < batch->n_inst; ++i) {
            const fot_result *src = (const fot_result *)h->hRecOut.p + i;
            std::memcpy(&out[i], src, head);
            for (int f = 0; f < 15; ++f) std::memcpy(out[i].t + (size_t)f * FOT_MAX_NT, src->t + (size_t)f * FOT_MAX_NT, used);
        }
        return FOT_OK;
    }
    HIP_TRY(h, h->dUserStatic.ensure(std::max<size_t>(st_bytes, 16)));
    HIP_TRY(h, h->dUserDyn.ensure(std::max<size_t>(dy_bytes, 16)));
    HIP_TRY(h, h->dOut.ensure_zeroed(sizeof(fot_result) * (size_t)batch->n_inst));
    if (st_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserStatic.p, batch->static_xy, st_bytes, hipMemcpyHostToDevice, h->stream));
    if (dy_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserDyn.p, batch->dyn_xy, dy_bytes, hipMemcpyHostToDevice, h->stream));
    rc = enqueue_plan(h, *batch, scenario, h->dUserStatic.p, h->dUserDyn.p, h->dOut.as<fot_result>(), h->stream);
    if (rc != FOT_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, h->dOut.p, sizeof(fot_result) * (size_t)batch->n_inst, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FOT_OK;
}

int fot_frenet_state_batch(fot_handle *h, int32_t n, const fot_ego *ego,
                           double *frenet, double *ref, double *new_prev_s, int32_t *ok)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    if (n <= 0) return FOT_OK;
    if (!ego) return fail(h, FOT_ERR_INVALID, "ego is NULL");
    std::vector<InstDesc> desc((size_t)n);
    for (int i = 0; i < n; ++i) { desc[i] = InstDesc(); desc[i].ego = ego[i]; }
    for (int i = n - 1, run = 0; i >= 0; --i) {                 // chain lengths, as build_batch_layout sets them
        desc[i].n_chained = run;
        run = desc[i].ego.has_prev_s == FOT_PREV_S_CHAINED ? run + 1 : 0;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    { int r = order_begin(h, h->stream); if (r != FOT_OK) return r; }
    if (sizeof(InstDesc) * (size_t)n <= SMALL_CALL_BYTES) {      // small call: straight from / into pinned host memory
        HIP_TRY(h, h->hSmallIn.ensure(sizeof(InstDesc) * (size_t)n));
        HIP_TRY(h, h->hSmallOut.ensure(sizeof(InstState) * (size_t)n));
        std::memcpy(h->hSmallIn.p, desc.data(), sizeof(InstDesc) * (size_t)n);
        LAUNCH_TRY(h, launch_frenet_state(h->dP.as<DevParams>(), PathSet::single(spline_view(h, 0)), (const InstDesc *)h->hSmallIn.p,
                                          (InstState *)h->hSmallOut.p, n, MetaImport(), NanScan(), nullptr, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const InstState *stp = (const InstState *)h->hSmallOut.p;
        for (int i = 0; i < n; ++i) {
            if (frenet) std::memcpy(frenet + 6 * (size_t)i, stp[i].frenet0, sizeof(double) * 6);
            if (ref) std::memcpy(ref + 6 * (size_t)i, stp[i].ref0, sizeof(double) * 6);
            if (new_prev_s) new_prev_s[i] = stp[i].new_prev_s;
            if (ok) ok[i] = stp[i].c2f_ok;
        }
        return FOT_OK;
    }
    HIP_TRY(h, h->dTmpA.ensure(sizeof(InstDesc) * (size_t)n));
    HIP_TRY(h, h->dTmpB.ensure(sizeof(InstState) * (size_t)n));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpA.p, desc.data(), sizeof(InstDesc) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    LAUNCH_TRY(h, launch_frenet_state(h->dP.as<DevParams>(), PathSet::single(spline_view(h, 0)), h->dTmpA.as<InstDesc>(),
                                      h->dTmpB.as<InstState>(), n, MetaImport(), NanScan(), nullptr, h->stream));
    std::vector<InstState> st((size_t)n);
    HIP_TRY(h, hipMemcpyAsync(st.data(), h->dTmpB.p, sizeof(InstState) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
        if (frenet) std::memcpy(frenet + 6 * (size_t)i, st[i].frenet0, sizeof(double) * 6);
        if (ref) std::memcpy(ref + 6 * (size_t)i, st[i].ref0, sizeof(double) * 6);
        if (new_prev_s) new_prev_s[i] = st[i].new_prev_s;
        if (ok) ok[i] = st[i].c2f_ok;
    }
    return FOT_OK;
}

int fot_debug_candidates(fot_handle *h, int32_t inst, int32_t cap, double *cost,
                         int32_t *status, int32_t *keep, int32_t *n_t)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->last_valid) return fail(h, FOT_ERR_INVALID, "no completed plan call on this handle");
    int local = 0;
    Workspace *w = lane_of(h, inst, &local);
    if (!w) return fail(h, FOT_ERR_INVALID, "instance index out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // diagnostic entry: whatever stream the plan ran on
    const InstDesc &D = w->last.desc[local];
    InstState S;
    HIP_TRY(h, hipMemcpy(&S, w->dState.as<InstState>() + local, sizeof(InstState), hipMemcpyDeviceToHost));
    const int n = S.n_cand;
    const int m = n < cap ? n : cap;
    if (m <= 0) return n;
    std::vector<uint8_t> st8((size_t)m);
    std::vector<uint16_t> kp16((size_t)m);
    if (cost) HIP_TRY(h, hipMemcpy(cost, w->dCost.as<double>() + D.cand_off, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(st8.data(), w->dStatus.as<uint8_t>() + D.cand_off, (size_t)m, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(kp16.data(), w->dKeep.as<uint16_t>() + D.cand_off, sizeof(uint16_t) * (size_t)m, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; ++i) {
        if (status) status[i] = st8[i];
        if (keep) keep[i] = kp16[i];
        if (n_t) {                                               // (on the instance's own scenario)
            const DevParams &P = h->sc[(size_t)D.scen].P;
            if (i < D.n_grid) n_t[i] = P.ti[i / (D.n_tv * P.n_di)].n_t;
            else n_t[i] = P.n_total;
        }
    }
    return n;
}

int fot_debug_candidate_path(fot_handle *h, int32_t inst, int32_t index, double *arrays, int32_t *n_t)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->last_valid) return fail(h, FOT_ERR_INVALID, "no completed plan call on this handle");
    int local = 0;
    Workspace *w = lane_of(h, inst, &local);
    if (!w) return fail(h, FOT_ERR_INVALID, "instance index out of range");
    if (!arrays) return fail(h, FOT_ERR_INVALID, "arrays is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, h->dTmpA.ensure(sizeof(double) * 15 * FOT_MAX_NT));
    HIP_TRY(h, h->dTmpD.ensure(sizeof(int32_t) * 2));
    HIP_TRY(h, hipMemsetAsync(h->dTmpA.p, 0, sizeof(double) * 15 * FOT_MAX_NT, h->stream));
    const int scen = w->last.desc[(size_t)local].scen;          // the instance's own scenario
    LAUNCH_TRY(h, launch_debug_path(h->dP.as<DevParams>() + scen, (const InstDesc *)w->dMeta.p, w->dState.as<InstState>(),
                                    spline_view(h, scen), local, index,
                                    h->dTmpA.as<double>(), h->dTmpD.as<int32_t>(), h->stream));
    int32_t meta[2] = { 0, 0 };
    HIP_TRY(h, hipMemcpyAsync(arrays, h->dTmpA.p, sizeof(double) * 15 * FOT_MAX_NT, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(meta, h->dTmpD.p, sizeof(meta), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!meta[1]) return fail(h, FOT_ERR_INVALID, "candidate index out of range");
    if (n_t) *n_t = meta[0];
    return FOT_OK;
}

int32_t fot_wire_n_total(const fot_handle *h) { return h ? h->sc[0].P.n_total : FOT_ERR_INVALID; }

int32_t fot_wire_record_bytes(int32_t n_total)
{
    if (n_total < 1 || n_total > FOT_MAX_NT) return FOT_ERR_INVALID;
    return (int32_t)align256(sizeof(fot_wire_header) + sizeof(float) * 15 * (size_t)n_total);
}

int fot_pack_records_device(fot_handle *h, int32_t n, const fot_result *records_dev, void *wire_dev, void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (n <= 0) return n == 0 ? FOT_OK : fail(h, FOT_ERR_INVALID, "n < 0");
    if (!records_dev || !wire_dev) return fail(h, FOT_ERR_INVALID, "NULL buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // ordered behind the handle's previous enqueue whatever stream that ran on: the records are usually the output of
    // the plan call just made, and NULL (= the handle's own stream) is also torch's default-stream handle
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    LAUNCH_TRY(h, launch_pack_wire(n, h->sc[0].P.n_total, fot_wire_record_bytes(h->sc[0].P.n_total), records_dev,
                                   (unsigned char *)wire_dev, st));
    return order_end(h, st);
}

static_assert(offsetof(fot_result, s) - offsetof(fot_result, t) == sizeof(double) * FOT_MAX_NT &&
              offsetof(fot_result, c) - offsetof(fot_result, t) == sizeof(double) * FOT_MAX_NT * 14,
              "the 15 path arrays of fot_result are contiguous");

int fot_pack_records_host(int32_t n_total, int32_t n, const fot_result *records, void *wire)
{
    const int32_t stride = fot_wire_record_bytes(n_total);
    if (stride < 0 || n < 0 || (n > 0 && (!records || !wire))) return FOT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const fot_result &R = records[i];
        unsigned char *w = (unsigned char *)wire + (size_t)i * stride;
        std::memset(w, 0, (size_t)stride);
        fot_wire_header H;
        std::memset(&H, 0, sizeof(H));
        H.status = R.status; H.best_index = R.best_index; H.n_cand = R.n_cand; H.n_keep = R.n_keep;
        H.cost = R.cost; H.stats_valid = R.stats_valid; H.n_total = n_total;
        H.new_last_kappa = R.new_last_kappa; H.new_prev_s = R.new_prev_s;
        std::memcpy(H.stats, R.stats, sizeof(H.stats));
        std::memcpy(H.frenet0, R.frenet0, sizeof(H.frenet0));
        std::memcpy(H.ref0, R.ref0, sizeof(H.ref0));
        std::memcpy(w, &H, sizeof(H));
        float *path = (float *)(w + sizeof(H));
        const double *arr = R.t;
        for (int f = 0; f < 15; ++f) {                           // (k_pack_wire: offsets for s, x, y; zeros past n_keep)
            const double base = f == 1 ? R.frenet0[0] : f == 9 ? R.ref0[1] : f == 10 ? R.ref0[2] : 0.0;
            for (int k = 0; k < n_total; ++k)
                path[f * n_total + k] = k < R.n_keep ? (float)(arr[f * FOT_MAX_NT + k] - base) : 0.0f;
        }
    }
    return FOT_OK;
}

int fot_unpack_records(int32_t n_total, int32_t n, const void *wire, fot_result *records)
{
    const int32_t stride = fot_wire_record_bytes(n_total);
    if (stride < 0 || n < 0 || (n > 0 && (!records || !wire))) return FOT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const unsigned char *w = (const unsigned char *)wire + (size_t)i * stride;
        fot_wire_header H;
        std::memcpy(&H, w, sizeof(H));
        if (H.n_total != n_total) return FOT_ERR_INVALID;
        if (H.n_keep < 0 || H.n_keep > n_total || H.n_cand < 0 || H.best_index < -1 || H.best_index >= (H.n_cand > 0 ? H.n_cand : 1))
            return FOT_ERR_INVALID;                              // (a corrupt or foreign record)
        fot_result &R = records[i];
        std::memset(&R, 0, sizeof(R));
        R.status = H.status; R.best_index = H.best_index; R.n_cand = H.n_cand; R.n_keep = H.n_keep;
        R.cost = H.cost; R.stats_valid = H.stats_valid;
        R.new_last_kappa = H.new_last_kappa; R.new_prev_s = H.new_prev_s;
        std::memcpy(R.stats, H.stats, sizeof(H.stats));
        std::memcpy(R.frenet0, H.frenet0, sizeof(H.frenet0));
        std::memcpy(R.ref0, H.ref0, sizeof(H.ref0));
        const float *path = (const float *)(w + sizeof(H));
        double *arr = R.t;
        const int keep = H.n_keep < n_total ? H.n_keep : n_total;
        for (int f = 0; f < 15; ++f) {
            const double base = f == 1 ? R.frenet0[0] : f == 9 ? R.ref0[1] : f == 10 ? R.ref0[2] : 0.0;
            for (int k = 0; k < keep; ++k) arr[f * FOT_MAX_NT + k] = base + (double)path[f * n_total + k];
        }
    }
    return FOT_OK;
}

int fot_debug_set_eval_segments(fot_handle *h, int32_t n_seg)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_seg < 0 || n_seg > 4) return fail(h, FOT_ERR_INVALID, "fot_debug_set_eval_segments: 0 (automatic) .. 4");
    h->eval_segments = n_seg;
    return FOT_OK;
}

int fot_debug_set_tile_cut(fot_handle *h, int32_t cut)
{
    if (!h) return FOT_ERR_INVALID;
    if (cut != TILE_CUT_AUTO && cut != TILE_CUT_WAVE && cut != TILE_CUT_GROUP)
        return fail(h, FOT_ERR_INVALID, "fot_debug_set_tile_cut: 0 (automatic), 1 (per-wave rows), 2 (groups)");
    if (cut == h->tile_cut) return FOT_OK;
    return upload_tile_shapes(h, cut);
}

int fot_debug_set_eval_form(fot_handle *h, int32_t form)
{
    if (!h) return FOT_ERR_INVALID;
    if (form < -1 || form > 1)
        return fail(h, FOT_ERR_INVALID, "fot_debug_set_eval_form: 0 (by eligibility), 1 (general form), -1 (query only)");
    if (form >= 0) h->eval_form = form;
    return h->last_eval_forms;
}

int fot_debug_time_info(const fot_handle *h, double time, int32_t *n_t, double *quartic_inv4, double *quintic_inv9)
{
    if (!h || !(time > 0.0)) return FOT_ERR_INVALID;
    TimeInfo ti;
    if (!time_info(time, h->sc[0].params.dt, ti)) return FOT_ERR_UNSUPPORTED;      // more than FOT_MAX_NT samples
    if (n_t) *n_t = ti.n_t;
    if (quartic_inv4) std::memcpy(quartic_inv4, ti.qa, sizeof(ti.qa));
    if (quintic_inv9) std::memcpy(quintic_inv9, ti.qi, sizeof(ti.qi));
    return FOT_OK;
}

int fot_debug_margins(fot_handle *h, int32_t inst, int32_t cap, double *margins)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->last_valid) return fail(h, FOT_ERR_INVALID, "no completed plan call on this handle");
    int local = 0;
    Workspace *w = lane_of(h, inst, &local);
    if (!w) return fail(h, FOT_ERR_INVALID, "instance index out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // diagnostic entry: whatever stream the plan ran on
    InstState S;
    HIP_TRY(h, hipMemcpy(&S, w->dState.as<InstState>() + local, sizeof(InstState), hipMemcpyDeviceToHost));
    const int n = S.n_cand;
    const int m = n < cap ? n : cap;
    if (m <= 0 || !margins) return n;
    const size_t bytes = sizeof(double) * FOT_MARGIN_GROUPS * (size_t)m;
    HIP_TRY(h, h->dTmpB.ensure(bytes));
    EntryArrays ea;
    ea.cnt = w->dEntCnt.as<int32_t>(); ea.e32 = w->dEnt32.as<f2>(); ea.e64 = w->dEnt64.as<d2>();
    ea.sid = w->dEntSid.as<uint8_t>(); ea.rng = w->dWaveRng.as<TileStep>();
    const int scen = w->last.desc[(size_t)local].scen;          // the instance's own scenario
    LAUNCH_TRY(h, launch_debug_margins(h->dP.as<DevParams>() + scen, (const InstDesc *)w->dMeta.p, w->dState.as<InstState>(),
                                       spline_view(h, scen), local, ea, m, h->dTmpB.as<double>(), h->stream));
    HIP_TRY(h, hipMemcpyAsync(margins, h->dTmpB.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return n;
}

}  // extern "C"

namespace {

// shared body of fot_check_collision_paths (mode 0) and fot_check_paths (mode 1)
int check_ext(fot_handle *h, int mode, int32_t n_paths, const int32_t *len, const int32_t *rule_len,
              const double *const arr[9], const fot_overrides *ov, double max_stop,
              int32_t n_static, const double *static_xy, int32_t dmode, int32_t S, int32_t Pn, int32_t T,
              const double *dyn, int32_t *status_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_paths <= 0) return FOT_OK;
    if (!len || !status_out) return fail(h, FOT_ERR_INVALID, "NULL path array");
    const DevParams &P = h->sc[0].P;
    // one single-instance batch carries limits + obstacle set
    fot_ego ego = {};
    double target = 0.0;
    int32_t soff[2] = { 0, n_static > 0 ? n_static : 0 };
    int64_t doff[1] = { 0 };
    int32_t dims[4] = { dmode, S, Pn, T };
    fot_batch b = {};
    b.n_inst = 1; b.obstacle_dtype = FOT_F64; b.ego = &ego; b.target_speed = &target;
    b.overrides = ov; b.max_stop_distance = &max_stop;
    b.static_xy = static_xy; b.static_off = soff; b.dyn_xy = dyn; b.dyn_off = doff; b.dyn_dims = dims;
    BatchLayout L;
    std::string err;
    int rc = build_batch_layout(h->sc[0].params, P, h->sc[0].shapes, b, L, err);
    if (rc != FOT_OK) return fail(h, rc, err);
    h->last_valid = false;

    const size_t np = (size_t)n_paths, plane = np * FOT_MAX_NT;
    std::vector<double> flat(9 * plane, 0.0);
    for (int i = 0; i < n_paths; ++i)
        if (len[i] < 0 || len[i] > FOT_MAX_NT) return fail(h, FOT_ERR_INVALID, "path length out of range");
    for (int f = 0; f < 9; ++f)
        if (arr[f]) std::memcpy(flat.data() + f * plane, arr[f], sizeof(double) * plane);
    // meta: len[np], then rule_len[np][FOT_CHECK_RULE_LENS] (NULL: every array holds len[i] samples)
    std::vector<int32_t> meta((1 + FOT_CHECK_RULE_LENS) * np);
    std::memcpy(meta.data(), len, sizeof(int32_t) * np);
    for (size_t j = 0; j < FOT_CHECK_RULE_LENS * np; ++j) {
        const int32_t v = rule_len ? rule_len[j] : len[j / FOT_CHECK_RULE_LENS];
        if (v < 0 || v > FOT_MAX_NT) return fail(h, FOT_ERR_INVALID, "rule length out of range");
        meta[np + j] = v;
    }

    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const size_t st_bytes = sizeof(double) * 2 * (size_t)L.n_static, dy_bytes = sizeof(double) * 2 * (size_t)L.dyn_src_points;
    HIP_TRY(h, h->dUserStatic.ensure(std::max<size_t>(st_bytes, 16)));
    HIP_TRY(h, h->dUserDyn.ensure(std::max<size_t>(dy_bytes, 16)));
    HIP_TRY(h, h->dTmpA.ensure(sizeof(InstDesc)));
    HIP_TRY(h, h->dTmpB.ensure(sizeof(double) * flat.size()));
    HIP_TRY(h, h->dTmpC.ensure(sizeof(int32_t) * meta.size()));
    HIP_TRY(h, h->dTmpD.ensure(sizeof(int32_t) * np));
    if (st_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserStatic.p, static_xy, st_bytes, hipMemcpyHostToDevice, st));
    // a pedestrian whose track holds a NaN coordinate anywhere is no obstacle at any step (the reference's pre-filter
    // takes np.min / np.max over the whole track, frenet_planner.py:1211-1219): k_check_ext tests step by step, where an
    // all-NaN track says the same
    std::vector<double> dyn_clean;
    if (dy_bytes && L.desc[0].dyn_mode != FOT_DYN_NONE) {
        const InstDesc &D0 = L.desc[0];
        const size_t row = 2 * (size_t)D0.T;
        for (size_t j = 0; j < (size_t)D0.S * D0.P; ++j) {
            bool bad = false;
            for (size_t e = 0; e < row; ++e) bad |= std::isnan(dyn[j * row + e]);
            if (!bad) continue;
            if (dyn_clean.empty()) dyn_clean.assign(dyn, dyn + 2 * (size_t)L.dyn_src_points);
            for (size_t e = 0; e < row; ++e) dyn_clean[j * row + e] = NAN;
        }
    }
    if (dy_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserDyn.p, dyn_clean.empty() ? dyn : dyn_clean.data(), dy_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpA.p, L.desc.data(), sizeof(InstDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpB.p, flat.data(), sizeof(double) * flat.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpC.p, meta.data(), sizeof(int32_t) * meta.size(), hipMemcpyHostToDevice, st));
    LAUNCH_TRY(h, launch_check_ext(h->dP.as<DevParams>(), h->dTmpA.as<InstDesc>(), n_paths, mode, h->dTmpC.as<int32_t>(),
                                   h->dTmpC.as<int32_t>() + np, h->dTmpB.as<double>(), h->dUserStatic.as<double>(),
                                   h->dUserDyn.as<double>(), h->dTmpD.as<int32_t>(), st));
    HIP_TRY(h, hipMemcpyAsync(status_out, h->dTmpD.p, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

}  // namespace

extern "C" {

int fot_check_collision_paths(fot_handle *h, int32_t n_paths, const int32_t *len,
                              const double *x, const double *y, const double *yaw, const double *t,
                              int32_t n_static, const double *static_xy,
                              int32_t mode, int32_t S, int32_t Pn, int32_t T, const double *dyn,
                              int32_t *free_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_paths > 0 && (!x || !y || !t)) return fail(h, FOT_ERR_INVALID, "NULL path array");
    if (n_paths > 0 && h->sc[0].P.has_footprint && !yaw)
        return fail(h, FOT_ERR_INVALID, "yaw is required with a multi-circle footprint");
    const double *arr[9] = { x, y, yaw, nullptr, nullptr, nullptr, nullptr, nullptr, t };
    return check_ext(h, 0, n_paths, len, nullptr, arr, nullptr, NAN, n_static, static_xy, mode, S, Pn, T, dyn, free_out);
}

int fot_check_paths(fot_handle *h, int32_t n_paths, const int32_t *len, const int32_t *rule_len,
                    const double *x, const double *y, const double *yaw, const double *v, const double *a,
                    const double *c, const double *d, const double *s, const double *t,
                    const fot_overrides *overrides, double max_stop_distance,
                    int32_t n_static, const double *static_xy,
                    int32_t mode, int32_t S, int32_t Pn, int32_t T, const double *dyn, int32_t *status_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_paths > 0 && (!x || !y || !v || !a || !c || !t)) return fail(h, FOT_ERR_INVALID, "NULL path array");
    const double *arr[9] = { x, y, yaw, v, a, c, d, s, t };
    return check_ext(h, 1, n_paths, len, rule_len, arr, overrides, max_stop_distance, n_static, static_xy, mode, S, Pn, T,
                     dyn, status_out);
}

}  // extern "C"
