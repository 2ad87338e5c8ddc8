// fot_loop_kernels.hip -- gfx950 kernels of the prediction entry points and of the closed loop: everything below the C ABI
// that is not the plan pipeline (fot_kernels.hip) or the Social-GAN generator (fot_sgan.hip).
//
//   k_resample / k_sample_dist   fot_resample_predictions, fot_predict_cv: predictor output -> dense obstacle tensor
//   k_pred_scores                fot_prediction_scores: best-of-N ADE / FDE and KDE-NLL of a prediction origin
//   k_safety                     fot_safety_metrics_batch and the loop's per-step metrics
//   k_footprint_steps / _yaw / _fold
//                                fot_footprint_recheck: centre, circle cover and exact rectangle per step, the heading
//                                reconstruction, the fold of a trajectory
//   k_fidelity_peds / _series / _fold
//                                fot_fidelity_eval: avoidance onset and roll-out error per pedestrian, the separation per
//                                step, the record of an encounter
//   k_enc_columns / _compact / _gather / _rows
//                                fot_encounters_extract: presence and closest approach per column of a span, the kept
//                                columns and the span's minimum, the packed encounters and speeds, cruise speed and goal
//   k_loop_* / k_static_gather / k_predict_cv_frame
//                                the resident loop (fot_loop_run): frame, sample gather, prediction, digests, history,
//                                prediction-error summaries, predictor scores, representative sample
// No inline assembly here, so no ISA-guard pass: the evaluation kernels' object file does not depend on this unit.
#include <hip/hip_runtime.h>

#include "fot_math.hpp"
#include "fot_loop_kernels.h"

namespace fot {

// ---------------------------------------------------------------------------
// prediction resampling -> obstacle tensor
// ---------------------------------------------------------------------------

struct ResampleArgs {
    double sgan_dt, sim_dt, staleness;
    int S, pred_len, P, n_dense, T;          // T = n_dense + prepend
    int has_anchor, prepend, cv;             // cv: sources are (obs_prev, obs_last) -> constant velocity; 2: float32 obs
    int tmajor;                              // out[k][s][p][axis] (FOT_OUT_TMAJOR) instead of out[s][p][k][axis]
    // per-episode blocks (the closed loop's distribution frame): pedestrian p belongs to episode ped_ep[p], whose
    // pedestrians are [ep_ped0[e], ep_ped0[e + 1]) and whose [S][P_e][T][2] block starts at point ep_blk[e]; nullptr: one
    // [S][P][T][2] tensor
    const int32_t *ped_ep; const int32_t *ep_ped0; const int64_t *ep_blk;
};

// one thread per (sample, pedestrian, axis); out[s][p][k][axis]
template <typename TI, typename TO>
__global__ void k_resample(ResampleArgs A, const TI *__restrict__ pred, const double *__restrict__ anchor,
                           const double *__restrict__ current, TO *__restrict__ out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.S * A.P * 2) return;
    const int ax = idx & 1, sp = idx >> 1, p = sp % A.P, smp = sp / A.P;
    // element (row k) of this thread's (sample, pedestrian, axis): rows are T apart in the reference's layout and a whole
    // S x P plane apart in the T-major one (where neighbouring threads then write neighbouring addresses)
    const int64_t k_stride = A.tmajor ? (int64_t)A.S * A.P * 2 : 2;
    TO *dst = out + (A.tmajor ? (int64_t)sp * 2 : (int64_t)sp * A.T * 2) + ax;
    if (A.ped_ep) {
        const int e = A.ped_ep[p], p0 = A.ep_ped0[e], P_e = A.ep_ped0[e + 1] - p0;
        dst = out + 2 * (A.ep_blk[e] + ((int64_t)smp * P_e + (p - p0)) * A.T) + ax;
    }
    if (A.prepend) dst[0] = (TO)current[2 * p + ax];
    dst += k_stride * A.prepend;
    if (A.cv) {                                                     // predict_cv (:188-231)
        const double cur = anchor[2 * p + ax];                      // obs_last
        double vel = 0.0;
        if (pred && A.cv == 2)                                      // float32 observations: float32 velocity (:216)
            vel = (double)(((float)cur - (float)pred[2 * p + ax]) / (float)A.sgan_dt);
        else if (pred)
            vel = (cur - (double)pred[2 * p + ax]) / A.sgan_dt;     // obs_prev
        for (int i = 0; i < A.n_dense; ++i) {
            const double t = (A.sim_dt + (double)i * A.sim_dt) + A.staleness;
            dst[k_stride * i] = (TO)(cur + vel * t);
        }
        return;
    }
    ResampleAxis R;
    R.sgan_dt = A.sgan_dt; R.staleness = A.staleness;
    R.first_k = A.has_anchor ? 0 : 1;
    int n = 0;
    if (A.has_anchor) R.co[n++] = anchor[2 * p + ax];
    for (int k = 0; k < A.pred_len; ++k) R.co[n++] = (double)pred[(((int64_t)smp * A.pred_len + k) * A.P + p) * 2 + ax];
    R.n_src = n;
    const bool constant = R.all_close(R.co[0]) || R.all_close(0.0);
    const double v_tail = R.tail_velocity();
    for (int i = 0; i < A.n_dense; ++i)
        dst[k_stride * i] = (TO)R.at(A.sim_dt + (double)i * A.sim_dt, constant, v_tail);
}

// The ragged form of a sweep loop with a sample count per slot (fot_loop_set_slot_samples): running episode e keeps the
// first ep_S[e] samples of the raw tensor [S_src][pred_len][rows][2] in its [ep_S[e]][P_e][n_dense + 1][2] block.  The grid
// is (episode, sample, chunk of the episode's (pedestrian, axis) pairs): a workgroup whose sample lies beyond its
// episode's count, or whose chunk lies beyond its pedestrians, leaves on a uniform test before it loads a coordinate, so
// the work and the stores follow sum S_e * P_e.  The arithmetic of a point is k_resample's anchored, prepending path
// (has_anchor = prepend = 1, cv = 0, float64 out), operation for operation: a point has the bits it has in any company.
struct ResampleSlotsArgs {
    double sgan_dt, sim_dt, staleness;
    int pred_len, rows, n_dense;             // rows: the frame's pedestrians (the raw tensor's innermost extent)
    const int32_t *ep_ped0; const int64_t *ep_blk; const int32_t *ep_S;
};
constexpr int RSS_THREADS = WAVE;

// ResampleAxis (fot_math.hpp) with the source coordinates of a lane in its own column of LDS instead of a private array
// (which the run-time index of `at` sends to scratch memory): every method is ResampleAxis's, expression for expression,
// with co[i] spelled co(i) -- the same operations in the same order, so the same bits.
struct ResampleAxisLds {
    const double *col;                       // element i of this lane: col[i * RSS_THREADS]
    int n_src, first_k;
    double sgan_dt, staleness;
    __device__ __forceinline__ double co(int i) const { return col[i * RSS_THREADS]; }
    __device__ __forceinline__ double ts(int i) const { return (double)(i + first_k) * sgan_dt - staleness; }
    __device__ __forceinline__ bool all_close(double b) const
    {
        bool ok = true;
        for (int i = 0; i < n_src; ++i) ok = ok && (fabs(co(i) - b) <= 1e-8 + 1e-5 * fabs(b));
        return ok;
    }
    __device__ __forceinline__ double at(double t, bool constant, double v_tail) const
    {
        if (constant) return co(n_src - 1);
        const double t_last = ts(n_src - 1);
        if (n_src >= 2 && t > t_last) return co(n_src - 1) + v_tail * (t - t_last);
        if (t > t_last) return co(n_src - 1);
        if (t < ts(0)) return co(0);
        int j = 0;
        for (int i = 1; i < n_src; ++i) j = ts(i) <= t ? i : j;     // last source time <= t
        if (j == n_src - 1 || ts(j) == t) return co(j);
        const double slope = (co(j + 1) - co(j)) / (ts(j + 1) - ts(j));
        return slope * (t - ts(j)) + co(j);
    }
    __device__ __forceinline__ double tail_velocity() const
    {
        if (n_src < 2) return 0.0;
        const int lookback = n_src < 3 ? n_src : 3;
        const double v = (co(n_src - 1) - co(n_src - lookback)) / ((double)(lookback - 1) * sgan_dt);
        return fmax(fmin(v, 2.5), -2.5);                              // MAX_WALKING_SPEED
    }
};

template <typename TI>
__global__ void __launch_bounds__(RSS_THREADS)
k_resample_slots(ResampleSlotsArgs A, const TI *__restrict__ pred, const double *__restrict__ anchor,
                 const double *__restrict__ current, double *__restrict__ out)
{
    __shared__ double s_co[FOT_MAX_PRED_LEN + 1][RSS_THREADS];       // 18.5 KB: source i of lane t at [i][t], no bank conflicts
    const int e = blockIdx.x, smp = blockIdx.y;
    if (smp >= A.ep_S[e]) return;                                    // (uniform)
    const int p0 = A.ep_ped0[e], P_e = A.ep_ped0[e + 1] - p0;
    if ((int)(blockIdx.z * RSS_THREADS) >= 2 * P_e) return;          // (uniform)
    const int idx = blockIdx.z * RSS_THREADS + threadIdx.x;
    if (idx >= 2 * P_e) return;
    const int ax = idx & 1, q = idx >> 1, p = p0 + q, T = A.n_dense + 1;
    double *dst = out + 2 * (A.ep_blk[e] + ((int64_t)smp * P_e + q) * T) + ax;
    dst[0] = current[2 * p + ax];
    dst += 2;
    double *col = &s_co[0][threadIdx.x];                             // (a lane reads only what it wrote: no barrier)
    ResampleAxisLds R;
    R.col = col;
    R.sgan_dt = A.sgan_dt; R.staleness = A.staleness;
    R.first_k = 0;
    int n = 0;
    col[RSS_THREADS * n++] = anchor[2 * p + ax];
    for (int k = 0; k < A.pred_len; ++k)
        col[RSS_THREADS * n++] = (double)pred[(((int64_t)smp * A.pred_len + k) * A.rows + p) * 2 + ax];
    R.n_src = n;
    const bool constant = R.all_close(R.co(0)) || R.all_close(0.0);
    const double v_tail = R.tail_velocity();
    for (int i = 0; i < A.n_dense; ++i)
        dst[2 * i] = R.at(A.sim_dt + (double)i * A.sim_dt, constant, v_tail);
}

// block = sample: sum over (p, k) of the distance to the sample mean (predict_single_best :346-350)
template <typename TO>
__global__ void __launch_bounds__(256)
k_sample_dist(int S, int P, int T, int skip, int tmajor, const TO *__restrict__ out, double *__restrict__ dist)
{
    auto at = [&](int q, int p, int k) {
        return out + (tmajor ? ((int64_t)k * S + q) * P + p : ((int64_t)q * P + p) * T + k) * 2;
    };
    const int smp = blockIdx.x;
    const int n = P * (T - skip);
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int p = i / (T - skip), k = i - p * (T - skip) + skip;  // the prepended current position is not part of it
        double mx = 0.0, my = 0.0;
        for (int q = 0; q < S; ++q) {
            const TO *e = at(q, p, k);
            mx += (double)e[0]; my += (double)e[1];
        }
        mx /= (double)S; my /= (double)S;
        const TO *e = at(smp, p, k);
        const double dx = (double)e[0] - mx, dy = (double)e[1] - my;
        acc += sqrt(dx * dx + dy * dy);
    }
    __shared__ double part[256 / WAVE];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int)(blockDim.x / WAVE); ++w) t += part[w];
        dist[smp] = t;
    }
}

// ---------------------------------------------------------------------------
// fot_prediction_scores (fot_predscore.hpp): one workgroup per prediction origin
// ---------------------------------------------------------------------------
// Pedestrians are taken in tiles of PS_TILE_PAIRS / E whose truth points lie in LDS.  Per tile, lanes first run over the
// pedestrians (sequential over s and j: the row sums d[s][p][.] feed the per-agent minima in registers and, through a
// butterfly over the wave, the per-sample scene sums in LDS, one slot per (s, wave)), then over the (p, j) pairs (the
// bandwidths and log p of a pair stay in the lane that owns it).  Lanes past the tile add 0.0.  The partial sums of the
// lanes meet in a butterfly and the waves' in index order: the order of every sum follows from (S, P, E) alone.
constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / WAVE;
constexpr int PS_TILE_PAIRS = 1024;              // truth points of a tile in LDS (16 KB); >= FOT_MAX_PRED_LEN
static_assert(PS_TILE_PAIRS >= FOT_MAX_PRED_LEN, "a tile holds one pedestrian's evaluation points at least");

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

template <typename TO>
__global__ void __launch_bounds__(PS_THREADS)
k_pred_scores(const PredOriginDev *__restrict__ desc, const TO *__restrict__ tensor, int stride, int E,
              const double *__restrict__ truth, fot_pred_score *__restrict__ out)
{
#define PS_ROWS FOT_MAX_SAMPLES
#include "fot_pred_scores_body.inc"
#undef PS_ROWS
}

// The wide form: a launch with an origin of more than FOT_MAX_SAMPLES samples (a handle with a raised sample capacity).
// The same body (fot_pred_scores_body.inc) over tables of FOT_MAX_PLAN_SAMPLES rows (2 x 254 x 4 doubles, 16 KB beside the
// tile's 16 KB): an origin's sums are taken in the same order in either form, so a narrow origin of a wide launch has the
// record it has alone.
template <typename TO>
__global__ void __launch_bounds__(PS_THREADS)
k_pred_scores_wide(const PredOriginDev *__restrict__ desc, const TO *__restrict__ tensor, int stride, int E,
                   const double *__restrict__ truth, fot_pred_score *__restrict__ out)
{
#define PS_ROWS FOT_MAX_PLAN_SAMPLES
#include "fot_pred_scores_body.inc"
#undef PS_ROWS
}

// ---------------------------------------------------------------------------
// safety metrics, one wave per ego, lanes over (footprint circle, pedestrian) pairs
// ---------------------------------------------------------------------------

__device__ __forceinline__ double wave_min_f64(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, WAVE));
    return v;
}

__global__ void __launch_bounds__(WAVE)
k_safety(const DevParams *__restrict__ Pp, int n, const double *__restrict__ ego, const int32_t *__restrict__ ped_off,
         const double *__restrict__ ped_pos, const double *__restrict__ ped_vel, double ego_radius, double ped_radius,
         double footprint_radius, int use_fp, fot_safety *__restrict__ out, const int32_t *__restrict__ ep_scen,
         const SafetyScen *__restrict__ scen_tab)
{
    const int e = blockIdx.x;
    if (e >= n) return;
    // a scenario loop: the episode's scenario picks the constants, the footprint radius and the flag.  One episode = one
    // workgroup of one wave, so the id and everything read through it are wave-uniform (scalar loads).
    if (ep_scen) {
        const int scen = ep_scen[e];
        Pp += scen;
        footprint_radius = scen_tab[scen].footprint_radius;
        use_fp = scen_tab[scen].use_fp;
    }
    const DevParams &P = *Pp;
    const double x = ego[4 * e], y = ego[4 * e + 1], yaw = ego[4 * e + 2], v = ego[4 * e + 3];
    const double hx = cos(yaw), hy = sin(yaw);
    const bool fp = use_fp && P.has_footprint;
    const int nc = fp ? P.n_circ : 1;
    const double combined = (fp ? footprint_radius : ego_radius) + ped_radius;
    const int p0 = ped_off[e], np_ = ped_off[e + 1] - p0;
    double min_d = INFINITY, ttc = INFINITY, ahead = INFINITY;
    for (int i = threadIdx.x; i < nc * np_; i += WAVE) {
        const int c = i / np_, p = i - c * np_;
        const double off = fp ? P.circ_off[c] : 0.0;
        const double cx = x + off * hx, cy = y + off * hy;                      // footprint.py:42-45
        const double px = ped_pos[2 * (p0 + p)], py = ped_pos[2 * (p0 + p) + 1];
        const double rx = px - cx, ry = py - cy;
        const double dist = sqrt(rx * rx + ry * ry);
        min_d = fmin(min_d, dist);
        const double vx = ped_vel[2 * (p0 + p)] - v * hx, vy = ped_vel[2 * (p0 + p) + 1] - v * hy;
        const double along = -(rx * vx + ry * vy) / (dist + 1e-8);
        if (along > 1e-5) {
            const double t = (dist - combined) / along;
            if (t >= 0.0) ttc = fmin(ttc, t);
        }
        if ((px - x) * hx + (py - y) * hy > 0.0) ahead = fmin(ahead, dist);      // strictly ahead of the vehicle centre
    }
    min_d = wave_min_f64(min_d); ttc = wave_min_f64(ttc); ahead = wave_min_f64(ahead);
    if (threadIdx.x == 0) {
        fot_safety r;
        r.min_distance = min_d; r.ttc = ttc; r.clearance = min_d - combined;
        r.clearance_ahead = isinf(ahead) ? INFINITY : ahead - combined;
        r.collision = min_d < combined ? 1 : 0; r._pad = 0;
        out[e] = r;
    }
}

// ---------------------------------------------------------------------------
// fot_loop_run: the step's frame from the resident recording, the records' digests, the history of followed paths
// ---------------------------------------------------------------------------

// One workgroup per running episode.  Its rows of the recording -- current positions and velocities at frame f_cur, the
// observer's last two samples at f_last / f_prev, each clamped to the slot's own recording -- go into the compacted
// frame as 16-byte rows; thread 0 moves the episode's entries of the host's tables into HBM.
__global__ void __launch_bounds__(WAVE)
k_loop_frame(ReplayView rv, FrameStage in, FrameDev out, int n_run, int f_cur, int f_last, int f_prev)
{
    const int i = blockIdx.x;
    if (i >= n_run) return;
    const int slot = in.slot[i], q0 = in.ped0[i], q1 = in.ped0[i + 1];
    const int c0 = rv.slot_ped0[slot], last_row = rv.slot_frames[slot] - 1;
    const int64_t cols = rv.n_cols;
    const double2 *pos = (const double2 *)rv.pos, *vel = (const double2 *)rv.vel;
    const int64_t r_cur = (int64_t)min(f_cur, last_row) * cols + c0;
    const int64_t r_last = (int64_t)min(max(f_last, 0), last_row) * cols + c0;
    const int64_t r_prev = (int64_t)min(max(f_prev, 0), last_row) * cols + c0;
    for (int p = threadIdx.x; p < q1 - q0; p += WAVE) {
        const int q = q0 + p;
        ((double2 *)out.pos)[q] = pos[r_cur + p];
        ((double2 *)out.vel)[q] = vel[r_cur + p];
        out.ped_ep[q] = i;
        if (f_last >= 0) {
            const double2 l = pos[r_last + p];
            double2 w; w.x = (double)(float)l.x; w.y = (double)(float)l.y;     // the observer hands over float32 (observer.py:134)
            ((double2 *)out.last)[q] = w;
            double2 u = w;                                               // (no second sample: zero velocity)
            if (f_prev >= 0) { const double2 v = pos[r_prev + p]; u.x = (double)(float)v.x; u.y = (double)(float)v.y; }
            ((double2 *)out.prev)[q] = u;
        }
    }
    if (threadIdx.x == 0) {
        out.ped0[i] = q0; out.blk[i] = in.blk[i]; out.prepend[i] = in.prepend[i];
        if (i == n_run - 1) { out.ped0[n_run] = q1; out.blk[n_run] = in.blk[n_run]; }
    }
    if (threadIdx.x < 4) out.ego[4 * i + threadIdx.x] = in.ego[4 * i + threadIdx.x];
    if (in.scen && threadIdx.x == 0) out.scen[i] = in.scen[i];
}

namespace {

constexpr int SR_THREADS = 256;

// One thread per (sample s, predictor step j, frame row q) element of two coordinates, rows innermost: a wave reads and
// writes runs of neighbouring pedestrians, 8 bytes (float32) or 16 bytes (float64) a lane.  The place in the recording
// is fot_samplerec.hpp's, 64-bit throughout; nothing but the element's own lane index decides what a lane moves.
template <class V>
__global__ __launch_bounds__(SR_THREADS) void k_loop_sample_rows(LoopSampleRows a)
{
    const int64_t t = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x;
    if (t >= sr_step_elems(a.d)) return;
    int32_t s, j, q;
    sr_split(a.d, t, s, j, q);
    ((V *)a.out)[t] = ((const V *)a.rec)[sr_src_elem(a.d, s, j, a.col[q])];    // (t = sr_dst_elem(a.d, s, j, q))
}

// The same lane layout over the raw tensors of several models: row q's 16-byte table entry names its model's tensor, that
// tensor's width and the row's column (fot_sweep.hpp).  The lanes of a wave load neighbouring entries and, within one
// episode, read and write runs of neighbouring pedestrians.
__global__ __launch_bounds__(SR_THREADS) void k_loop_model_rows(LoopModelRows a)
{
    SampleRecDims d;
    d.S = a.S; d.pred_len = a.pred_len; d.rows = a.rows;
    const int64_t t = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x;
    if (t >= sr_step_elems(d)) return;
    int32_t s, j, q;
    sr_split(d, t, s, j, q);
    a.out[t] = a.pool[sweep_model_src_elem(a.tab[q], a.pred_len, s, j)];       // (t = sr_dst_elem(d, s, j, q))
}

// k_loop_sample_rows for a loop with a sample count per slot: the step's raw tensor holds the first a.d.S samples only
// (the largest count among the loop's slots), read out of a source of S_src >= a.d.S samples a row.
template <class V>
__global__ __launch_bounds__(SR_THREADS) void k_loop_sample_rows_prefix(LoopSampleRows a, int32_t S_src)
{
    const int64_t t = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x;
    if (t >= sr_step_elems(a.d)) return;
    int32_t s, j, q;
    sr_split(a.d, t, s, j, q);
    SampleRecDims src = a.d;
    src.S = S_src;
    ((V *)a.out)[t] = ((const V *)a.rec)[sr_src_elem(src, s, j, a.col[q])];
}

}  // namespace

// One workgroup per request of a scenario loop: its scenario's static points, resident once in HBM, into the request's
// own run of the block k_cull reads (fot_batch::static_off layout).  16-byte rows, coalesced both ways.
__global__ void __launch_bounds__(256)
k_static_gather(const StaticGather *__restrict__ tab, int n_req, const double2 *__restrict__ points, double2 *__restrict__ out)
{
    const int j = blockIdx.x;
    if (j >= n_req) return;
    const int src = tab[j].src, dst = tab[j].dst, n = tab[j].n;
    for (int p = threadIdx.x; p < n; p += 256) out[dst + p] = points[src + p];
}

// one thread per (row, axis) of the frame; the arithmetic of k_resample's cv = 2 path, operation for operation
__global__ void k_predict_cv_frame(double sgan_dt, double sim_dt, double staleness, int n_rows, int n_dense, FrameDev f,
                                   double *__restrict__ out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * 2) return;
    const int ax = idx & 1, p = idx >> 1;
    const int e = f.ped_ep[p], p0 = f.ped0[e], pre = f.prepend[e] ? 1 : 0;
    const int T = n_dense + pre;
    double *dst = out + 2 * (f.blk[e] + (int64_t)(p - p0) * T) + ax;
    if (pre) dst[0] = f.pos[2 * p + ax];
    dst += 2 * pre;
    const double cur = f.last[2 * p + ax];                          // obs_last
    const double vel = (double)(((float)cur - (float)f.prev[2 * p + ax]) / (float)sgan_dt);
    for (int i = 0; i < n_dense; ++i) {
        const double t = (sim_dt + (double)i * sim_dt) + staleness;
        dst[2 * i] = (double)(cur + vel * t);
    }
}

// One workgroup: eight lanes per record, one 16-byte store each into the pinned digest; every wave releases its stores
// at system scope before the barrier behind which thread 0 raises the completion word the host polls (the ordering of
// record_written, for any number of records).
__global__ void __launch_bounds__(256)
k_loop_digest(const fot_result *__restrict__ rec, int n, LoopDigest *out, int32_t *done, int32_t seq)
{
    for (int c = threadIdx.x; c < 8 * n; c += 256) {
        const int r = c >> 3, j = c & 7;
        double2 v;
        if (j < 5) v = ((const double2 *)(rec + r))[j];                   // the header up to new_prev_s, as it is
        else if (j == 5) { v.x = rec[r].x[1]; v.y = rec[r].y[1]; }
        else if (j == 6) { v.x = rec[r].yaw[1]; v.y = rec[r].v[1]; }
        else { v.x = rec[r].a[1]; v.y = 0.0; }
        ((double2 *)(out + r))[j] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Workgroup i copies the followed record of running episode i into the step's history block; workgroup 0 first raises
// the step's completion word: this launch runs behind the step's last kernels on its stream, whose results in pinned
// memory are complete when it starts.
__global__ void __launch_bounds__(256)
k_loop_history(const fot_result *__restrict__ rec, int n_run, const int32_t *__restrict__ src,
               const int32_t *__restrict__ slot, double *__restrict__ hist, int n_slots, int n_total, int32_t *done,
               int32_t seq)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int i = blockIdx.x;
    if (!hist || i >= n_run) return;
    const int r = src[i];
    if (r < 0) return;
    const double *from = rec[r].t;                                   // the 15 arrays lie back to back, FOT_MAX_NT apart
    double *to = hist + (int64_t)slot[i] * n_total;
    for (int c = threadIdx.x; c < 15 * n_total; c += 256) {
        const int f = c / n_total, k = c - f * n_total;
        to[(int64_t)f * n_slots * n_total + k] = from[f * FOT_MAX_NT + k];
    }
}

// ---------------------------------------------------------------------------
// fot_loop_summaries: the prediction error of a resident loop, accumulated while it runs (fot_summary.hpp)
// ---------------------------------------------------------------------------

// One workgroup per running episode, behind the step's prediction.  Row c[k] = sum_p |pred[p][k] - recording[f_cur + 1 +
// k][p]| of this step goes into place step % n_dense of the slot's ring; the row it replaces -- the one of step - n_dense,
// whose horizon is complete now -- is folded into the slot's totals first, by thread 0 from a copy in LDS.
// Lanes: G = the power of two >= P (at most 64) lanes side by side take the pedestrians of one dense sample, so a
// recording row's [P][2] run is read as adjacent 16-byte loads; 256 / G samples are in flight per pass.  The sum over the
// pedestrians is a butterfly over the G lanes: its order depends on P alone, never on the other slots or on timing.
__global__ void __launch_bounds__(256)
k_loop_pred_error(ReplayView rv, const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn, int n_run,
                  int have_pred, int f_cur, int step, SummaryShape S, double *__restrict__ ring,
                  int32_t *__restrict__ ring_P, SummaryTotals *__restrict__ totals, const int32_t *__restrict__ best)
{
    __shared__ double old_row[FOT_MAX_NT];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= n_run) return;
    const int slot = slot_of[i], nd = S.n_dense, r = step % nd;
    double *row = ring + ((int64_t)slot * nd + r) * nd;
    int32_t *row_P = ring_P + (int64_t)slot * nd + r;
    for (int k = tid; k < nd; k += 256) old_row[k] = row[k];
    __syncthreads();
    const int p0 = f.ped0[i], P = have_pred ? f.ped0[i + 1] - p0 : 0;
    if (tid == 0) {
        const int old_P = *row_P;
        if (step >= nd && old_P > 0) {
            SummaryTotals T = totals[slot];
            summary_fold_row(T, S, old_row, old_P, step - nd, step + 1);
            totals[slot] = T;
        }
        *row_P = P > 0 ? P : 0;
    }
    if (P <= 0) {
        for (int k = tid; k < nd; k += 256) row[k] = 0.0;
        return;
    }
    const int pre = f.prepend[i] ? 1 : 0, T_blk = nd + pre;
    // [P][T_blk], the prepended column skipped below; of a distribution [S][P][T_blk]: the slot's representative sample
    const double2 *pred = (const double2 *)dyn + f.blk[i] + (best ? (int64_t)max(best[slot], 0) * P * T_blk : 0);
    const double2 *rec = (const double2 *)rv.pos + rv.slot_ped0[slot];
    const int last_row = rv.slot_frames[slot] - 1;
    const int64_t cols = rv.n_cols;
    int G = 1;
    while (G < P && G < WAVE) G <<= 1;
    const int per_pass = 256 / G, g = tid / G, lane = tid & (G - 1);
    for (int base = 0; base < nd; base += per_pass) {               // (uniform trip count: every lane takes part in the butterfly)
        const int k = base + g;
        double acc = 0.0;
        if (k < nd) {
            const int64_t gt_row = (int64_t)min(f_cur + 1 + k, last_row) * cols;
            for (int p = lane; p < P; p += G) {
                const double2 q = pred[(int64_t)p * T_blk + pre + k], w = rec[gt_row + p];
                acc += sqrt(sum_sq_unfused(q.x - w.x, q.y - w.y));
            }
        }
        for (int m = G >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, WAVE);
        if (k < nd && lane == 0) row[k] = acc;
    }
}

// One workgroup per slot, on request: thread t forms the terms of the ring's t-th oldest row under the slot's current
// length L (its truncated horizon), thread 0 adds them to a COPY of the totals in step order and writes the
// prediction-error keys of the slot's record in pinned memory.  Ring and totals are left as they are.
__global__ void __launch_bounds__(256)
k_loop_summary(SummaryShape S, const double *__restrict__ ring, const int32_t *__restrict__ ring_P,
               const SummaryTotals *__restrict__ totals, const int32_t *__restrict__ steps, int n_slots, int num_samples,
               fot_loop_summary *out)
{
    __shared__ SummaryTerms terms[FOT_MAX_NT];
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (slot >= n_slots) return;
    const int L = steps[slot], nd = S.n_dense;
    const int first = L > nd ? L - nd : 0, n_tail = L - first;
    for (int t = tid; t < n_tail; t += 256) {
        const int i = first + t, r = i % nd;
        terms[t] = summary_row_terms(S, ring + ((int64_t)slot * nd + r) * nd, ring_P[(int64_t)slot * nd + r], i, L);
    }
    __syncthreads();
    if (tid != 0) return;
    SummaryTotals T = totals[slot];
    for (int t = 0; t < n_tail; ++t) summary_add_terms(T, terms[t]);
    double m[4];
    summary_means(T, m);
    fot_loop_summary *o = out + slot;
    o->ade = m[0]; o->fde = m[1]; o->ade_per_agent = m[0]; o->fde_per_agent = m[1];
    o->planning_ade = m[2]; o->planning_fde = m[3];
    o->nll = __builtin_nan("");
    o->pred_samples = T.std_count > 0 ? num_samples : 0;
    o->ade_eval_count = (int32_t)T.std_count; o->planning_eval_count = (int32_t)T.plan_count;
    o->nll_eval_count = 0;
}

// ---------------------------------------------------------------------------
// fot_loop_scores_enable (fot_loopscore.hpp): a resident sampler loop scores its predictor while it runs
// ---------------------------------------------------------------------------

// One workgroup per running episode, behind the ragged resample: the representative sample of the episode's
// [S][P][n_dense + 1][2] block (predict_single_best).  Lanes run over the (p, k) points of the dense tracks, 256 a pass
// (adjacent lanes: adjacent samples k of a track); a lane forms its point's mean over the samples in index order, then
// its deviation from every sample; the lanes of a wave meet in a butterfly per sample and pass, the passes add up in a
// slot of LDS per (sample, wave), the waves in index order: the order of every sum follows from (S, P, n_dense) alone,
// so an episode chooses the same sample alone and in any batch.  An episode without pedestrians has no distribution: -1.
constexpr int BS_THREADS = 256;
constexpr int BS_WAVES = BS_THREADS / WAVE;

// (the body of both forms: running episode i = blockIdx.x, checked by the caller)
// ROWS: the rows of the per-sample tables in LDS (S <= ROWS, checked by the launcher); dev_stride: the row stride of dev_tab
// (the narrow forms hand in the constant FOT_MAX_SAMPLES, the wide ones their launch argument)
static_assert(FOT_MAX_PLAN_SAMPLES <= BS_THREADS, "the fold of the waves' columns: one thread per sample (tid < S)");
template <int ROWS>
__device__ __forceinline__ void
best_sample_episode(const int32_t *__restrict__ slot_of, const FrameDev &f, const double *__restrict__ dyn, int S,
                    int n_dense, double *__restrict__ dev_tab, int dev_stride, int32_t *__restrict__ best_tab,
                    int32_t *best_host)
{
    __shared__ double s_part[ROWS][BS_WAVES];
    __shared__ double s_dev[ROWS];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int slot = slot_of[i], p0 = f.ped0[i], P = f.ped0[i + 1] - p0;
    if (P <= 0) {                                                    // (uniform)
        if (tid == 0) { best_tab[slot] = -1; best_host[slot] = -1; }
        return;
    }
    const int T = n_dense + 1, n = P * n_dense;
    const int64_t sample_pts = (int64_t)P * T;
    const double2 *blk = (const double2 *)dyn + f.blk[i];
    for (int c = tid; c < ROWS * BS_WAVES; c += BS_THREADS) (&s_part[0][0])[c] = 0.0;
    __syncthreads();
    for (int base = 0; base < n; base += BS_THREADS) {               // (uniform trip count: the butterflies)
        const int idx = base + tid;
        const bool active = idx < n;
        const int p = idx / n_dense, k = idx - p * n_dense;
        const double2 *e = blk + (int64_t)p * T + 1 + k;             // sample s: e[s * sample_pts]; the prepended entry skipped
        double mx = 0.0, my = 0.0;
        if (active) {
            for (int s = 0; s < S; ++s) {
                const double2 v = e[s * sample_pts];
                mx += v.x; my += v.y;
            }
            mx /= (double)S; my /= (double)S;
        }
        for (int s = 0; s < S; ++s) {
            double d = 0.0;
            if (active) {
                const double2 v = e[s * sample_pts];
                d = bs_dev(v.x, v.y, mx, my);
            }
            d = wave_sum_f64(d);
            if (lane == 0) s_part[s][wave] += d;                     // (this wave's own column)
        }
    }
    __syncthreads();
    if (tid < S) {
        double t = s_part[tid][0];
        for (int w = 1; w < BS_WAVES; ++w) t += s_part[tid][w];
        s_dev[tid] = t;
        dev_tab[(int64_t)slot * dev_stride + tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        const int best = bs_first_min(S, s_dev);
        best_tab[slot] = best; best_host[slot] = best;
    }
}

__global__ void __launch_bounds__(BS_THREADS)
k_loop_best_sample(const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn, int n_run, int S,
                   int n_dense, double *__restrict__ dev_tab, int32_t *__restrict__ best_tab, int32_t *best_host)
{
    if ((int)blockIdx.x >= n_run) return;
    best_sample_episode<FOT_MAX_SAMPLES>(slot_of, f, dyn, S, n_dense, dev_tab, FOT_MAX_SAMPLES, best_tab, best_host);
}

// The wide form: S > FOT_MAX_SAMPLES on a handle with a raised sample capacity.  The same body over tables of
// FOT_MAX_PLAN_SAMPLES rows (254 x 4 + 254 doubles, 10 KB); dev_tab's rows are dev_stride apart.  The shape of the sums is
// the narrow form's -- a butterfly per (sample, pass, wave), the passes in order, the waves in index order.
__global__ void __launch_bounds__(BS_THREADS)
k_loop_best_sample_wide(const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn, int n_run, int S,
                        int n_dense, double *__restrict__ dev_tab, int dev_stride, int32_t *__restrict__ best_tab,
                        int32_t *best_host)
{
    if ((int)blockIdx.x >= n_run) return;
    best_sample_episode<FOT_MAX_PLAN_SAMPLES>(slot_of, f, dyn, S, n_dense, dev_tab, dev_stride, best_tab, best_host);
}

// The sweep form (fot_sweep.hpp): only the episodes whose table row asks for it choose; the others leave their slot's
// entries alone (the host reads them for chosen episodes only).  An episode's sums are the uniform form's, bit for bit.
__global__ void __launch_bounds__(BS_THREADS)
k_loop_best_sample_sweep(const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn,
                         const SweepEp *__restrict__ tab, int n_run, int S, int n_dense, double *__restrict__ dev_tab,
                         int32_t *__restrict__ best_tab, int32_t *best_host)
{
    if ((int)blockIdx.x >= n_run || tab[blockIdx.x].select == 0) return;     // (uniform)
    best_sample_episode<FOT_MAX_SAMPLES>(slot_of, f, dyn, S, n_dense, dev_tab, FOT_MAX_SAMPLES, best_tab, best_host);
}

__global__ void __launch_bounds__(BS_THREADS)
k_loop_best_sample_sweep_wide(const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn,
                              const SweepEp *__restrict__ tab, int n_run, int S, int n_dense, double *__restrict__ dev_tab,
                              int dev_stride, int32_t *__restrict__ best_tab, int32_t *best_host)
{
    if ((int)blockIdx.x >= n_run || tab[blockIdx.x].select == 0) return;     // (uniform)
    best_sample_episode<FOT_MAX_PLAN_SAMPLES>(slot_of, f, dyn, S, n_dense, dev_tab, dev_stride, best_tab, best_host);
}

// The sweep forms with a sample count per slot (fot_loop_set_slot_samples): episode i chooses among its own ep_S[i]
// samples -- one scalar load, uniform for the workgroup.  The shape of the sums is unchanged (lanes over (p, k), a butterfly
// per (sample, pass, wave), the passes in order, the waves in index order), so a slot chooses what the uniform loop of its
// count chooses.  The narrow form serves a step whose running counts are all <= FOT_MAX_SAMPLES; dev_tab's rows are
// dev_stride apart in both.
__global__ void __launch_bounds__(BS_THREADS)
k_loop_best_sample_slots(const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn,
                         const SweepEp *__restrict__ tab, const int32_t *__restrict__ ep_S, int n_run, int n_dense,
                         double *__restrict__ dev_tab, int dev_stride, int32_t *__restrict__ best_tab, int32_t *best_host)
{
    if ((int)blockIdx.x >= n_run || tab[blockIdx.x].select == 0) return;     // (uniform)
    best_sample_episode<FOT_MAX_SAMPLES>(slot_of, f, dyn, ep_S[blockIdx.x], n_dense, dev_tab, dev_stride, best_tab, best_host);
}

__global__ void __launch_bounds__(BS_THREADS)
k_loop_best_sample_slots_wide(const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn,
                              const SweepEp *__restrict__ tab, const int32_t *__restrict__ ep_S, int n_run, int n_dense,
                              double *__restrict__ dev_tab, int dev_stride, int32_t *__restrict__ best_tab, int32_t *best_host)
{
    if ((int)blockIdx.x >= n_run || tab[blockIdx.x].select == 0) return;     // (uniform)
    best_sample_episode<FOT_MAX_PLAN_SAMPLES>(slot_of, f, dyn, ep_S[blockIdx.x], n_dense, dev_tab, dev_stride, best_tab, best_host);
}

// One thread per (row of the frame, evaluation step j): the truth of the step's origins, [rows][E][2], from the resident
// recording -- row min(f_cur + stride (j + 1), frames - 1) of the pedestrian's slot (a shorter recording holds its last frame).
__global__ void __launch_bounds__(256)
k_loop_score_truth(ReplayView rv, const int32_t *__restrict__ slot_of, FrameDev f, int n_rows, int f_cur, int stride, int E,
                   double2 *__restrict__ out)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_rows * E) return;
    const int p = idx / E, j = idx - p * E;
    const int e = f.ped_ep[p], slot = slot_of[e];
    const int row = min(f_cur + stride * (j + 1), rv.slot_frames[slot] - 1);
    out[idx] = ((const double2 *)rv.pos)[(int64_t)row * rv.n_cols + rv.slot_ped0[slot] + (p - f.ped0[e])];
}

// ---------------------------------------------------------------------------
// fot_loop_plan_sample (fot_repsample.hpp): the step's requests plan against every episode's representative sample
// ---------------------------------------------------------------------------

// One workgroup per running episode, behind k_loop_best_sample: the episode's [P][n_dense + 1][2] planning block from
// sample best_tab[slot] of its [S][P][n_dense + 1][2] distribution block.  The lanes first AND np.allclose(first dense
// sample, current position) over the episode's pedestrians (a ballot per wave, the waves' answers side by side in LDS: no
// atomics, the same answer for any number of lanes), then copy: adjacent lanes take adjacent time entries of a track, one double2 each.  The flag goes to
// pre_dev[i] (HBM) and pre_host[i] (pinned).  An episode without pedestrians writes nothing.
constexpr int RB_THREADS = 256;

// (the body of both forms: running episode i = blockIdx.x, checked by the caller; the block starts at point out_pt of rep)
__device__ __forceinline__ void
rep_block_episode(const int32_t *__restrict__ slot_of, const FrameDev &f, const double *__restrict__ dyn,
                  const int32_t *__restrict__ best_tab, int S, int n_dense, double *__restrict__ rep, int64_t out_pt,
                  int32_t *__restrict__ pre_dev, int32_t *pre_host)
{
    __shared__ int s_far[RB_THREADS / WAVE];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int p0 = f.ped0[i], P = f.ped0[i + 1] - p0;
    if (P <= 0) return;                                              // (uniform)
    const int T = n_dense + 1, n = P * T;
    const int best = min(max(best_tab[slot_of[i]], 0), S - 1);       // (k_loop_best_sample's choice: always in range)
    const double2 *src = (const double2 *)dyn + f.blk[i] + (int64_t)best * P * T;
    const double2 *cur = (const double2 *)f.pos + p0;
    int close = 1;
    for (int p = tid; p < P; p += RB_THREADS) {
        const double2 a = src[(int64_t)p * T + 1], c = cur[p];
        close &= rs_close_xy(a.x, a.y, c.x, c.y) ? 1 : 0;
    }
    // the vote: every wave's ballot into its own slot of LDS (plain stores), every lane reads all of them
    const unsigned long long far_lanes = __ballot(close == 0);
    if (lane == 0) s_far[wave] = far_lanes != 0ull ? 1 : 0;
    __syncthreads();
    int far = 0;
    for (int w = 0; w < RB_THREADS / WAVE; ++w) far |= s_far[w];
    const bool prepend = far != 0;
    double2 *out = (double2 *)rep + out_pt;
    for (int idx = tid; idx < n; idx += RB_THREADS) {
        const int p = idx / T, t = idx - p * T;
        out[idx] = prepend && t == 0 ? cur[p] : src[(int64_t)p * T + rs_src(t, T, prepend)];
    }
    if (tid == 0) { pre_dev[i] = prepend ? 1 : 0; pre_host[i] = prepend ? 1 : 0; }
}

__global__ void __launch_bounds__(RB_THREADS)
k_loop_rep_block(const int32_t *__restrict__ slot_of, FrameDev f, const double *__restrict__ dyn,
                 const int32_t *__restrict__ best_tab, int n_run, int S, int n_dense, double *__restrict__ rep,
                 int32_t *__restrict__ pre_dev, int32_t *pre_host)
{
    const int i = blockIdx.x;
    if (i >= n_run) return;
    rep_block_episode(slot_of, f, dyn, best_tab, S, n_dense, rep, (int64_t)f.ped0[i] * (n_dense + 1), pre_dev, pre_host);
}

// The sweep form (fot_sweep.hpp): the episodes in representative mode write their blocks into the step's tensor itself,
// at the compacted offsets behind the distribution blocks (which are only read: the two regions never overlap).
__global__ void __launch_bounds__(RB_THREADS)
k_loop_rep_block_sweep(const int32_t *__restrict__ slot_of, FrameDev f, const double *dyn, const SweepEp *__restrict__ tab,
                       const int32_t *__restrict__ best_tab, int n_run, int S, int n_dense, double *tensor,
                       int32_t *__restrict__ pre_dev, int32_t *pre_host)
{
    const int i = blockIdx.x;
    if (i >= n_run || !sweep_plans_on_block(tab[i])) return;             // (uniform)
    rep_block_episode(slot_of, f, dyn, best_tab, S, n_dense, tensor, tab[i].rep_off, pre_dev, pre_host);
}

// ... with a sample count per slot: the clamp of the choice and the source's sample stride are the episode's own.
__global__ void __launch_bounds__(RB_THREADS)
k_loop_rep_block_slots(const int32_t *__restrict__ slot_of, FrameDev f, const double *dyn, const SweepEp *__restrict__ tab,
                       const int32_t *__restrict__ ep_S, const int32_t *__restrict__ best_tab, int n_run, int n_dense,
                       double *tensor, int32_t *__restrict__ pre_dev, int32_t *pre_host)
{
    const int i = blockIdx.x;
    if (i >= n_run || !sweep_plans_on_block(tab[i])) return;             // (uniform)
    rep_block_episode(slot_of, f, dyn, best_tab, ep_S[i], n_dense, tensor, tab[i].rep_off, pre_dev, pre_host);
}

// ---------------------------------------------------------------------------
// fot_openloop_eval (fot_openloop.hpp): the rows of a chunk of windows out of the resident scene
// ---------------------------------------------------------------------------
// One workgroup per OL_TILE_ROWS rows of the chunk.  Row r reads scene point (row_f0[r] + t, row_col[r]) for t = 0 ..
// obs_len + pred_len - 1.  A frame's columns are contiguous and the rows of a window are mostly ascending columns, so the
// lanes run over the ROWS of one frame and the waves over the frames: a wave's loads fall into one or two runs of a
// frame's columns.  The observation window [obs_len][rows][2] has the rows innermost too: a wave stores 64 adjacent
// float2.  The truth [rows][pred_len][2] has them outermost -- a tile's block of it is ONE contiguous run, so the loads
// go through LDS (row-major, as the block lies in HBM) and the block is written out linearly, adjacent lanes adjacent
// double2.  No atomics; every output element is written once by one thread.
constexpr int OL_THREADS = 256;
static_assert(OL_THREADS % OL_TILE_ROWS == 0 && OL_MAX_PRED_LEN == FOT_MAX_PRED_LEN, "tile rows divide the workgroup");

template <typename V2>
__global__ void __launch_bounds__(OL_THREADS)
k_openloop_rows(OpenLoopRows A)
{
    __shared__ double2 s_truth[OL_TILE_ROWS * FOT_MAX_PRED_LEN];         // 32 KB
    const V2 *__restrict__ scene = (const V2 *)A.scene;
    const int row0 = blockIdx.x * OL_TILE_ROWS;
    const int tile_rows = min(OL_TILE_ROWS, A.rows - row0);               // >= 1: the grid is ceil(rows / tile)
    const int lr = threadIdx.x % OL_TILE_ROWS, t_first = threadIdx.x / OL_TILE_ROWS;
    constexpr int T_STEP = OL_THREADS / OL_TILE_ROWS;
    if (lr < tile_rows) {
        const int r = row0 + lr;
        const int32_t f0 = A.row_f0[r], col = A.row_col[r];
        for (int t = t_first; t < A.obs_len; t += T_STEP) {
            const V2 v = scene[ol_scene_point(f0, t, A.n_cols, col)];
            const float2 o = make_float2(ol_observe((double)v.x), ol_observe((double)v.y));
            A.obs[(int64_t)t * A.rows + r] = o;
            if (t == A.obs_len - 1) A.anchor[r] = make_double2((double)o.x, (double)o.y);
        }
        for (int j = t_first; j < A.pred_len; j += T_STEP) {
            const V2 v = scene[ol_scene_point(f0, A.obs_len + j, A.n_cols, col)];
            s_truth[lr * A.pred_len + j] = make_double2((double)v.x, (double)v.y);
        }
    }
    __syncthreads();
    double2 *__restrict__ dst = A.truth + (int64_t)row0 * A.pred_len;
    for (int i = threadIdx.x; i < tile_rows * A.pred_len; i += OL_THREADS) dst[i] = s_truth[i];
}

// ---------------------------------------------------------------------------
// fot_footprint_recheck (fot_footprint_obs.hpp): centre, circle cover and exact rectangle, observed per step
// ---------------------------------------------------------------------------
// One wave per pose, as k_safety.  cos / sin once per wave; lanes over the pedestrians for the centre and the rectangle,
// over the (circle, pedestrian) pairs for the cover.  A pose without pedestrians writes +inf three times.  No atomics.
__global__ void __launch_bounds__(WAVE)
k_footprint_steps(const FpoGeom *__restrict__ geom, int n, const double *__restrict__ xy, int xy_stride,
                  const double *__restrict__ yaw, int yaw_stride, const int32_t *__restrict__ ped_off,
                  const double *__restrict__ ped_xy, FpoStep *__restrict__ out)
{
    const int i = blockIdx.x;
    if (i >= n) return;
    const FpoGeom &G = *geom;
    const double x = xy[(int64_t)i * xy_stride], y = xy[(int64_t)i * xy_stride + 1];
    const double a = yaw[(int64_t)i * yaw_stride];
    const double c = cos(a), s = sin(a);
    const int p0 = ped_off[i], np_ = ped_off[i + 1] - p0;
    const double *__restrict__ peds = ped_xy + 2 * (int64_t)p0;  // (8-byte loads: a frame's rows need not be 16-byte aligned)
    double legacy = INFINITY, multi = INFINITY, rect = INFINITY;
    for (int p = threadIdx.x; p < np_; p += WAVE) {
        double2 q;
        q.x = peds[2 * p]; q.y = peds[2 * p + 1];
        legacy = fmin(legacy, fpo_legacy(q.x, q.y, x, y));
        rect = fmin(rect, fpo_rect(q.x, q.y, x, y, c, s, G.half_l, G.half_w));
    }
    const int pairs = G.n_circles * np_;
    for (int j = threadIdx.x; j < pairs; j += WAVE) {
        const int k = j / np_, p = j - k * np_;
        double2 q;
        q.x = peds[2 * p]; q.y = peds[2 * p + 1];
        const double off = G.off[k];
        multi = fmin(multi, fpo_multi(q.x, q.y, fpo_centre(x, off, c), fpo_centre(y, off, s)));
    }
    legacy = wave_min_f64(legacy); multi = wave_min_f64(multi); rect = wave_min_f64(rect);
    if (threadIdx.x == 0) {
        FpoStep r;
        r.legacy = legacy; r.multi = multi; r.rect = rect;
        out[i] = r;
    }
}

constexpr int FPO_THREADS = 256;
constexpr int FPO_WAVES = FPO_THREADS / WAVE;

// One workgroup per trajectory: the heading of every step from the central differences of its positions, a standing
// step holding the heading of the last moving one.  The hold is an inclusive scan of (source step, heading) in chunks of
// the workgroup's width: a butterfly-free shift scan within a wave, the waves' totals through LDS, the carry of the
// chunks before in every thread's registers (all threads form the same carry).  The steps in front of the first moving
// one are written last, once that step is known; a trajectory that never moves is all zeros.  Every element of yaw_out
// is written once.
__global__ void __launch_bounds__(FPO_THREADS)
k_footprint_yaw(const int32_t *__restrict__ step_off, const double *__restrict__ xy, double *__restrict__ yaw_out)
{
    __shared__ int32_t s_src[FPO_WAVES];
    __shared__ double s_yaw[FPO_WAVES];
    __shared__ int32_t s_first[FPO_WAVES];
    __shared__ double s_first_yaw;
    const int i0 = step_off[blockIdx.x], n = step_off[blockIdx.x + 1] - i0;
    const double *__restrict__ q = xy + 2 * (int64_t)i0;
    double *__restrict__ out = yaw_out + i0;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    auto X = [&](int i) { return q[2 * i]; };
    auto Y = [&](int i) { return q[2 * i + 1]; };
    FpoHold carry;
    carry.src = -1; carry.yaw = 0.0;
    int my_first = INT32_MAX;
    double my_first_yaw = 0.0;
    for (int c0 = 0; c0 < n; c0 += FPO_THREADS) {
        const int i = c0 + tid;
        FpoHold h;
        h.src = -1; h.yaw = 0.0;
        if (i < n) {
            const double dx = fpo_gradient(X, i, n), dy = fpo_gradient(Y, i, n);
            if (fpo_moving(dx, dy)) {
                h.src = i; h.yaw = atan2(dy, dx);
                if (my_first == INT32_MAX) { my_first = i; my_first_yaw = h.yaw; }
            }
        }
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            FpoHold o;
            o.src = __shfl_up(h.src, off, WAVE); o.yaw = __shfl_up(h.yaw, off, WAVE);
            if (lane >= off) h = fpo_hold_join(o, h);
        }
        if (lane == WAVE - 1) { s_src[wave] = h.src; s_yaw[wave] = h.yaw; }
        __syncthreads();
        FpoHold next = carry;                                        // the carry after this chunk: the same in every thread
        for (int w = 0; w < FPO_WAVES; ++w) {
            if (w == wave) h = fpo_hold_join(next, h);               // (next: the carry joined with the waves before this one)
            FpoHold t;
            t.src = s_src[w]; t.yaw = s_yaw[w];
            next = fpo_hold_join(next, t);
        }
        if (i < n && h.src >= 0) out[i] = h.yaw;
        carry = next;
        __syncthreads();                                             // the next chunk writes s_src / s_yaw again
    }
    int first = my_first;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off, WAVE));
    if (lane == 0) s_first[wave] = first;
    __syncthreads();
    first = s_first[0];
    for (int w = 1; w < FPO_WAVES; ++w) first = min(first, s_first[w]);
    const bool any_moving = first != INT32_MAX;
    if (any_moving && my_first == first) s_first_yaw = my_first_yaw; // (one thread: the chunk's owner of that step)
    __syncthreads();
    FpoHold none;
    none.src = -1; none.yaw = 0.0;
    const double lead = fpo_hold_pick(none, any_moving, any_moving ? s_first_yaw : 0.0);
    const int n_lead = any_moving ? first : n;
    for (int i = tid; i < n_lead; i += FPO_THREADS) out[i] = lead;
}

// One workgroup per trajectory: the minima and the counts of its steps' records.  Minima and integer sums: the result
// does not depend on the order, so lanes stride over the steps, the wave folds with shuffles and the waves meet in LDS.
__global__ void __launch_bounds__(FPO_THREADS)
k_footprint_fold(const FpoGeom *__restrict__ geom, const int32_t *__restrict__ step_off, const int32_t *__restrict__ ped_off,
                 const FpoStep *__restrict__ series, FpoRecord *__restrict__ out)
{
    __shared__ FpoAcc s_acc[FPO_WAVES];
    const FpoGeom &G = *geom;
    const int i0 = step_off[blockIdx.x], n = step_off[blockIdx.x + 1] - i0;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    FpoAcc a = fpo_acc_zero();
    for (int i = tid; i < n; i += FPO_THREADS) {
        const FpoStep r = series[i0 + i];
        fpo_acc_step(a, G, r.legacy, r.multi, r.rect, ped_off[i0 + i + 1] > ped_off[i0 + i]);
    }
    a.legacy = wave_min_f64(a.legacy); a.multi = wave_min_f64(a.multi); a.rect = wave_min_f64(a.rect);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.n_legacy += __shfl_xor(a.n_legacy, off, WAVE); a.n_multi += __shfl_xor(a.n_multi, off, WAVE);
        a.n_rect += __shfl_xor(a.n_rect, off, WAVE); a.with_peds += __shfl_xor(a.with_peds, off, WAVE);
    }
    if (lane == 0) s_acc[wave] = a;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < FPO_WAVES; ++w) fpo_acc_merge(a, s_acc[w]);
    out[blockIdx.x] = fpo_acc_record(a, G, n);
}

// ---------------------------------------------------------------------------
// fot_fidelity_eval (fot_fidelity.hpp): separation series, avoidance onset and roll-out error of ragged encounters
// ---------------------------------------------------------------------------
constexpr int FID_THREADS = 256;

// the encounter that owns entry g of a table of n + 1 non-decreasing offsets from 0: the LAST e with off[e] <= g (an
// encounter without entries shares its offset with the next one and is never the answer); g < off[n]
template <typename T>
__device__ __forceinline__ int fid_owner(const T *__restrict__ off, int n, int64_t g)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Lane = pedestrian, over all encounters' pedestrians back to back, so that waves stay full however small the crowds
// are: the rows [t][0 .. N) are contiguous over the lanes of an encounter.  Each lane walks its own steps in ascending
// order with a sliding window of three velocities and leaves the walk at its first onset; the wave leaves when all of
// its lanes have.  With a truth array a second walk over all steps sums the pedestrian's error.  Nothing is shared
// between lanes: what a pedestrian gets depends on its encounter alone.
__global__ void __launch_bounds__(FID_THREADS)
k_fidelity_peds(FidelityArgs A)
{
    const int64_t g = (int64_t)blockIdx.x * FID_THREADS + threadIdx.x;
    if (g >= A.n_peds) return;
    const int e = fid_owner(A.ped_base, A.n_enc, g);
    const int64_t j = g - A.ped_base[e], N = A.n_ped[e];
    const int s0 = A.step_off[e], T = A.step_off[e + 1] - s0;
    const double dt = A.dt[e];
    const double *__restrict__ eg = A.ego + 2 * (int64_t)s0;
    const int64_t first = 2 * (A.row_off[e] + j), stride = 2 * N;   // (t, c) of this pedestrian: first + t stride + c
    const double *__restrict__ xy = A.ped_xy + first;
    auto pos = [&](int t, int c) { return xy[t * stride + c]; };
    auto ego = [&](int t, int c) { return eg[2 * t + c]; };
    int32_t step;
    double dist, away;
    if (A.ped_vel) {
        const double *__restrict__ v = A.ped_vel + first;
        auto vel = [&](int t, int c) { return v[t * stride + c]; };
        fid_onset(pos, vel, ego, T, dt, A.p, &step, &dist, &away);
    } else {
        auto vel = [&](int t, int c) { return fid_gradient([&](int s) { return xy[s * stride + c]; }, t, T, dt); };
        fid_onset(pos, vel, ego, T, dt, A.p, &step, &dist, &away);
    }
    A.onset_step[g] = step;
    A.onset_dist[g] = dist;
    if (A.truth) {
        const double *__restrict__ q = A.truth + first;
        auto truth = [&](int t, int c) { return q[t * stride + c]; };
        double sum;
        int32_t keep;
        fid_ped_error(pos, truth, ego, T, A.p.interaction_distance, &sum, &keep);
        A.ped_sum[g] = sum;
        A.ped_keep[g] = keep;
    }
}

// Lane = step, over all encounters' steps back to back: the minimum over the step's pedestrians in ascending order, as
// np.min forms it (a NaN stays).  A lane reads its row of N positions front to back; neighbouring lanes own
// neighbouring rows, so every line fetched is used whole.
__global__ void __launch_bounds__(FID_THREADS)
k_fidelity_series(FidelityArgs A)
{
    const int64_t g = (int64_t)blockIdx.x * FID_THREADS + threadIdx.x;
    if (g >= A.n_steps) return;
    const int e = fid_owner(A.step_off, A.n_enc, g);
    const int t = (int)(g - A.step_off[e]), N = A.n_ped[e];
    const double *__restrict__ r = A.ped_xy + 2 * (A.row_off[e] + (int64_t)t * N);
    auto row = [&](int j, int c) { return r[2 * j + c]; };
    A.series[g] = fid_separation(row, N, A.ego[2 * g], A.ego[2 * g + 1]);
}

// One wave per encounter: the series' minimum and its first step (lanes stride over the steps, the wave joins with
// shuffles: the join is exact in any order), then lane 0 adds the kept pedestrians' error sums in ascending order.
__global__ void __launch_bounds__(WAVE)
k_fidelity_fold(FidelityArgs A)
{
    const int e = blockIdx.x;
    if (e >= A.n_enc) return;
    const int s0 = A.step_off[e], T = A.step_off[e + 1] - s0, N = A.n_ped[e];
    FidMin m = fid_min_zero();
    for (int t = threadIdx.x; t < T; t += WAVE) m = fid_min_take(m, A.series[s0 + t], t);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        FidMin o;
        o.v = __shfl_xor(m.v, off, WAVE); o.step = __shfl_xor(m.step, off, WAVE); o.nan = __shfl_xor(m.nan, off, WAVE);
        m = fid_min_join(m, o);
    }
    if (threadIdx.x != 0) return;
    const int64_t b = A.ped_base[e];
    const bool have_truth = A.truth != nullptr;
    A.out[e] = fid_record(m, T, N, have_truth, [&](int j) { return A.ped_sum[b + j]; }, [&](int j) { return A.ped_keep[b + j] != 0; },
                          [&](int j) { return A.onset_step[b + j]; });
}

// ---------------------------------------------------------------------------
// fot_encounters_extract (fot_encounter.hpp): populations and closest approaches of candidate spans of a resident clip,
// the kept encounters gathered into fot_fidelity_eval's packed layout, cruise speeds and far goals
// ---------------------------------------------------------------------------
// coordinate c of column a at frame f of the clip, and of its velocity (recorded, or the whole-grid fallback)
__device__ __forceinline__ double enc_pos_at(const EncScene &s, int64_t f, int a, int c) { return s.ped_xy[2 * (f * s.A + a) + c]; }
__device__ __forceinline__ double enc_vel_at(const EncScene &s, int64_t f, int a, int c)
{
    if (s.ped_vel) return s.ped_vel[2 * (f * s.A + a) + c];
    return enc_fallback_vel([&](int32_t t, int cc) { return enc_pos_at(s, t, a, cc); }, (int32_t)f, s.T, c, s.dt);
}

// Block = 64 columns of one span (the spans' tiles back to back); lane = column, so that a step's row is read in whole lines; wave w walks the
// steps w, w + ENC_STEP_WAVES, ...  and wave 0 joins the four shares (the join is exact in any order).
__global__ void __launch_bounds__(ENC_COL_TILE * ENC_STEP_WAVES)
k_enc_columns(EncSpansArgs A)
{
    __shared__ EncCol s_c[ENC_STEP_WAVES][ENC_COL_TILE];
    const int tiles = (A.s.A + ENC_COL_TILE - 1) / ENC_COL_TILE;
    const int lane = threadIdx.x & (ENC_COL_TILE - 1), w = threadIdx.x / ENC_COL_TILE, g = blockIdx.x / tiles;
    const int a = (blockIdx.x - g * tiles) * ENC_COL_TILE + lane;
    const int32_t *sp = A.span + 4 * g;
    const int k = sp[0], f0 = sp[1], L = sp[2] - sp[1];
    EncCol c; c.m = fid_min_zero(); c.absent = 0;
    if (a < A.s.A) {
        const double *__restrict__ eg = A.s.ego_xy + 2 * ((int64_t)k * A.s.T + f0);
        c = enc_column([&](int32_t t, int cc) { return enc_pos_at(A.s, (int64_t)f0 + t, a, cc); },
                       [&](int32_t t, int cc) { return enc_vel_at(A.s, (int64_t)f0 + t, a, cc); },
                       [&](int32_t t, int cc) { return eg[2 * t + cc]; }, w, ENC_STEP_WAVES, L);
    }
    s_c[w][lane] = c;
    __syncthreads();
    if (w != 0 || a >= A.s.A) return;
#pragma unroll
    for (int o = 1; o < ENC_STEP_WAVES; ++o) c = enc_column_join(c, s_c[o][lane]);
    A.col[(int64_t)g * A.s.A + a] = c;
}

// One wave per span: the present columns compacted in ascending order (ballot and prefix count, 64 columns a turn), their
// minima joined with the compacted column as the last key.
__global__ void __launch_bounds__(WAVE)
k_enc_compact(EncSpansArgs A)
{
    const int g = blockIdx.x, lane = threadIdx.x, n_col = A.s.A;
    const EncCol *__restrict__ col = A.col + (int64_t)g * n_col;
    int32_t *__restrict__ cols = A.cols + (int64_t)g * n_col;
    int count = 0;
    EncMin m = enc_min_zero();
    for (int base = 0; base < n_col; base += WAVE) {
        const int a = base + lane;
        const bool present = a < n_col && !col[a].absent;
        const unsigned long long mask = __ballot(present);
        if (present) {
            const int idx = count + __popcll(mask & ((1ull << lane) - 1ull));
            cols[idx] = a;
            m = enc_min_join(m, enc_min_of_column(col[a].m, idx));
        }
        count += __popcll(mask);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        EncMin o;
        o.v = __shfl_xor(m.v, off, WAVE); o.step = __shfl_xor(m.step, off, WAVE); o.col = __shfl_xor(m.col, off, WAVE);
        o.nan = __shfl_xor(m.nan, off, WAVE);
        m = enc_min_join(m, o);
    }
    if (lane != 0) return;
    EncSpanOut r; r.m = m; r.n_ped = count; r.pad_ = 0;
    A.out[g] = r;
}

// Lane = cell of the packed layout, over all kept encounters' cells back to back: the position gathered from the clip
// through the span's column list; with a cruise mode the step's speed, filed per pedestrian over its steps.
__global__ void __launch_bounds__(FID_THREADS)
k_enc_gather(EncRowsArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * FID_THREADS + threadIdx.x;
    if (r >= A.n_cells) return;
    const int e = fid_owner(A.row_off, A.n_kept, r);
    const int64_t local = r - A.row_off[e];
    const int N = A.n_ped[e], L = A.step_off[e + 1] - A.step_off[e];
    const int t = (int)(local / N), n = (int)(local - (int64_t)t * N);
    const int32_t *kp = A.kept + 4 * e;
    const int a = A.cols[(int64_t)kp[2] * A.s.A + n];
    const int64_t f = (int64_t)kp[1] + t;
    const double px = enc_pos_at(A.s, f, a, 0), py = enc_pos_at(A.s, f, a, 1);
    if (A.packed_xy) { A.packed_xy[2 * r] = px; A.packed_xy[2 * r + 1] = py; }
    if (!A.speeds) return;
    const double s = fid_dist(enc_vel_at(A.s, f, a, 0), enc_vel_at(A.s, f, a, 1));
    const int64_t at = A.row_off[e] + (int64_t)n * L + t;
    A.speeds[at] = s;
    if (!A.free_speeds) return;
    const double *__restrict__ eg = A.s.ego_xy + 2 * ((int64_t)kp[0] * A.s.T + f);
    const bool is_free = fid_dist(px - eg[0], py - eg[1]) > A.p.free_distance && s - s == 0.0;
    A.free_speeds[at] = is_free ? s : (double)NAN;
}

// the order statistics pick.lo and pick.hi of the non-NaN entries of v[0 .. L): lanes stride over the entries, each ranks
// its own by counting (ties by index: every rank is taken once), the two hits go through LDS
__device__ __forceinline__ void enc_select(const double *__restrict__ v, int L, const EncPick &pick, double *s_sel, double *s_lo, double *s_hi)
{
    for (int i = threadIdx.x; i < L; i += WAVE) {
        const double x = v[i];
        if (x != x) continue;
        const int32_t r = enc_rank([&](int32_t j) { return v[j]; }, i, L);
        if (r == pick.lo) s_sel[0] = x;
        if (r == pick.hi) s_sel[1] = x;
    }
    __syncthreads();
    *s_lo = s_sel[0]; *s_hi = s_sel[1];
    __syncthreads();
}

// One wave per kept pedestrian: its column, its cruise speed by the launch's mode, its far goal.
__global__ void __launch_bounds__(WAVE)
k_enc_rows(EncRowsArgs A)
{
    __shared__ double s_sel[2];
    const int64_t g = blockIdx.x;
    const int e = fid_owner(A.ped_base, A.n_kept, g);
    const int n = (int)(g - A.ped_base[e]), L = A.step_off[e + 1] - A.step_off[e];
    const int32_t *kp = A.kept + 4 * e;
    const int a = A.cols[(int64_t)kp[2] * A.s.A + n];
    if (threadIdx.x == 0) A.col_out[g] = a;
    if (A.p.cruise_mode == ENC_CRUISE_NONE) return;
    const double *__restrict__ sp = A.speeds + A.row_off[e] + (int64_t)n * L;
    double lo, hi, value = 0.0;
    bool median = A.p.cruise_mode == ENC_CRUISE_MEDIAN;
    if (A.p.cruise_mode == ENC_CRUISE_FREEWALK) {
        const double *__restrict__ fs = A.free_speeds + A.row_off[e] + (int64_t)n * L;
        int n_free = 0;
        for (int i = threadIdx.x; i < L; i += WAVE) n_free += fs[i] == fs[i] ? 1 : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) n_free += __shfl_xor(n_free, off, WAVE);
        if (n_free > 0) {
            const EncPick pick = enc_pick_quantile(n_free, A.p.cruise_q);
            enc_select(fs, L, pick, s_sel, &lo, &hi);
            value = enc_quantile_value(lo, hi, pick.g);
        } else median = true;                                      // never free-walking: the all-step median
    } else if (!median) {
        const EncPick pick = enc_pick_quantile(L, A.p.cruise_q);
        enc_select(sp, L, pick, s_sel, &lo, &hi);
        value = enc_quantile_value(lo, hi, pick.g);
    }
    if (median) {
        enc_select(sp, L, enc_pick_median(L), s_sel, &lo, &hi);
        value = enc_median_value(L, lo, hi);
    }
    if (threadIdx.x != 0) return;
    A.cruise[g] = enc_floor(value);
    const int64_t f0 = kp[1], f1 = f0 + L - 1;
    double gx, gy;
    enc_goal(enc_pos_at(A.s, f0, a, 0), enc_pos_at(A.s, f0, a, 1), enc_pos_at(A.s, f1, a, 0), enc_pos_at(A.s, f1, a, 1),
             enc_vel_at(A.s, f0, a, 0), enc_vel_at(A.s, f0, a, 1), A.p.goal_distance, &gx, &gy);
    A.goals[2 * g] = gx; A.goals[2 * g + 1] = gy;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

#define FOT_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int launch_resample(double sgan_dt, double sim_dt, double staleness, int S, int pred_len, int P, int n_dense,
                    int has_anchor, int prepend, int cv, const void *pred, int pred_dtype, const double *anchor,
                    const double *current, void *out, int out_dtype, int tmajor, hipStream_t st,
                    const int32_t *ped_ep, const int32_t *ep_ped0, const int64_t *ep_blk)
{
    const int total = S * P * 2;
    if (total <= 0) return 0;
    ResampleArgs A;
    A.sgan_dt = sgan_dt; A.sim_dt = sim_dt; A.staleness = staleness;
    A.S = S; A.pred_len = pred_len; A.P = P; A.n_dense = n_dense; A.T = n_dense + (prepend ? 1 : 0);
    A.has_anchor = has_anchor; A.prepend = prepend; A.cv = cv; A.tmajor = tmajor;
    A.ped_ep = ped_ep; A.ep_ped0 = ep_ped0; A.ep_blk = ep_blk;
    if (ped_ep && tmajor) return (int)hipErrorInvalidValue;
    const int bs = 128, grid = (total + bs - 1) / bs;
    if (pred_dtype == FOT_F32 && out_dtype == FOT_F32)
        k_resample<float, float><<<grid, bs, 0, st>>>(A, (const float *)pred, anchor, current, (float *)out);
    else if (pred_dtype == FOT_F32)
        k_resample<float, double><<<grid, bs, 0, st>>>(A, (const float *)pred, anchor, current, (double *)out);
    else if (out_dtype == FOT_F32)
        k_resample<double, float><<<grid, bs, 0, st>>>(A, (const double *)pred, anchor, current, (float *)out);
    else
        k_resample<double, double><<<grid, bs, 0, st>>>(A, (const double *)pred, anchor, current, (double *)out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_resample_slots(double sgan_dt, double sim_dt, double staleness, int S_max, int pred_len, int rows, int n_dense,
                          int n_run, int P_max, const void *pred, int pred_dtype, const double *anchor, const double *current,
                          double *out, const int32_t *ep_ped0, const int64_t *ep_blk, const int32_t *ep_S, hipStream_t st)
{
    if (n_run <= 0 || S_max <= 0 || P_max <= 0 || rows <= 0) return 0;
    if (S_max > FOT_MAX_PLAN_SAMPLES || pred_len < 1 || pred_len > FOT_MAX_PRED_LEN || n_dense < 1 || !ep_ped0 || !ep_blk || !ep_S)
        return (int)hipErrorInvalidValue;
    ResampleSlotsArgs A;
    A.sgan_dt = sgan_dt; A.sim_dt = sim_dt; A.staleness = staleness;
    A.pred_len = pred_len; A.rows = rows; A.n_dense = n_dense;
    A.ep_ped0 = ep_ped0; A.ep_blk = ep_blk; A.ep_S = ep_S;
    const dim3 grid((unsigned)n_run, (unsigned)S_max, (unsigned)((2 * P_max + RSS_THREADS - 1) / RSS_THREADS));
    if (pred_dtype == FOT_F32) k_resample_slots<float><<<grid, RSS_THREADS, 0, st>>>(A, (const float *)pred, anchor, current, out);
    else k_resample_slots<double><<<grid, RSS_THREADS, 0, st>>>(A, (const double *)pred, anchor, current, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_sample_dist(int S, int P, int T, int skip, const void *out, int out_dtype, int tmajor, double *dist,
                       hipStream_t st)
{
    if (S <= 0) return 0;
    if (out_dtype == FOT_F32) k_sample_dist<float><<<S, 256, 0, st>>>(S, P, T, skip, tmajor, (const float *)out, dist);
    else k_sample_dist<double><<<S, 256, 0, st>>>(S, P, T, skip, tmajor, (const double *)out, dist);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_pred_scores(const PredOriginDev *desc, int n, const void *tensor, int dtype, int stride, int E,
                       const double *truth, fot_pred_score *out, hipStream_t st, int wide)
{
    if (n <= 0) return 0;
    if (wide) {
        if (dtype == FOT_F32) k_pred_scores_wide<float><<<n, PS_THREADS, 0, st>>>(desc, (const float *)tensor, stride, E, truth, out);
        else k_pred_scores_wide<double><<<n, PS_THREADS, 0, st>>>(desc, (const double *)tensor, stride, E, truth, out);
    } else if (dtype == FOT_F32) k_pred_scores<float><<<n, PS_THREADS, 0, st>>>(desc, (const float *)tensor, stride, E, truth, out);
    else k_pred_scores<double><<<n, PS_THREADS, 0, st>>>(desc, (const double *)tensor, stride, E, truth, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_safety(const DevParams *P, int n, const double *ego, const int32_t *ped_off, const double *ped_pos,
                  const double *ped_vel, double ego_radius, double ped_radius, double footprint_radius, int use_fp,
                  fot_safety *out, hipStream_t st, const int32_t *ep_scen, const SafetyScen *scen_tab)
{
    if (n <= 0) return 0;
    if (!scen_tab) ep_scen = nullptr;
    k_safety<<<n, WAVE, 0, st>>>(P, n, ego, ped_off, ped_pos, ped_vel, ego_radius, ped_radius, footprint_radius, use_fp, out,
                                 ep_scen, scen_tab);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_static_gather(const StaticGather *tab, int n_req, const double *points, double *out, hipStream_t st)
{
    if (n_req <= 0) return 0;
    k_static_gather<<<n_req, 256, 0, st>>>(tab, n_req, (const double2 *)points, (double2 *)out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_frame(ReplayView rv, FrameStage in, FrameDev out, int n_run, int f_cur, int f_last, int f_prev,
                      hipStream_t st)
{
    if (n_run <= 0) return 0;
    k_loop_frame<<<n_run, WAVE, 0, st>>>(rv, in, out, n_run, f_cur, f_last, f_prev);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_sample_rows(const LoopSampleRows &a, hipStream_t st)
{
    const int64_t total = sr_step_elems(a.d);
    if (total <= 0) return 0;
    const unsigned grid = (unsigned)((total + SR_THREADS - 1) / SR_THREADS);
    if (a.dtype == FOT_F32) k_loop_sample_rows<float2><<<grid, SR_THREADS, 0, st>>>(a);
    else k_loop_sample_rows<double2><<<grid, SR_THREADS, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_sample_rows_prefix(const LoopSampleRows &a, int S_src, hipStream_t st)
{
    const int64_t total = sr_step_elems(a.d);
    if (total <= 0) return 0;
    if (a.d.S > S_src) return (int)hipErrorInvalidValue;             // (the step moves a prefix of the source's samples)
    const unsigned grid = (unsigned)((total + SR_THREADS - 1) / SR_THREADS);
    if (a.dtype == FOT_F32) k_loop_sample_rows_prefix<float2><<<grid, SR_THREADS, 0, st>>>(a, S_src);
    else k_loop_sample_rows_prefix<double2><<<grid, SR_THREADS, 0, st>>>(a, S_src);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_model_rows(const LoopModelRows &a, hipStream_t st)
{
    const int64_t total = (int64_t)a.S * a.pred_len * a.rows;
    if (total <= 0) return 0;
    k_loop_model_rows<<<(unsigned)((total + SR_THREADS - 1) / SR_THREADS), SR_THREADS, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_predict_cv_frame(double sgan_dt, double sim_dt, double staleness, int n_rows, int n_dense, FrameDev f,
                            double *out, hipStream_t st)
{
    if (n_rows <= 0) return 0;
    const int bs = 128, grid = (2 * n_rows + bs - 1) / bs;
    k_predict_cv_frame<<<grid, bs, 0, st>>>(sgan_dt, sim_dt, staleness, n_rows, n_dense, f, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_digest(const fot_result *rec, int n, LoopDigest *out, int32_t *done, int32_t seq, hipStream_t st)
{
    k_loop_digest<<<1, 256, 0, st>>>(rec, n > 0 ? n : 0, out, done, seq);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_history(const fot_result *rec, int n_run, const int32_t *src, const int32_t *slot, double *hist,
                        int n_slots, int n_total, int32_t *done, int32_t seq, hipStream_t st)
{
    const int grid = hist && n_run > 0 ? n_run : 1;
    k_loop_history<<<grid, 256, 0, st>>>(rec, n_run, src, slot, hist, n_slots, n_total, done, seq);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_pred_error(ReplayView rv, const int32_t *slot_of, FrameDev f, const double *dyn, int n_run, int have_pred,
                           int f_cur, int step, SummaryShape S, double *ring, int32_t *ring_P, SummaryTotals *totals,
                           hipStream_t st, const int32_t *best)
{
    if (n_run <= 0) return 0;
    if (S.n_dense < 1 || S.n_dense > FOT_MAX_NT || step < 0) return (int)hipErrorInvalidValue;
    k_loop_pred_error<<<n_run, 256, 0, st>>>(rv, slot_of, f, dyn, n_run, have_pred, f_cur, step, S, ring, ring_P, totals, best);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_best_sample(const int32_t *slot_of, FrameDev f, const double *dyn, int n_run, int S, int n_dense,
                            double *dev_tab, int32_t *best_tab, int32_t *best_host, hipStream_t st)
{
    if (n_run <= 0) return 0;
    if (S < 1 || S > FOT_MAX_PLAN_SAMPLES || n_dense < 1) return (int)hipErrorInvalidValue;
    if (S > FOT_MAX_SAMPLES)
        k_loop_best_sample_wide<<<n_run, BS_THREADS, 0, st>>>(slot_of, f, dyn, n_run, S, n_dense, dev_tab, best_dev_stride(S),
                                                              best_tab, best_host);
    else
        k_loop_best_sample<<<n_run, BS_THREADS, 0, st>>>(slot_of, f, dyn, n_run, S, n_dense, dev_tab, best_tab, best_host);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_best_sample_sweep(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab, int n_run, int S,
                                  int n_dense, double *dev_tab, int32_t *best_tab, int32_t *best_host, hipStream_t st)
{
    if (n_run <= 0) return 0;
    if (S < 1 || S > FOT_MAX_PLAN_SAMPLES || n_dense < 1 || !tab) return (int)hipErrorInvalidValue;
    if (S > FOT_MAX_SAMPLES)
        k_loop_best_sample_sweep_wide<<<n_run, BS_THREADS, 0, st>>>(slot_of, f, dyn, tab, n_run, S, n_dense, dev_tab,
                                                                    best_dev_stride(S), best_tab, best_host);
    else
        k_loop_best_sample_sweep<<<n_run, BS_THREADS, 0, st>>>(slot_of, f, dyn, tab, n_run, S, n_dense, dev_tab, best_tab, best_host);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_rep_block_sweep(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab,
                                const int32_t *best_tab, int n_run, int S, int n_dense, double *tensor, int32_t *pre_dev,
                                int32_t *pre_host, hipStream_t st)
{
    if (n_run <= 0) return 0;
    if (S < 1 || S > FOT_MAX_PLAN_SAMPLES || n_dense < 1 || !tab) return (int)hipErrorInvalidValue;
    k_loop_rep_block_sweep<<<n_run, RB_THREADS, 0, st>>>(slot_of, f, dyn, tab, best_tab, n_run, S, n_dense, tensor, pre_dev, pre_host);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_best_sample_slots(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab, const int32_t *ep_S,
                                  int n_run, int S_max, int n_dense, double *dev_tab, int dev_stride, int32_t *best_tab,
                                  int32_t *best_host, hipStream_t st)
{
    if (n_run <= 0) return 0;
    if (S_max < 1 || S_max > FOT_MAX_PLAN_SAMPLES || dev_stride < S_max || n_dense < 1 || !tab || !ep_S) return (int)hipErrorInvalidValue;
    if (S_max > FOT_MAX_SAMPLES)
        k_loop_best_sample_slots_wide<<<n_run, BS_THREADS, 0, st>>>(slot_of, f, dyn, tab, ep_S, n_run, n_dense, dev_tab, dev_stride,
                                                                    best_tab, best_host);
    else
        k_loop_best_sample_slots<<<n_run, BS_THREADS, 0, st>>>(slot_of, f, dyn, tab, ep_S, n_run, n_dense, dev_tab, dev_stride,
                                                               best_tab, best_host);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_rep_block_slots(const int32_t *slot_of, FrameDev f, const double *dyn, const SweepEp *tab, const int32_t *ep_S,
                                const int32_t *best_tab, int n_run, int n_dense, double *tensor, int32_t *pre_dev,
                                int32_t *pre_host, hipStream_t st)
{
    if (n_run <= 0) return 0;
    if (n_dense < 1 || !tab || !ep_S) return (int)hipErrorInvalidValue;
    k_loop_rep_block_slots<<<n_run, RB_THREADS, 0, st>>>(slot_of, f, dyn, tab, ep_S, best_tab, n_run, n_dense, tensor, pre_dev, pre_host);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_rep_block(const int32_t *slot_of, FrameDev f, const double *dyn, const int32_t *best_tab, int n_run, int S,
                          int n_dense, double *rep, int32_t *pre_dev, int32_t *pre_host, hipStream_t st)
{
    if (n_run <= 0) return 0;
    if (S < 1 || S > FOT_MAX_PLAN_SAMPLES || n_dense < 1) return (int)hipErrorInvalidValue;
    k_loop_rep_block<<<n_run, RB_THREADS, 0, st>>>(slot_of, f, dyn, best_tab, n_run, S, n_dense, rep, pre_dev, pre_host);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_score_truth(ReplayView rv, const int32_t *slot_of, FrameDev f, int n_rows, int f_cur, int stride, int E,
                            double *out, hipStream_t st)
{
    if (n_rows <= 0) return 0;
    if (stride < 1 || E < 1 || E > FOT_MAX_PRED_LEN) return (int)hipErrorInvalidValue;
    const int n = n_rows * E;
    k_loop_score_truth<<<(n + 255) / 256, 256, 0, st>>>(rv, slot_of, f, n_rows, f_cur, stride, E, (double2 *)out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_openloop_rows(const OpenLoopRows &a, hipStream_t st)
{
    if (a.rows <= 0) return 0;
    if (a.obs_len < 1 || a.pred_len < 1 || a.pred_len > FOT_MAX_PRED_LEN || a.n_cols < 1 || !a.scene || !a.row_col ||
        !a.row_f0 || !a.obs || !a.anchor || !a.truth)
        return (int)hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.rows + OL_TILE_ROWS - 1) / OL_TILE_ROWS);
    if (a.dtype == FOT_F32) k_openloop_rows<float2><<<grid, OL_THREADS, 0, st>>>(a);
    else k_openloop_rows<double2><<<grid, OL_THREADS, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_loop_summary(SummaryShape S, const double *ring, const int32_t *ring_P, const SummaryTotals *totals,
                        const int32_t *steps, int n_slots, int num_samples, fot_loop_summary *out, hipStream_t st)
{
    if (n_slots <= 0) return 0;
    if (S.n_dense < 1 || S.n_dense > FOT_MAX_NT) return (int)hipErrorInvalidValue;
    k_loop_summary<<<n_slots, 256, 0, st>>>(S, ring, ring_P, totals, steps, n_slots, num_samples, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_footprint_steps(const FpoGeom *geom, int n, const double *xy, int xy_stride, const double *yaw, int yaw_stride,
                           const int32_t *ped_off, const double *ped_xy, FpoStep *out, hipStream_t st)
{
    if (n <= 0) return 0;
    if (!geom || !xy || !yaw || !ped_off || !out || xy_stride < 2 || yaw_stride < 1) return (int)hipErrorInvalidValue;
    k_footprint_steps<<<n, WAVE, 0, st>>>(geom, n, xy, xy_stride, yaw, yaw_stride, ped_off, ped_xy, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_footprint_yaw(int n_traj, const int32_t *step_off, const double *xy, double *yaw_out, hipStream_t st)
{
    if (n_traj <= 0) return 0;
    if (!step_off || !xy || !yaw_out) return (int)hipErrorInvalidValue;
    k_footprint_yaw<<<n_traj, FPO_THREADS, 0, st>>>(step_off, xy, yaw_out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_footprint_fold(const FpoGeom *geom, int n_traj, const int32_t *step_off, const int32_t *ped_off,
                          const FpoStep *series, FpoRecord *out, hipStream_t st)
{
    if (n_traj <= 0) return 0;
    if (!geom || !step_off || !ped_off || !series || !out) return (int)hipErrorInvalidValue;
    k_footprint_fold<<<n_traj, FPO_THREADS, 0, st>>>(geom, step_off, ped_off, series, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_fidelity(const FidelityArgs &a, hipStream_t st)
{
    if (a.n_enc <= 0) return 0;
    if (!a.step_off || !a.n_ped || !a.dt || !a.row_off || !a.ped_base || !a.ego || !a.series || !a.out || a.n_steps <= 0 ||
        a.n_peds < 0) return (int)hipErrorInvalidValue;
    if (a.n_peds > 0 && (!a.ped_xy || !a.onset_dist || !a.onset_step || (a.truth && (!a.ped_sum || !a.ped_keep))))
        return (int)hipErrorInvalidValue;
    const int64_t ped_blocks = (a.n_peds + FID_THREADS - 1) / FID_THREADS, step_blocks = (a.n_steps + FID_THREADS - 1) / FID_THREADS;
    if (ped_blocks > 0x7fffffffLL || step_blocks > 0x7fffffffLL) return (int)hipErrorInvalidConfiguration;
    if (ped_blocks > 0) {
        k_fidelity_peds<<<(unsigned)ped_blocks, FID_THREADS, 0, st>>>(a);
        FOT_LAUNCH_CHECK();
    }
    k_fidelity_series<<<(unsigned)step_blocks, FID_THREADS, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    k_fidelity_fold<<<a.n_enc, WAVE, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_enc_spans(const EncSpansArgs &a, hipStream_t st)
{
    if (a.n_go <= 0) return 0;
    if (!a.s.ped_xy || !a.s.ego_xy || !a.span || !a.col || !a.cols || !a.out || a.s.T < 1 || a.s.A < 1) return (int)hipErrorInvalidValue;
    const int64_t blocks = (int64_t)a.n_go * ((a.s.A + ENC_COL_TILE - 1) / ENC_COL_TILE);
    if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidConfiguration;
    k_enc_columns<<<(unsigned)blocks, ENC_COL_TILE * ENC_STEP_WAVES, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    k_enc_compact<<<a.n_go, WAVE, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_enc_rows(const EncRowsArgs &a, hipStream_t st)
{
    if (a.n_kept <= 0) return 0;
    if (!a.s.ped_xy || !a.s.ego_xy || !a.kept || !a.step_off || !a.n_ped || !a.row_off || !a.ped_base || !a.cols || !a.col_out ||
        a.n_rows < 1 || a.n_cells < 1) return (int)hipErrorInvalidValue;
    const bool cruise = a.p.cruise_mode != ENC_CRUISE_NONE;
    if (cruise && (!a.speeds || !a.cruise || !a.goals || (a.p.cruise_mode == ENC_CRUISE_FREEWALK && !a.free_speeds)))
        return (int)hipErrorInvalidValue;
    const int64_t cell_blocks = (a.n_cells + FID_THREADS - 1) / FID_THREADS;
    if (cell_blocks > 0x7fffffffLL || a.n_rows > 0x7fffffffLL) return (int)hipErrorInvalidConfiguration;
    if (a.packed_xy || a.speeds) {
        k_enc_gather<<<(unsigned)cell_blocks, FID_THREADS, 0, st>>>(a);
        FOT_LAUNCH_CHECK();
    }
    k_enc_rows<<<(unsigned)a.n_rows, WAVE, 0, st>>>(a);
    FOT_LAUNCH_CHECK();
    return 0;
}

}  // namespace fot
