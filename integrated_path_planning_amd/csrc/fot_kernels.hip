// fot_kernels.hip -- gfx950 kernels of the Frenet optimal-trajectory planner.
//
// Pipeline of one fot_plan_batch (one launch each over the whole batch; every decision in float64):
//   k_frenet_state : 4 waves / instance: pulls the instance's descriptor out of the pinned staging block, nearest point
//                    (sample scan over the workgroup, three refinement rounds per evaluation) + Cartesian->Frenet;
//                    behind the last scan ONE wave goes on (refinement, state, group headers), the other three end
//   k_cull         : 8 waves / (instance, 8 consecutive time steps): derives and merges the boxes of the instance's
//                    longitudinal profiles, sorts the obstacles of those time rows that lie inside the grown boxes
//                    into per-step entry lists (strips, LDS atomics), writes each candidate wave's chunk range
//   k_evaluate     : 1 wave / TILE (up to 64 consecutive candidates of one instance, at most three full-length
//                    profiles), 1 lane / candidate, tiles dealt out longest first: the wave builds the rows of its
//                    tile's profiles in its own slice of LDS, then: quintic, Frenet->Cartesian, cost,
//                    truncation, kinematic checks, and -- while the candidate can still pass -- the collision test of
//                    each sample against the entry list of its time step (wave-uniform chunk walk on scalar loads,
//                    float32 bounds, float64 only between them).  Candidate points never leave registers.
//   (selection)    : the wave that finishes an instance's last tile: stop-distance filter, rejection histogram,
//                    first-minimum argmin (lowest index wins ties), selected path rebuilt from its profile and written
//                    out -- inside the evaluation launch (select_instance_wave)
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "fot_math.hpp"
#include "fot_kernels.h"

namespace fot {

// ---------------------------------------------------------------------------
// wave-level reductions on the DPP data path (no LDS traffic)
// ---------------------------------------------------------------------------

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float v)
{
    // lanes without a valid source (or masked rows) keep their own value
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}

// butterfly inside quads / half rows / rows, then row_bcast15 and row_bcast31: lane 63 ends with the reduction
#define FOT_WAVE_REDUCE_F32(NAME, OP)                                                        \
    __device__ __forceinline__ float NAME(float v)                                           \
    {                                                                                        \
        v = OP(v, dpp_f32<0xB1, 0xf>(v));  /* quad_perm [1,0,3,2] */                         \
        v = OP(v, dpp_f32<0x4E, 0xf>(v));  /* quad_perm [2,3,0,1] */                         \
        v = OP(v, dpp_f32<0x141, 0xf>(v)); /* row_half_mirror */                             \
        v = OP(v, dpp_f32<0x140, 0xf>(v)); /* row_mirror */                                  \
        v = OP(v, dpp_f32<0x142, 0xa>(v)); /* row_bcast15 -> rows 1, 3 */                    \
        v = OP(v, dpp_f32<0x143, 0xc>(v)); /* row_bcast31 -> rows 2, 3 */                    \
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));             \
    }
FOT_WAVE_REDUCE_F32(wave_min_f32, fminf)
FOT_WAVE_REDUCE_F32(wave_max_f32, fmaxf)

// The same reductions for values that are never NaN (k_cull's boxes: finite or +-inf), one instruction a step.  From the
// source form above the compiler makes four a step: fminf's operands are canonicalised first, which keeps the DPP
// read out of the min itself.  v_min_f32 / v_max_f32 order -0 below +0 and return an operand unchanged, as fminf and
// fmaxf compile here, so the results are the same bits.  The statement pads its own hazards (a VALU result read through DPP: two
// wait states); rows a step masks and lanes without a source are not written, i.e. keep their value, as above.
#define FOT_WAVE_REDUCE_F32_ASM(NAME, OP)                                                    \
    __device__ __forceinline__ float NAME(float v)                                           \
    {                                                                                        \
        asm("s_nop 1\n\t"                                                                    \
            OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"   \
            OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"   \
            OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"       \
            OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"            \
            OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"          \
            OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"              \
            : "+v"(v));                                                                      \
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));             \
    }
FOT_WAVE_REDUCE_F32_ASM(wave_min_nonan_f32, "v_min_f32_dpp")
FOT_WAVE_REDUCE_F32_ASM(wave_max_nonan_f32, "v_max_f32_dpp")

// inclusive prefix sum over the wave's lanes on the DPP data path: shifts inside the rows of 16, then the last lane of
// a row to the rows behind it (row_bcast15 -> rows 1 and 3, row_bcast31 -> rows 2 and 3); a lane without a source adds 0
__device__ __forceinline__ int wave_prefix_sum_i32(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast31
    return v;
}

// minimum over the wave's lanes (every lane active), as a scalar: the shifts and broadcasts of the prefix sum, lane 63
// ends with the reduction; a lane without a source keeps its own value
__device__ __forceinline__ int wave_min_i32(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));   // row_bcast15
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));   // row_bcast31
    return __builtin_amdgcn_readlane(v, 63);
}

// ---------------------------------------------------------------------------
// ego -> Frenet state
// ---------------------------------------------------------------------------

__device__ __forceinline__ ScanBest wave_argmin(ScanBest b)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ScanBest o;
        o.dist = __shfl_xor(b.dist, off, WAVE);
        o.idx = __shfl_xor(b.idx, off, WAVE);
        scan_merge(b, o);
    }
    return b;
}

// Entry i of a read-only table in HBM (the scenarios' SplineView table) read through the constant address space: a
// scalar load even where the kernel also stores to global memory, instead of vector loads that hold the entry's 80
// bytes in VGPRs until they are read back to scalars.
template <typename T>
__device__ __forceinline__ T load_const(const T *table, int i)
{
    static_assert(sizeof(T) % sizeof(uint64_t) == 0, "copied in 8-byte words");
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint64_t const_u64;
    const_u64 *src = (const_u64 *)(table + i);
    T v;
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / sizeof(uint64_t)); ++k) ((uint64_t *)&v)[k] = src[k];
    return v;
#else
    return table[i];
#endif
}

// The reference spline (9 coefficient arrays of n knots) copied into LDS: the nearest-point search and the segment
// lookups are chains of dependent reads of these arrays, each an L2 round trip otherwise.  Paths with more knots than
// the launch reserved LDS for (lds_knots) stay in HBM.  Dynamic LDS: 9 * lds_knots doubles.
extern __shared__ double s_spl[];
constexpr int SPLINE_LDS_KNOTS = 512;

// (in two steps, for a caller that has more to put behind the same barrier: the copy, and the view of the copied path)
__device__ __forceinline__ void stage_spline_copy(const SplineView &g, double *s_spl)
{
    const double *src[9] = { g.s, g.ax, g.bx, g.cx, g.dx, g.ay, g.by, g.cy, g.dy };
    for (int i = threadIdx.x; i < 9 * g.n; i += blockDim.x) {
        const int a = i / g.n, j = i - a * g.n;
        s_spl[i] = src[a][j];
    }
}

__device__ __forceinline__ SplineView staged_spline_view(const SplineView &g, double *s_spl)
{
    SplineView l = g;
    l.s = s_spl; l.ax = s_spl + g.n; l.bx = s_spl + 2 * g.n; l.cx = s_spl + 3 * g.n; l.dx = s_spl + 4 * g.n;
    l.ay = s_spl + 5 * g.n; l.by = s_spl + 6 * g.n; l.cy = s_spl + 7 * g.n; l.dy = s_spl + 8 * g.n;
    return l;
}

__device__ __forceinline__ SplineView stage_spline(const SplineView &g, int lds_knots, double *s_spl = fot::s_spl)
{
    if (g.n > lds_knots) return g;
    stage_spline_copy(g, s_spl);
    __syncthreads();
    return staged_spline_view(g, s_spl);
}

// refine_nearest (fot_math.hpp), three rounds per evaluation.  A round compares the distances at s - ds, s, s + ds and
// either moves left, moves right or halves ds; the next round's probes depend on that outcome.  39 lanes evaluate, in
// one go, the probes of round r (3 lanes), of round r+1 under each of the 3 outcomes of r (9 lanes) and of round r+2
// under each of the 9 outcome pairs (27 lanes); the rounds are then resolved from the shuffled distances.  Every lane
// derives its (s, ds) with the very expressions of the sequential loop, so the result is bit-identical to it -- a
// third of the dependent spline evaluations.  Uniform across the wave.
__device__ __forceinline__ void refine_apply(int outcome, double s_end, double &s, double &ds)
{
    if (outcome == 0) s = fmax(0.0, s - ds);                      // left probe won
    else if (outcome == 1) s = fmin(s_end, s + ds);               // right probe won
    else ds *= 0.5;                                               // centre: halve the step
}

__device__ __forceinline__ double refine_nearest_wave(const SplineView &sp, double x, double y, double best_s, int lane)
{
    const double s_end = sp.s[sp.n - 1];
    // role of this lane: depth 0 (lanes 0-2), depth 1 (3-11: outcome o1), depth 2 (12-38: outcomes o1, o2)
    int depth = 0, o1 = 0, o2 = 0, pos = lane;
    if (lane >= 12) { const int i = lane - 12; depth = 2; o1 = i / 9; o2 = (i / 3) % 3; pos = i % 3; }
    else if (lane >= 3) { const int i = lane - 3; depth = 1; o1 = i / 3; pos = i % 3; }
    if (lane >= 39) { depth = 0; pos = 1; }                       // idle lanes probe the centre (values unused)
    double ds = 0.2;
    for (int it = 0; it < 20; it += 3) {
        double ms = best_s, mds = ds;
        if (depth >= 1) refine_apply(o1, s_end, ms, mds);
        if (depth >= 2) refine_apply(o2, s_end, ms, mds);
        const double probe = pos == 0 ? fmax(0.0, ms - mds) : (pos == 1 ? ms : fmin(s_end, ms + mds));
        double px, py;
        spline_xy(sp, probe, px, py);
        const double dist = hypot_cr(x - px, y - py);
        const int rounds = 20 - it < 3 ? 20 - it : 3;
        int base = 0, r1 = 0;
        for (int r = 0; r < rounds; ++r) {
            const double dist_left = __shfl(dist, base, WAVE), dist_curr = __shfl(dist, base + 1, WAVE),
                         dist_right = __shfl(dist, base + 2, WAVE);
            int o = 2;
            if (dist_left < dist_curr && dist_left < dist_right) o = 0;
            else if (dist_right < dist_curr && dist_right < dist_left) o = 1;
            refine_apply(o, s_end, best_s, ds);
            if (r == 0) { r1 = o; base = 3 + 3 * o; } else base = 12 + 9 * r1 + 3 * o;
        }
    }
    return best_s;
}

constexpr int FRENET_WG = 256;

// NanScan (fot_kernels.h): block `part` of `parts` of instance D flags the tracks [j0, j1) it owns.  A track is a
// (sample, pedestrian) pair, T points; the flags of the block's own tracks are cleared, then every NaN coordinate sets
// its track's flag (plain byte stores of the same value: no ordering between them is needed).
template <typename T>
__device__ __forceinline__ void scan_nan_tracks(const InstDesc &D, const T *__restrict__ dyn_xy, uint8_t *__restrict__ flag,
                                                int part, int parts, T *__restrict__ stage)
{
    if (D.dyn_mode == FOT_DYN_NONE) return;
    const int n_tracks = D.S * D.P;
    const int per = (n_tracks + parts - 1) / parts;
    const int j0 = part * per, j1 = j0 + per < n_tracks ? j0 + per : n_tracks;
    if (j0 >= j1) return;
    uint8_t *f = flag + D.nan_off;
    for (int j = j0 + (int)threadIdx.x; j < j1; j += FRENET_WG) f[j] = 0;
    __syncthreads();
    struct Pt { T x, y; };
    const Pt *base = (const Pt *)dyn_xy + D.dyn_off;
    Pt *out = stage ? (Pt *)stage + D.dyn_off : nullptr;          // (NanScan::stage: what is read is also copied into HBM)
    if (D.dyn_tmajor) {                                          // [T][S][P]: thread = track, rows n_tracks apart
        constexpr int TU = 8;                                     // rows in flight per thread (neighbouring threads read
        for (int j = j0 + (int)threadIdx.x; j < j1; j += FRENET_WG) {   // neighbouring points of a row)
            bool bad = false;
            for (int t0 = 0; t0 < D.T; t0 += TU) {
                Pt p[TU];
#pragma unroll
                for (int u = 0; u < TU; ++u) p[u] = base[(int64_t)(t0 + u < D.T ? t0 + u : D.T - 1) * n_tracks + j];
#pragma unroll
                for (int u = 0; u < TU; ++u) bad |= (p[u].x != p[u].x) | (p[u].y != p[u].y);
                if (out) {
#pragma unroll
                    for (int u = 0; u < TU; ++u) if (t0 + u < D.T) out[(int64_t)(t0 + u) * n_tracks + j] = p[u];
                }
            }
            if (bad) f[j] = 1;
        }
    } else {                                                     // [S][P][T]: the block's tracks are one contiguous run
        // 16-byte loads, sixteen in flight per thread (64 KB per block and round): the run is read once, at memory speed,
        // while the nearest-point blocks of the same launch wait on their chains of dependent spline evaluations
        typedef T V __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int PER = (int)(16 / sizeof(T)) / 2;            // points per load: 2 (float) or 1 (double)
        constexpr int UNROLL = 16;
        const int64_t i0 = (int64_t)j0 * D.T, i1 = (int64_t)j1 * D.T;            // points [i0, i1)
        // head: points in front of the first 16-byte boundary (at most one, float only)
        int64_t a0 = i0;
        if (PER == 2 && ((uintptr_t)(base + i0) & 15)) {             // (global loads need dword alignment only; speed)
            if (threadIdx.x == 0) {
                const Pt p = base[i0];
                if ((p.x != p.x) | (p.y != p.y)) f[(int)(i0 / D.T)] = 1;
                if (out) out[i0] = p;
            }
            a0 = i0 + 1;
        }
        const int64_t n_vec = (i1 - a0) / PER;
        const V *vb = (const V *)(base + a0);
        V *vo = out ? (V *)(out + a0) : nullptr;
        for (int64_t vbase = threadIdx.x; vbase < n_vec; vbase += (int64_t)UNROLL * FRENET_WG) {
            V v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int64_t vi = vbase + (int64_t)u * FRENET_WG;
                v[u] = vb[vi < n_vec ? vi : n_vec - 1];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int64_t vi = vbase + (int64_t)u * FRENET_WG;
                if (vi >= n_vec) continue;
                if (vo) vo[vi] = v[u];
                bool b0 = (v[u][0] != v[u][0]) | (v[u][1] != v[u][1]);
                if (PER == 2) {
                    const bool b1 = (v[u][2 % (2 * PER)] != v[u][2 % (2 * PER)]) | (v[u][3 % (2 * PER)] != v[u][3 % (2 * PER)]);
                    if (b1) f[(int)((a0 + vi * PER + 1) / D.T)] = 1;
                }
                if (b0) f[(int)((a0 + vi * PER) / D.T)] = 1;
            }
        }
        // tail: the last point when an odd number is left (float only)
        if (PER == 2 && threadIdx.x == 0 && a0 + n_vec * PER < i1) {
            const Pt p = base[i1 - 1];
            if ((p.x != p.x) | (p.y != p.y)) f[(int)((i1 - 1) / D.T)] = 1;
            if (out) out[i1 - 1] = p;
        }
    }
}

// A condition every lane of the wave holds alike, as a scalar: the branch on it is a jump, not a lane mask (a wave that
// leaves under it is gone as a whole)
__device__ __forceinline__ bool wave_uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

// The wave ends HERE, inside whatever loop or branch: a `return` out of a loop the compiler holds for divergent only
// clears the lanes' bits and walks on to the loop's exit.  Kernel-level code only (nothing to unwind on the device).
__device__ __forceinline__ void end_wave()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_endpgm();
#endif
}

// arg-min of a sample scan over the whole workgroup (lowest index wins ties); every thread gets the result
__device__ __forceinline__ ScanBest block_argmin(ScanBest b, ScanBest *s_best)
{
    b = wave_argmin(b);
    __syncthreads();                                              // s_best free again
    if ((threadIdx.x & (WAVE - 1)) == 0) s_best[threadIdx.x / WAVE] = b;
    __syncthreads();
    ScanBest r = s_best[0];
    for (int w = 1; w < FRENET_WG / WAVE; ++w) scan_merge(r, s_best[w]);
    return r;
}

// One workgroup (4 waves) per instance: the sample scans are spread over all threads; the refinement, the Frenet state
// and the tail are uniform values, which wave 0 ALONE computes for an instance that heads no chain: waves 1 - 3 end
// behind the last block-wide scan of the search (a terminated wave gives its registers back to the evaluation waves of
// the calls in flight beside it; the workgroup's LDS, the staged path included, stays until wave 0 ends), and no
// barrier is reachable for such a block from there on.  The head of a chain keeps its four waves throughout (a barrier
// and a scan per member), as does every block under all_waves (FOT_FRENET_WAVES=all: tests, A/B runs).  `block` is the
// workgroup's role: an instance, or (behind the instances) one part of the NaN scan of an instance's tensor.  `sp`: the
// reference path, staged by the caller.
__device__ __forceinline__ void frenet_state_block(const DevParams *__restrict__ Pp, const SplineView &sp, const InstDesc *desc,
                                                   InstState *__restrict__ state, int n_inst, const MetaImport &imp,
                                                   const NanScan &scan, int32_t *__restrict__ inst_done, int block,
                                                   const GroupHeadOut &gh, int all_waves)
{
    __shared__ ScanBest s_best[FRENET_WG / WAVE];
    __shared__ InstDesc s_desc;                                   // the descriptor being worked on, read once
    int inst = block;
    if (inst >= n_inst) {
        // the blocks behind the nearest-point blocks: NaN scan of the dynamic tensors (memory-bound, on CUs whose
        // nearest-point block is a chain of dependent spline evaluations)
        const int b = inst - n_inst, si = b / scan.blocks_per_inst, part = b - si * scan.blocks_per_inst;
        if (si >= n_inst) return;
        const InstDesc &D = (imp.h_desc ? imp.h_desc : desc)[si];
        if (!D.dyn_tmajor && !scan.stage && !scan.eager) return;                // ([S][P][T] tensors in HBM: k_cull looks for NaNs itself)
        if (scan.dtype == FOT_F32)
            scan_nan_tracks(D, (const float *)scan.dyn_xy, scan.flag, part, scan.blocks_per_inst, (float *)scan.stage);
        else
            scan_nan_tracks(D, (const double *)scan.dyn_xy, scan.flag, part, scan.blocks_per_inst, (double *)scan.stage);
        return;
    }
    constexpr int DESC_WORDS = (int)(sizeof(InstDesc) / sizeof(unsigned long long));
    static_assert(sizeof(InstDesc) % sizeof(unsigned long long) == 0, "InstDesc is copied in 8-byte words");
    if (imp.h_desc) {
        // First kernel of a plan call: the descriptors still sit in the caller-side pinned staging block.  Every
        // workgroup moves its own instance's descriptor into HBM for the kernels that follow
        // (instead of a separate H2D copy in front of the launch sequence) and works from the staging copy itself.
        desc = imp.h_desc;
        const unsigned long long *src = (const unsigned long long *)&desc[inst];
        if (threadIdx.x < DESC_WORDS) {
            const unsigned long long v = src[threadIdx.x];
            ((unsigned long long *)&imp.d_desc[inst])[threadIdx.x] = v;
            ((unsigned long long *)&s_desc)[threadIdx.x] = v;
        }
        __syncthreads();
    } else {
        if (threadIdx.x < DESC_WORDS)
            ((unsigned long long *)&s_desc)[threadIdx.x] = ((const unsigned long long *)&desc[inst])[threadIdx.x];
        __syncthreads();
    }
    if (s_desc.ego.has_prev_s == FOT_PREV_S_CHAINED) return;      // handled by the head of its chain
    const DevParams &P = *Pp;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const double s_end = sp.s[sp.n - 1];
    const int n_glob = global_search_count(sp);
    double carry_prev_s = 0.0;                                 // new_prev_s of the previous member of the chain
    bool chained = false;
    const int n_members = 1 + __builtin_amdgcn_readfirstlane(s_desc.n_chained);   // (a scalar: the loop is no lane mask)
    // one wave behind the search (the wave's number as a scalar: a jump decides who leaves, not a lane mask)
    const bool solo = n_members == 1 && !all_waves;
    const bool leaves = solo && __builtin_amdgcn_readfirstlane(tid / WAVE) != 0;
    const int n_thr = solo ? WAVE : FRENET_WG;                  // threads behind the search (solo: tid < WAVE there)
    for (int m = 0; m < n_members; ++m, ++inst) {
        if (m > 0) {                                           // next member of the chain: its descriptor
            __syncthreads();
            if (threadIdx.x < DESC_WORDS)
                ((unsigned long long *)&s_desc)[threadIdx.x] = ((const unsigned long long *)&desc[inst])[threadIdx.x];
            __syncthreads();
        }
        const InstDesc &D = s_desc;
        const double x = D.ego.x, y = D.ego.y;
        // (the branches of the search on scalars: what the waves that leave it jump on must not hang on a lane mask)
        const int ego_form = __builtin_amdgcn_readfirstlane(D.ego.has_prev_s);
        const bool has_prev = chained ? true : ego_form != 0;
        const double prev_s = chained ? carry_prev_s : D.ego.prev_s;

        double best_s = 0.0;
        bool need_global = true;
        const bool given = ego_form == FOT_EGO_IS_FRENET;          // the Frenet state itself: nothing to search
        if (given) need_global = false;
        if (leaves && given) end_wave();
        if (has_prev && !given) {                              // cached window +-10 m, 100 samples
            const double s_min = fmax(0.0, prev_s - 10.0);
            const double s_max = fmin(s_end, prev_s + 10.0);
            ScanBest b = block_argmin(scan_samples(sp, x, y, s_min, s_max, 100, tid, FRENET_WG, false), s_best);
            best_s = b.idx >= 0 ? linspace_at(s_min, s_max, 100, b.idx) : 0.0;
            const bool at_lower = fabs(best_s - s_min) < 1e-3 && s_min > 0.0;
            const bool at_upper = fabs(best_s - s_max) < 1e-3 && s_max < s_end;
            need_global = wave_uniform(at_lower || at_upper);
            if (leaves && !need_global) end_wave();
        }
        if (need_global) {
            ScanBest b = block_argmin(scan_samples(sp, x, y, 0.0, s_end, n_glob, tid, FRENET_WG, true), s_best);
            if (leaves) end_wave();
            best_s = linspace_at(0.0, s_end, n_glob, b.idx >= 0 ? b.idx : 0);
        }
        if (!given) best_s = refine_nearest_wave(sp, x, y, best_s, lane);
        const double new_prev_s = given ? NAN : best_s;

        double fr[6], ref[6];
        bool ok = given ? frenet_state_given(sp, D.ego, fr, ref) : frenet_state_at(sp, D.ego, best_s, fr, ref);
        if (!ok && !given) {
            double px, py;
            spline_xy(sp, best_s, px, py);
            if (isnan(px) || isnan(py)) {                     // coordinate_converter.py:289-295
                // (solo: the one wave scans alone -- the arg-min takes the lowest index among equal distances, whoever
                // evaluated which sample, so the entry is the four waves' one)
                ScanBest b = scan_samples(sp, x, y, 0.0, s_end, n_glob, tid, n_thr, true);
                b = solo ? wave_argmin(b) : block_argmin(b, s_best);
                best_s = linspace_at(0.0, s_end, n_glob, b.idx >= 0 ? b.idx : 0);
                ok = frenet_state_at(sp, D.ego, best_s, fr, ref);
            }
        }
        const int nb = (ok && fr[1] > 0.1) ? P.n_brake : 0;       // BRAKE_MIN_SPEED gate
        const int n_cand = ok ? D.n_grid + nb : 0;
        if (tid == 0) {
            if (inst_done) inst_done[inst] = 0;                   // tiles of this instance evaluated so far (tile_done)
            InstState &S = state[inst];
            for (int i = 0; i < 6; ++i) { S.frenet0[i] = ok ? fr[i] : NAN; S.ref0[i] = ok ? ref[i] : NAN; }
            S.new_prev_s = new_prev_s;
            S.c2f_ok = ok ? 1 : 0;
            S.n_brake = nb;
            S.n_cand = n_cand;
        }
        // The group headers of the instance (GroupHead): one lane per (position, profile).  What the lattice decides comes
        // out of the handle's template for the instance's shape, with or without the brake ladder (HeadTemplate: the
        // position's lanes share out the copy); the first lane adds the instance's own fields, and every lane forms the
        // summary of its profile.  Every position of the batch gets at least its `present` word: the table outlives the call.
        if (gh.heads) {
            const int variant = nb > 0 ? HEAD_VARIANT_BRAKE : HEAD_VARIANT_GRID;
            // Item t of the loop `t = tid; t += n_thr`, HEAD_PASSES of a thread's items at a time: the shares of all of
            // them are fetched before the first header is written (the one wave has three passes over the bench lattice's
            // 144 items where four waves have one; a pass's loads would wait behind the stores of the pass before).
            constexpr int HEAD_PASSES = 3;
            const int n_items = gh.n_pos * GROUP_MAX_PROFILES;
            for (int t0 = tid; t0 < n_items; t0 += HEAD_PASSES * n_thr) {
                HeadShare share[HEAD_PASSES];
#pragma unroll
                for (int u = 0; u < HEAD_PASSES; ++u) {
                    const int t = t0 + u * n_thr;
                    if (t >= n_items) break;
                    const int pos = t / GROUP_MAX_PROFILES, p = t - pos * GROUP_MAX_PROFILES;
                    group_head_fetch(gh.tmpl[head_template_index(D, variant, gh.tmpl_entries, pos)], p, share[u]);
                }
#pragma unroll
                for (int u = 0; u < HEAD_PASSES; ++u) {
                    const int t = t0 + u * n_thr;
                    if (t >= n_items) break;
                    const int pos = t / GROUP_MAX_PROFILES, p = t - pos * GROUP_MAX_PROFILES;
                    group_head_put(P, D, fr, ok ? 1 : 0, share[u], p, gh.heads[(int64_t)inst * gh.n_pos + pos]);
                }
            }
        }
        carry_prev_s = new_prev_s;
        chained = true;
    }
}

__global__ void __launch_bounds__(FRENET_WG)
k_frenet_state(const DevParams *__restrict__ Pp, SplineView sp_hbm, const SplineView *__restrict__ sp_table, int mixed,
               int lds_knots, const InstDesc *desc, InstState *__restrict__ state, int n_inst, MetaImport imp,
               NanScan scan, int32_t *__restrict__ inst_done, GroupHeadOut gh, int all_waves)
{
    SplineView sp = sp_hbm;
    if ((int)blockIdx.x < n_inst) {                              // (the scan blocks never look at the path)
        if (mixed) {                                             // the instance's scenario (a chain shares its head's)
            const int scen = (imp.h_desc ? imp.h_desc : desc)[blockIdx.x].scen;
            Pp += scen;
            sp_hbm = load_const(sp_table, scen);
        }
        sp = stage_spline(sp_hbm, lds_knots);
    }
    frenet_state_block(Pp, sp, desc, state, n_inst, imp, scan, inst_done, (int)blockIdx.x, gh, all_waves);
}

// ---------------------------------------------------------------------------
// candidate evaluation
// ---------------------------------------------------------------------------

// a wave-uniform double as an opaque scalar-register value
__device__ __forceinline__ double uniform_f64(double v)
{
    int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    asm volatile("" : "+s"(lo), "+s"(hi));                       // opaque: a register value, not a re-loadable address
    return __hiloint2double(hi, lo);
}

typedef float f16 __attribute__((ext_vector_type(16)));           // one chunk = 8 (x, y) pairs in 16 SGPRs

// s_load_dwordx16 of the chunk OFF bytes behind src, NOT waited for (see FusedSink::put)
template <int OFF>
__device__ __forceinline__ void sload_chunk(f16 &dst, const f2x8 *src)
{
    asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(dst) : "s"(src), "n"(OFF) : "memory");
}

// the same, issued before anything that reads `ahead` afterwards: the compiler otherwise sinks the load below the
// distance arithmetic of the chunk in use (which does not depend on it) and the wait then follows it at once
template <int OFF>
__device__ __forceinline__ void sload_chunk_ahead(f16 &dst, const f2x8 *src, float &ahead)
{
    asm volatile("s_load_dwordx16 %0, %2, %3" : "=s"(dst), "+v"(ahead) : "s"(src), "n"(OFF) : "memory");
}

// waits for every outstanding scalar load; `c` is tied in so that its uses stay behind the wait
__device__ __forceinline__ void swait_chunk(f16 &c)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(c) : : "memory");
}

// smallest float32 squared distance from (fx, fy) to the 8 entries of a chunk held in SGPRs as x[8], y[8].
// Two obstacles per instruction: v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 on (x_j, x_j+1) and (y_j, y_j+1).
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float min_sqdist32_f16(const f16 &c, float fx, float fy)
{
    const v2f px = { fx, fx }, py = { fy, fy };
    v2f t[ENT_CHUNK / 2];
#pragma unroll
    for (int j = 0; j < ENT_CHUNK / 2; ++j) {
        const v2f ox = { c[2 * j], c[2 * j + 1] }, oy = { c[8 + 2 * j], c[8 + 2 * j + 1] };
        const v2f dx = px - ox, dy = py - oy;
        t[j] = __builtin_elementwise_fma(dy, dy, dx * dx);
    }
    float m = fminf(fminf(t[0].x, t[0].y), t[1].x);
    m = fminf(fminf(m, t[1].y), t[2].x);
    m = fminf(fminf(m, t[2].y), t[3].x);
    return fminf(m, t[3].y);
}

// smallest float32 squared distance from (fx, fy) to the entries of chunks [0, n) behind cp: the double-buffered
// walk of FusedSink::put32 (same hand-issued loads, same prefetch of one chunk past the list) with one running
// minimum per lane instead of a near bit per chunk
__device__ __forceinline__ float min_sqdist32_walk(const f2x8 *cp, int n, float &fx, float fy)
{
    float m = INFINITY;
    f16 ca, cb;
    sload_chunk<0>(ca, cp);
    swait_chunk(ca);
    for (int c = 0; c < n; c += 2) {
        sload_chunk_ahead<64>(cb, cp, fx);
        m = fminf(m, min_sqdist32_f16(ca, fx, fy));
        swait_chunk(cb);
        sload_chunk_ahead<128>(ca, cp, fx);
        if (c + 1 < n) m = fminf(m, min_sqdist32_f16(cb, fx, fy));  // wave-uniform
        swait_chunk(ca);
        cp += 2;
    }
    return m;
}

// EntryCollider (fot_math.hpp) with the chunk walk on the scalar unit.  Everything that addresses the entry lists is
// wave-uniform (instance, time step), so one chunk (8 obstacles, 64 B) is one s_load_dwordx16 shared by the 64
// candidates of the wave; each lane keeps the float32 minimum squared distance of the chunk and only chunks that
// come within the conservative threshold are re-checked in float64, so the decision is the reference's.
// Scalar registers are the scarce resource of k_evaluate (two 16-register chunk buffers): the sink keeps only
// what the per-chunk loop needs, the exact re-check fetches its constants where it runs.
// k_evaluate's only parameter, i.e. the layout of its argument segment.  What only rare branches or the epilogue
// read -- the spline view, the float64 / sample-id entry arrays, the output arrays -- is fetched from the segment at
// the point of use instead of occupying scalar registers across the time-step loop.
// Agent-coherent accesses to the candidate arrays: written by one wave, read by the wave that selects for the
// instance -- possibly on another XCD, whose L2 is a different one.  Relaxed atomic accesses at agent scope are plain
// loads / stores with the sc1 bit (write-through / read-through the XCD's L2): no L2 writeback or invalidation, which
// is what an agent-scope fence costs on this multi-XCD part (every wave paying one made the launch 45 % longer).
template <typename T>
__device__ __forceinline__ void st_agent(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T ld_agent(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct EvalKernArgs {
    const DevParams *Pp; SplineView sp; const InstDesc *desc; const InstState *state;
    int row_budget, lds_knots, ablate, n_inst, max_tiles;
    const SplineView *sp_table; int mixed;           // a mixed batch: Pp + desc[inst].scen, sp_table[desc[inst].scen] (PathSet)
    const int32_t *tile_cand0;
    const GroupHead *heads;                          // the grouped kernels' headers (TileTable::heads)
    const TileStep *wave_rng; const f2 *ent32; const d2 *ent64; const uint8_t *ent_sid;
    double *cand_cost; uint8_t *cand_status; uint16_t *cand_keep;   // per candidate: for fot_debug_candidates only
    TilePart *parts;                                 // per tile: what its wave found (tile_done)
    fot_result *out; int32_t *inst_done;             // selection by the wave that finishes an instance's last tile
    int32_t *done_flag; int32_t done_seq;            // host-visible flag per record (CandArrays::done_flag)
};
// k_evaluate's argument segment: EVAL_LEAD_PTRS read-only pointers (passed on their own so that they carry
// `__restrict__`: only no-alias inputs are certain to keep their loads on the scalar unit), then this struct
constexpr int EVAL_LEAD_PTRS = 7;
__device__ __forceinline__ const EvalKernArgs &eval_kernargs()
{
    return *(const EvalKernArgs *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + EVAL_LEAD_PTRS * sizeof(void *));
}

// LEAN: the form for launches whose every instance has no chance budget (max_viol == 0) on handles of at most 64 samples
// per candidate (launch_evaluate): a certain hit always settles the candidate, so thr_fatal is thr_sure -- no lane
// register, lane read or branch for it --, hit_mask / viol are never touched (the exact re-check counts on locals: its
// first violation is a hit), and the per-step values never need a second block of 64 steps.  Same thresholds, same
// min-only walk, same per-chunk walk of the band lanes, same exact re-check: the decisions are the general form's.
// W: the words of the sample mask.  1 in every launch whose instances have at most FOT_MAX_SAMPLES samples; the WIDE
// launches (an instance of up to FOT_MAX_PLAN_SAMPLES samples on a handle with a raised capacity) take WIDE_MASK_WORDS: the
// general form then counts distinct samples in a SampleMask4 (four register pairs, touched by the exact re-check alone,
// word chosen by a select chain -- no indexed array, no scratch), the lean form re-checks without looking at sample ids.
template <bool LEAN, int W = 1>
struct FusedSink {
    typedef typename SampleMaskOf<LEAN ? 1 : W>::type Mask;
    const DevParams *Pp;
    const InstDesc *Dp;
    // The per-step values of the tile (TileStep) sit in lanes: lane l holds time step step_base + l, 64 steps at a time;
    // a walk that crosses a multiple of 64 (more than 64 samples per candidate) reloads them there (steps_reload).
    uint32_t my_rng;                     // lane l: strip range of time step step_base + l (0: nothing to test)
    float my_thr, my_thr_sure;           // lane l: the float32 thresholds of that time step (TileStep)
    float my_thr_fatal;                  // lane l: my_thr_sure where a certain hit settles the candidate (no chance
                                         // budget), else -1
    int step_base;                       // multiple of 64 (wave-uniform)
    int step_row;                        // number of this tile in the batch: its TileSteps start at step_row * n_total
    int lane_id;
    float thr, thr_fatal;                // of the current time step (wave-uniform)
    const f2x8 *chunks;                  // float32 entries of this instance, ent_cap / 8 chunks per time step
    int chunks_per_k;                    // ent_cap / 8
    Mask hit_mask;
    int viol;
    bool hit;
    int c_lo, n_chunks;                  // chunk range of the current time step
    uint32_t pf;                         // destination of the warm-up loads below, reserved until they have landed
    bool no_warm;

    // Reads the range of time step k and touches the first cache lines of its chunks, so that they are on their
    // way into the scalar cache while the sample arithmetic runs.  The loads are hand-issued and their (unused)
    // destination register stays tied to the sink until pf_wait(): a scalar load retires at any later time, and
    // must not land in a register the compiler has meanwhile given to something else.
    // lane l <- TileStep of time step base + l of this tile (every lane of the wave is active here: the region that
    // calls row_begin holds lanes 0 .. min(n_total, 64) - 1 at least, all 64 once a second block of steps exists)
    __device__ __forceinline__ void steps_load(int base)
    {
        const DevParams &P = *Pp;
        const EvalKernArgs &KA = eval_kernargs();
        TileStep st = { 0u, 0.0f, 0.0f, 0u };
        if (Dp->ent_cap != 0 && base + lane_id < P.n_total && !(KA.ablate & 1))
            st = KA.wave_rng[(int64_t)step_row * P.n_total + base + lane_id];
        my_rng = st.rng; my_thr = st.thr; my_thr_sure = st.thr_sure;
        my_thr_fatal = Dp->max_viol == 0 ? st.thr_sure : -1.0f;
        step_base = base;
    }

    __device__ __forceinline__ void row_begin(int k)
    {
        if constexpr (!LEAN)
            if ((k & ~(WAVE - 1)) != step_base) steps_load(k & ~(WAVE - 1));  // wave-uniform; never taken up to 64 samples
        const int kl = LEAN ? k : k & (WAVE - 1);
        const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)my_rng, kl);
        c_lo = (int)(r >> 16);
        n_chunks = (int)(r & 0xffffu) - c_lo;
        thr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_thr), kl));
        thr_fatal = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, LEAN ? my_thr_sure : my_thr_fatal), kl));
        if (n_chunks > 0 && !no_warm) {
            const f2x8 *row = chunks + (int64_t)k * chunks_per_k + c_lo;
            asm volatile("s_load_dword %0, %1, 0x0\n\t"
                         "s_load_dword %0, %1, 0x40\n\t"
                         "s_load_dword %0, %1, 0x80\n\t"
                         "s_load_dword %0, %1, 0xc0"
                         : "=&s"(pf) : "s"(row) : "memory");          // (early clobber: four loads read `row`)
        } else {
            pf = 0;
        }
    }

    // end of the time step, reached by every lane: the warm-up loads have landed, pf may be reused
    __device__ __forceinline__ void row_end(int) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(pf) : : "memory"); }

    // the current time step has chunks to test a point against (wave-uniform; put32 returns at once without)
    __device__ __forceinline__ bool step_has_points() const { return n_chunks != 0; }

    __device__ __forceinline__ void put(int k, int ci, double px, double py, bool alive)
    {
        // (the rows are instance-local: evaluate_tile) -- the point itself is its own exact form
        put32(k, ci, (float)px, (float)py, alive, [&](double &ex, double &ey) { ex = px; ey = py; });
    }

    // the point in the instance-local float32 frame; get_exact(px, py) yields its float64 coordinates, asked for only by
    // the lanes whose float32 distance to some entry lies between the two thresholds
    template <class GetExact>
    __device__ __forceinline__ void put32(int k, int, float fx_in, float fy, bool alive, const GetExact &get_exact)
    {
        if (n_chunks == 0) return;                                // wave-uniform
        if (!alive || hit) return;                                // lanes whose collision outcome is already settled
        float fx = fx_in;                                         // (tied into the hand-issued loads below)
        const f2x8 *row = chunks + (int64_t)k * chunks_per_k + c_lo;
        if (LEAN || thr_fatal >= 0.0f) {                          // wave-uniform: a certain hit settles the candidate
            // Min-only walk: one running minimum over every chunk of the step, no per-chunk compare, bit or exec-mask
            // work.  A minimum at or below thr_fatal is a certain hit (some chunk's minimum is); a minimum above thr
            // means that no chunk of the step is near, so the classic walk below would neither set a near bit nor
            // re-check anything.  Only the lanes in between -- a float32 distance in the thin band (thr_sure, thr] --
            // walk the step again below, and there decide exactly as every lane did before.
            const float m = min_sqdist32_walk(row, n_chunks, fx, fy);
            if (m <= thr_fatal) { hit = true; return; }
            if (!(m <= thr)) return;
        }
        bool sure = false;                                        // some obstacle is certainly within its radius
        for (int c0 = 0; c0 < n_chunks; c0 += 32) {               // 32 chunks per pass: one bit per chunk and lane
            const int nb = n_chunks - c0 < 32 ? n_chunks - c0 : 32;   // (may be odd: the last pair then tests one chunk)
            const f2x8 *cp = row + c0;
            uint32_t near_bits = 0;                               // chunk c0+i within the threshold -> bit nb-1-i
            // Branch-free loop over two chunk buffers filled by hand-issued scalar loads.  SMEM returns out of
            // order, so a compiler-placed wait for the chunk in use would also wait for the prefetch behind it;
            // the loads are therefore inline asm (invisible to the waitcnt pass) and each buffer is waited for
            // right before its own use, one chunk of arithmetic after its load was issued.  The last pair
            // prefetches one chunk past the list (allocated slack, never used).
            f16 ca, cb;
            sload_chunk<0>(ca, cp);
            swait_chunk(ca);
            for (int c = 0; c < nb; c += 2) {
                sload_chunk_ahead<64>(cb, cp, fx);
                const float ma = min_sqdist32_f16(ca, fx, fy);
                near_bits = (near_bits << 1) | (uint32_t)(ma <= thr);
                sure |= ma <= thr_fatal;
                swait_chunk(cb);
                sload_chunk_ahead<128>(ca, cp, fx);
                if (c + 1 < nb) {                                     // wave-uniform
                    const float mb = min_sqdist32_f16(cb, fx, fy);
                    near_bits = (near_bits << 1) | (uint32_t)(mb <= thr);
                    sure |= mb <= thr_fatal;
                }
                swait_chunk(ca);
                cp += 2;
            }
            // a single violation is fatal (no chance constraint budget): a certain float32 hit settles the candidate
            if (sure) { hit = true; return; }
            if (near_bits != 0) {
                double px, py;
                get_exact(px, py);
                exact(k, c0, nb, near_bits, px, py, fx, fy);
            }
        }
    }

    // rare: exact float64 re-check of the chunks whose float32 distance came within the threshold
    __device__ __forceinline__ void exact(int k, int c0, int nb, uint32_t near_bits, double px, double py, float fx,
                                          float fy)
    {
        const DevParams &P = *Pp;
        const InstDesc &D = *Dp;
        px += D.ego.x; py += D.ego.y;                             // the exact entries are in the caller's frame
        const double sq_dyn = D.dyn_mode == FOT_DYN_SINGLE ? P.sq_r_dyn : P.sq_r;
        const EvalKernArgs &KA = eval_kernargs();
        const float thr_sure = LEAN ? thr_fatal :
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_thr_sure), k & (WAVE - 1)));
        const d2 *e64 = KA.ent64 + D.ent_off;
        const uint8_t *sid = KA.ent_sid + D.ent_off;
        const int64_t base = ((int64_t)k * chunks_per_k + c_lo) * ENT_CHUNK;
        uint64_t mask_l = 0;                                      // (LEAN: no budget, nothing outlives the first violation)
        int viol_l = 0;
        while (near_bits != 0 && !hit) {
            const int hb = 31 - __clz((int)near_bits);             // highest bit = earliest chunk
            near_bits &= ~(1u << hb);
            const int64_t e = base + (int64_t)(c0 + nb - 1 - hb) * ENT_CHUNK;
            if constexpr (LEAN && W != 1)                           // (ids of 64 and more: no one-word mask may see them)
                exact_chunk_f32first_nobudget(chunks[e / ENT_CHUNK], e64 + e, sid + e, fx, fy, thr, thr_sure, px, py, P.sq_r,
                                              sq_dyn, hit);
            else if constexpr (LEAN)
                exact_chunk_f32first(chunks[e / ENT_CHUNK], e64 + e, sid + e, fx, fy, thr, thr_sure, px, py, P.sq_r, sq_dyn,
                                     0, mask_l, viol_l, hit);
            else
                exact_chunk_f32first(chunks[e / ENT_CHUNK], e64 + e, sid + e, fx, fy, thr, thr_sure, px, py, P.sq_r, sq_dyn,
                                     D.max_viol, hit_mask, viol, hit);
        }
    }

    __device__ __forceinline__ bool collided() const { return hit; }
};

// Longitudinal rows of a tile's profiles in the wave's own slice of LDS: the 64 candidates of a tile share two or
// three longitudinal profiles (seven short ones in the brake-ladder tile).  Per profile a run of rows [k][field],
// 9 fields = 72 contiguous bytes per row (the arc length s is not in the row: only the low-speed rule and the
// travelled distance read it, and they rebuild it from the profile's polynomial); a profile's run holds
// profile_rows() rows and lanes clamp their row index to it (the last row of a brake-ladder profile is its hold).
constexpr int EVAL_WG = WAVES_PER_GROUP * WAVE;
extern __shared__ double s_lon[];

constexpr int ROW_FIELDS = 9;
constexpr int LONINFO_DOUBLES = (int)(sizeof(LonInfo) / sizeof(double));
static_assert(sizeof(LonInfo) % sizeof(double) == 0, "LonInfo sits in the double-typed LDS array");
// doubles of LDS per wave: rows | profile summaries | row offsets of the profiles (ints)
__host__ __device__ constexpr int eval_wave_doubles(int row_budget)
{
    return row_budget * ROW_FIELDS + TILE_MAX_PROFILES * LONINFO_DOUBLES + TILE_MAX_PROFILES / 2;
}
// doubles of LDS of a group's shared table (k_evaluate_group)
__host__ __device__ constexpr int eval_group_doubles()
{
    return GROUP_ROWS * ROW_FIELDS + (int)(sizeof(GroupHead) / sizeof(double));   // rows | the group's header
}
// A tile cut into time segments (k_evaluate_split): what a later segment hands to the wave of segment 0, per lane
constexpr int SEG_MAX = 4;
constexpr int SEG_F64 = 4, SEG_I32 = 4;  // d_last, v_last, max_step2, hit_mask | flags, first_nan, k_last, hit
// (the general form of a wide launch hands over WIDE_MASK_WORDS mask words: slots 3 .. 3 + words - 1, the ints behind them)
__host__ __device__ constexpr int seg_doubles(int mask_words) { return (SEG_F64 + mask_words - 1 + SEG_I32 / 2) * WAVE; }

// FLAT (the walk of an exactly straight path, frenet_to_cart<., true>): the step reads neither kr nor dkr of its row.
template <bool FLAT = false>
struct StagedTabT {
    static constexpr bool LOCAL = true;  // rx, ry relative to the ego position (evaluate_tile builds them so)
    int lds_row0;                        // index of this lane's profile row 0 in s_lon
    int k_max;                           // last row of the run (grid: n_t - 1; brake ladder: the hold row n_eval)
    double dt;
#ifdef FOT_TIMELINE
    mutable uint64_t t_rows = 0;         // shader cycles between issuing the row reads and having them (diagnostic)
#endif
    __device__ __forceinline__ void load(int k, LonSample &L) const
    {
#ifdef FOT_TIMELINE
        const uint64_t t0 = __builtin_amdgcn_s_memtime();
#endif
        const int kk = k < k_max ? k : k_max;
        const double *r = s_lon + lds_row0 + kk * ROW_FIELDS;
        L.s = 0.0; L.sd = r[0]; L.sdd = r[1]; L.rx = r[2]; L.ry = r[3];
        // the row is in registers from here on: what follows (the sink's scalar warm-up loads) must not sit
        // between these reads and the wait for them
        if constexpr (FLAT) {
            L.cos_r = r[4]; L.sin_r = r[5]; L.kr = 0.0; L.dkr = 0.0; L.inv_sd = r[8];   // (kr, dkr: never read)
            asm volatile("" : "+v"(L.sd), "+v"(L.sdd), "+v"(L.rx), "+v"(L.ry), "+v"(L.cos_r), "+v"(L.sin_r),
                              "+v"(L.inv_sd));
        } else {
            L.cos_r = r[4]; L.sin_r = r[5]; L.kr = r[6]; L.dkr = r[7]; L.inv_sd = r[8];
            asm volatile("" : "+v"(L.sd), "+v"(L.sdd), "+v"(L.rx), "+v"(L.ry), "+v"(L.cos_r), "+v"(L.sin_r),
                              "+v"(L.kr), "+v"(L.dkr), "+v"(L.inv_sd));
        }
#ifdef FOT_TIMELINE
        t_rows += __builtin_amdgcn_s_memtime() - t0;
#endif
    }
    // arc length s(t_k): asked for by the low-speed rules only (a few percent of the samples, but every eighth time
    // step of a wave has such a lane) -- lanes re-read their profile's coefficients from the tile's summaries
    const LonInfo *info;                 // in LDS
    __device__ __forceinline__ double s_at(int k) const
    {
        double s_, u0, u1, u2;
        lon_sample(*info, k, dt, s_, u0, u1, u2);
        return s_;
    }
    // the reference frame of row k alone, through load()'s clamp: for k - 1 the row step k - 1 read (the low-speed rule)
    __device__ __forceinline__ void frame_at(int k, double &cos_r, double &sin_r) const
    {
        const int kk = k < k_max ? k : k_max;
        const double *r = s_lon + lds_row0 + kk * ROW_FIELDS;
        cos_r = r[4]; sin_r = r[5];
    }
};
using StagedTab = StagedTabT<>;

#ifdef FOT_TIMELINE
// diagnostic build (scripts/timeline.sh): per tile of the last k_evaluate launch -- tile start, start of the sample
// loop (after the LDS rows are built), tile end on the 100 MHz clock, and the chunks its strip ranges cover
__device__ uint64_t g_timeline[4 * 16384];
__device__ uint64_t g_shader_clock[2 * 16384];     // s_memtime at loop start / end: shader cycles (in-kernel clock)
__device__ uint64_t g_row_wait[16384];             // shader cycles lane 0 spent between issuing and having its LDS rows
__device__ uint64_t g_phase[4 * 16384];            // kernel entry, spline staged, profile summaries ready, loop done
__shared__ uint64_t s_tl_entry[2];                 // kernel entry / spline staged, of this workgroup
extern "C" int fot_timeline_read_phase(uint64_t *out, int n_words)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(uint64_t) * (size_t)n_words);
}
extern "C" int fot_timeline_read_rows(uint64_t *out, int n_words)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_row_wait), sizeof(uint64_t) * (size_t)n_words);
}
extern "C" int fot_timeline_read(uint64_t *out, int n_words)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), sizeof(uint64_t) * (size_t)n_words);
}
extern "C" int fot_timeline_read_clock(uint64_t *out, int n_words)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_shader_clock), sizeof(uint64_t) * (size_t)n_words);
}
#endif

// this wave's LDS writes (other lanes') before the reads that follow, and the reads before the next writes
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// What a tile's wave leaves behind, every lane of it: the candidates' final statuses (stop-distance filter included,
// frenet_planner.py:307-324) in the candidate arrays and, in tp, what the selection needs of the tile: the histogram of
// the statuses and the cheapest 'ok' candidate (lowest index among equals)
template <class Tab>
__device__ __forceinline__ void tile_results(const DevParams &P, const InstDesc &D, const Tab &tab, const LonInfo &L,
                                             const double *q, SegState &g, bool hit, bool has_cand, int64_t slot, int cand0,
                                             int lane, TilePart &tp)
{
    int st_final = FOT_ST_DROPPED;
    ScanBest mine = { INFINITY, -1 };
    int my_keep = 0;
    if (has_cand) {
        CandResult r;
        {
            LonInfo Lf = *tab.info;                              // (read again here: not carried through the walk)
            Lf.n_t = L.n_t;
            finish_candidate(P, D, Lf, tab, q, g, hit, r);
        }
        st_final = final_status(r.status, r.v_last, r.travel, D.max_stop);
        const EvalKernArgs &KA = eval_kernargs();
        KA.cand_cost[slot] = r.cost;
        KA.cand_status[slot] = (uint8_t)st_final;
        KA.cand_keep[slot] = (uint16_t)r.keep;
        my_keep = r.keep;
        mine = select_entry(st_final, r.cost, cand0 + lane);     // (a cost not below +inf is never selected)
    }
    {
        const ScanBest best = wave_argmin(mine);                 // every lane of the wave is here
        tp.cost = best.dist; tp.idx = best.idx;
        tp.keep = __builtin_amdgcn_readfirstlane(__shfl(my_keep, best.idx >= 0 ? best.idx - cand0 : 0, WAVE));
#pragma unroll
        for (int c = 0; c < 8; ++c) tp.cnt[c] = __popcll(__ballot(st_final == c));
    }
}

// One tile: rows of its profiles into LDS, then one candidate per lane.
//   TILE_WAVE   the wave owns the tile and its slice of LDS (rows_base).
//   TILE_SPLIT  the workgroup's n_sub waves share the tile -- they build the rows together, wave `sub` walks the time
//               steps [sub, sub + 1) * ceil(n_loop / n_sub) of every candidate, and wave 0 merges the segments
//               (seg_merge) through `s_part`.
// (The grouped cut has its own form, evaluate_group_tile below.)
enum { TILE_WAVE = 0, TILE_SPLIT = 1 };
template <int MODE, bool LEAN, bool FLAT = false, int W = 1>
__device__ __forceinline__ void evaluate_tile(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc,
                                              const InstState *__restrict__ state,
                                              const int32_t *__restrict__ tile_cand0, const int32_t *__restrict__ tile_n,
                                              const TileStep *__restrict__ wave_rng, const f2 *__restrict__ ent32,
                                              const EvalKernArgs &a, const SplineView &sp_lds,
                                              double *my_rows, int inst, int tile, int lane, int tl_tag, TilePart &tp,
                                              int sub = 0, int n_sub = 1, double *s_part = nullptr)
{
    constexpr bool SPLIT = MODE == TILE_SPLIT;
    const int seg = SPLIT ? sub : 0, n_seg = SPLIT ? n_sub : 1;
    const DevParams &P = *Pp;
    const InstDesc &D = desc[inst];
    const InstState &S = state[inst];
    const int n_total = P.n_total;
    const int cand0 = tile_cand0[D.shape_off + tile];
    int n = tile_n[D.shape_off + tile];
    // candidates whose profiles are staged in this slice: the tile's own
    int stage_c0 = cand0, stage_c1 = cand0 + n;                  // [first, one past the last)
    if (n <= 0) return;                                          // (a padding tile of the grouped cut)
    if (!S.c2f_ok || stage_c0 >= S.n_cand) return;              // (the brake ladder of a standing ego) -- the whole workgroup
    if (stage_c1 > S.n_cand) stage_c1 = S.n_cand;
    if (cand0 + n > S.n_cand) n = S.n_cand - cand0 > 0 ? S.n_cand - cand0 : 0;
#ifdef FOT_TIMELINE
    const uint64_t t_blk = __builtin_amdgcn_s_memrealtime();
#endif
    LonInfo *s_info = (LonInfo *)(my_rows + a.row_budget * ROW_FIELDS);
    int *s_row0 = (int *)(s_info + TILE_MAX_PROFILES);
    // staged profiles: of the first .. last staged candidate (slots grow with the candidate index)
    const int slot_lo = decode_candidate(P, D, S.frenet0, stage_c0).lon_slot;
    const int n_stage = decode_candidate(P, D, S.frenet0, stage_c1 - 1).lon_slot - slot_lo + 1;
    const auto lds_fence = [] { if constexpr (MODE != TILE_WAVE) __syncthreads(); else wave_lds_fence(); };
    if constexpr (MODE == TILE_WAVE) wave_lds_fence();           // the previous tile's rows are no longer read
    // who builds: the wave itself, or all waves of the workgroup together
    const int bld_id = (MODE == TILE_WAVE ? 0 : sub * WAVE) + lane, bld_n = (MODE == TILE_WAVE ? 1 : n_sub) * WAVE;
    int total_rows = 0, n_loop = 0;
    for (int p = 0; p < n_stage; ++p) {                         // wave-uniform: a handful of scalar operations
        const int r = profile_rows(P, D, slot_lo + p);
        if (bld_id == p) s_row0[p] = total_rows;
        total_rows += r;
    }
    if (bld_id < n_stage) s_info[bld_id] = profile_info(P, D, S.frenet0, slot_lo + bld_id, true);
    lds_fence();
#ifdef FOT_TIMELINE
    const uint64_t t_info = __builtin_amdgcn_s_memrealtime();
#endif
    for (int i = bld_id; i < total_rows; i += bld_n) {
        int p = 0;
        for (int pp = 1; pp < n_stage; ++pp) p = i >= s_row0[pp] ? pp : p;
        const int k = i - s_row0[p];
        const LonInfo Lp = s_info[p];
        LonSample ls;
        double sddd;
        make_lon_sample(sp_lds, Lp, k, P.dt, ls, sddd);         // (k == n_eval of a brake profile: its hold state)
        double *r = my_rows + (int64_t)i * ROW_FIELDS;
        // the reference point in the instance-local frame (origin: the ego position, like the entry lists): the walk then
        // hands its points to the collision test as they are, and nothing else of it depends on the frame
        r[0] = ls.sd; r[1] = ls.sdd; r[2] = ls.rx - D.ego.x; r[3] = ls.ry - D.ego.y;
        r[4] = ls.cos_r; r[5] = ls.sin_r; r[6] = ls.kr; r[7] = ls.dkr; r[8] = ls.inv_sd;
    }
    lds_fence();
    // the time steps this tile needs: the longest of its OWN profiles -- and the steps before any of them holds (ne_min of
    // evaluate_segment: the slots between the first and the last candidate's are the ones its lanes read).  SREG: only the
    // lean split kernel has the scalar registers for that form of the walk (the others would lane-spill them)
    constexpr bool SREG = LEAN && SPLIT;
    int ne_min = INT_MAX;
    {
        const int own_lo = decode_candidate(P, D, S.frenet0, cand0).lon_slot - slot_lo;
        const int own_hi = decode_candidate(P, D, S.frenet0, cand0 + n - 1).lon_slot - slot_lo;
        for (int p = own_lo; p <= own_hi; ++p) {
            const int nt = s_info[p].n_t, ne = s_info[p].n_eval;
            n_loop = nt > n_loop ? nt : n_loop; ne_min = ne < ne_min ? ne : ne_min;
        }
        n_loop = __builtin_amdgcn_readfirstlane(n_loop);
        ne_min = __builtin_amdgcn_readfirstlane(ne_min);
    }
    // this wave's time steps
    const int seg_len = (n_loop + n_seg - 1) / n_seg;
    const int k0 = SPLIT ? seg * seg_len : 0;
    const int k1 = SPLIT ? (k0 + seg_len < n_loop ? k0 + seg_len : n_loop) : n_loop;

    // lane l holds the strip range of time step step_base + l (read back with v_readlane), 64 steps at a time: loaded
    // while every lane of the wave is still active, lanes without a candidate included
    const int step_base0 = k0 & ~(WAVE - 1);
    TileStep my_step = { 0u, 0.0f, 0.0f, 0u };
    if (D.ent_cap != 0 && step_base0 + lane < n_total && !(a.ablate & 1))
        my_step = wave_rng[(int64_t)(D.tile0 + tile) * n_total + step_base0 + lane];
    const uint32_t my_rng = my_step.rng;
    // (while every lane is active: the time-step loop reads lane k of these, candidate or not)
    const float my_thr_fatal = LEAN ? 0.0f : D.max_viol == 0 ? my_step.thr_sure : -1.0f;   // (LEAN: not read)
#ifdef FOT_TIMELINE
    const uint64_t t_wave = __builtin_amdgcn_s_memrealtime();
    const uint64_t c_wave = __builtin_amdgcn_s_memtime();
    const int tl_wave = D.tile0 + tile;
    uint64_t tl_rows = 0;
    int tl_chunks = (int)(my_rng & 0xffffu) - (int)(my_rng >> 16);
    for (int o = 32; o > 0; o >>= 1) tl_chunks += __shfl_xor(tl_chunks, o);
#endif
    // per-lane state that outlives the segment loop in the split form
    SegState g;
    seg_init(g);
    LonInfo L;
    StagedTabT<FLAT> tab;
    typedef typename FusedSink<LEAN, W>::Mask Mask;
    constexpr int MASK_WORDS = LEAN ? 1 : W;                     // words of a segment's hand-over (seg_doubles)
    Mask hit_mask = Mask();
    bool hit = false;
    int64_t slot = 0;
    double q[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };              // lateral quintic of the lane's candidate
    // Lanes 0 .. n_total-1 hold the per-step values of the tile (my_step) that the time-step loop reads ACROSS lanes
    // (v_readlane of lane k): they must be active wherever the compiler may place a copy of those registers, so they
    // all enter the region below -- a lane without a candidate walks an empty path (n_t = 0).
    const bool has_cand = lane < n;
    if (has_cand || lane < n_total) {                            // (n_total > 64: every lane)
        const int idx = cand0 + (has_cand ? lane : 0);           // candidate index inside the instance
        slot = (int64_t)D.cand_off + idx;
        const CandDecode cd = decode_candidate(P, D, S.frenet0, idx);
        const int p = cd.lon_slot - slot_lo;
        L = s_info[p];
        if (!has_cand) L.n_t = 0;
        tab.lds_row0 = (int)(my_rows - s_lon) + s_row0[p] * ROW_FIELDS;
        tab.k_max = profile_rows(P, D, cd.lon_slot) - 1;
        tab.info = s_info + p;
        lat_coeffs(S.frenet0, cd.di, cd.brake ? P.brake[cd.ti] : P.ti[cd.ti], q);
        // q[0..2] are the instance's lateral state (wave-uniform): as scalar values they end up in spilled SGPRs and
        // come back through v_readlane in every time step -- three vector registers are cheaper
        asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]));

        FusedSink<LEAN, W> sink;
        sink.Pp = Pp; sink.Dp = &D;
        sink.my_rng = my_rng;
        sink.my_thr = my_step.thr; sink.my_thr_sure = my_step.thr_sure; sink.thr = 0.0f; sink.thr_fatal = -1.0f;
        sink.my_thr_fatal = my_thr_fatal;
        sink.step_base = step_base0; sink.step_row = D.tile0 + tile; sink.lane_id = lane;
        sink.chunks = (const f2x8 *)(ent32 + D.ent_off);
        sink.chunks_per_k = D.ent_cap / ENT_CHUNK;
        sink.hit_mask = Mask(); sink.viol = 0; sink.hit = false; sink.n_chunks = 0; sink.c_lo = 0; sink.pf = 0;
        sink.no_warm = (a.ablate & 2) != 0;
        // loop constants as opaque register values: the compiler then keeps them instead of re-fetching each one from
        // the parameter blocks, behind a scalar-memory wait, in every time step
        LoopConst lc = loop_const(P, D);
        // The limits live in VECTOR registers although they are wave-uniform: as scalars they do not fit next to the two
        // chunk buffers, get lane-spilled and come back through ~27 v_readlane per time step -- vector issue slots of a
        // kernel that is bound by exactly those (r02: 0.257 -> 0.242 ms).  12 VGPRs; the kernel still fits 168.
        asm volatile("" : "+v"(lc.dt), "+v"(lc.lim_speed), "+v"(lc.lim_accel), "+v"(lc.lim_curv), "+v"(lc.lim_lat),
                          "+v"(lc.road_lim));
        // (the arc step of the low-speed rule reads the table's dt: the same vector register, not a scalar copy of
        //  P.dt that is lane-spilled before the loop and read back by two v_readlane in that branch)
        tab.dt = lc.dt;
        if constexpr (!LEAN) {                                   // (LEAN: the single centre circle, never read)
            lc.n_circ_fp = __builtin_amdgcn_readfirstlane(lc.n_circ_fp);
            asm volatile("" : "+s"(lc.n_circ_fp));
        }
        evaluate_segment<LEAN, SREG, FLAT>(P, lc, L, tab, q, k0, k1, sink, g, ne_min);   // (SPLIT: a quarter of the steps -- latency, not issue, bound)
        hit_mask = sink.hit_mask; hit = sink.hit;
#ifdef FOT_TIMELINE
        tl_rows = tab.t_rows;
#endif
    }
#ifdef FOT_TIMELINE
    const uint64_t t_loop_end = __builtin_amdgcn_s_memrealtime();
#endif
    if constexpr (SPLIT) {
        // segments 1.. leave their state in LDS, the wave of segment 0 folds them in, in time order
        double *pf = s_part + (seg - 1) * seg_doubles(MASK_WORDS);
        int *pi = (int *)(pf + (SEG_F64 + MASK_WORDS - 1) * WAVE);
        if (seg > 0 && has_cand) {
            pf[0 * WAVE + lane] = g.d_last; pf[1 * WAVE + lane] = g.v_last;
            pf[2 * WAVE + lane] = g.acc.max_step2;
            if constexpr (MASK_WORDS == 1) ((uint64_t *)pf)[3 * WAVE + lane] = hit_mask;
            else {
                ((uint64_t *)pf)[3 * WAVE + lane] = hit_mask.w0; ((uint64_t *)pf)[4 * WAVE + lane] = hit_mask.w1;
                ((uint64_t *)pf)[5 * WAVE + lane] = hit_mask.w2; ((uint64_t *)pf)[6 * WAVE + lane] = hit_mask.w3;
            }
            pi[0 * WAVE + lane] = (int)g.acc.fl; pi[1 * WAVE + lane] = g.first_nan;
            pi[2 * WAVE + lane] = g.k_last; pi[3 * WAVE + lane] = hit ? 1 : 0;
        }
        __syncthreads();
        if (seg != 0) return;
        if (has_cand) {
            for (int sg = 1; sg < n_seg; ++sg) {
                if (sg * seg_len >= L.n_t) break;                // that segment held no sample of this candidate
                const double *qf = s_part + (sg - 1) * seg_doubles(MASK_WORDS);
                const int *qi = (const int *)(qf + (SEG_F64 + MASK_WORDS - 1) * WAVE);
                SegState nx;
                nx.d_last = qf[0 * WAVE + lane]; nx.v_last = qf[1 * WAVE + lane];
                nx.acc.max_step2 = qf[2 * WAVE + lane];
                nx.acc.fl = (uint32_t)qi[0 * WAVE + lane]; nx.first_nan = qi[1 * WAVE + lane];
                nx.k_last = qi[2 * WAVE + lane];
                if (seg_merge(g, nx)) {
                    if constexpr (MASK_WORDS == 1) hit_mask |= ((const uint64_t *)qf)[3 * WAVE + lane];
                    else {
                        const uint64_t *qm = (const uint64_t *)qf;
                        const SampleMask4 o = { qm[3 * WAVE + lane], qm[4 * WAVE + lane], qm[5 * WAVE + lane], qm[6 * WAVE + lane] };
                        mask_or(hit_mask, o);
                    }
                    hit |= qi[3 * WAVE + lane] != 0;
                }
            }
            if constexpr (MASK_WORDS == 1) hit |= __popcll(hit_mask) > D.max_viol;
            else hit |= mask_count(hit_mask) > D.max_viol;
        }
    }
    // The candidate's final status (stop-distance filter included, frenet_planner.py:307-324) and, per tile, what the
    // selection needs: the histogram of the statuses and the cheapest 'ok' candidate (lowest index among equals)
    int st_final = FOT_ST_DROPPED;
    ScanBest mine = { INFINITY, -1 };
    int my_keep = 0;
    if (has_cand) {
        CandResult r;
        {
            LonInfo Lf = *tab.info;                              // (read again here: not carried through the walk)
            Lf.n_t = L.n_t;
            finish_candidate(P, D, Lf, tab, q, g, hit, r);
        }
        st_final = final_status(r.status, r.v_last, r.travel, D.max_stop);
        const EvalKernArgs &KA = eval_kernargs();
        KA.cand_cost[slot] = r.cost;
        KA.cand_status[slot] = (uint8_t)st_final;
        KA.cand_keep[slot] = (uint16_t)r.keep;
        my_keep = r.keep;
        mine = select_entry(st_final, r.cost, cand0 + lane);     // (a cost not below +inf is never selected)
    }
    {
        const ScanBest best = wave_argmin(mine);                 // every lane of the wave is here
        tp.cost = best.dist; tp.idx = best.idx;
        tp.keep = __builtin_amdgcn_readfirstlane(__shfl(my_keep, best.idx >= 0 ? best.idx - cand0 : 0, WAVE));
#pragma unroll
        for (int c = 0; c < 8; ++c) tp.cnt[c] = __popcll(__ballot(st_final == c));
    }
#ifdef FOT_TIMELINE
    tl_rows = (uint64_t)__shfl((unsigned long long)tl_rows, 0);
    if (tl_wave < 16384 && lane == 0) {
        g_timeline[tl_wave * 4 + 0] = t_blk; g_timeline[tl_wave * 4 + 1] = t_wave;
        g_timeline[tl_wave * 4 + 2] = __builtin_amdgcn_s_memrealtime();
        g_timeline[tl_wave * 4 + 3] = (uint64_t)(uint32_t)tl_chunks | ((uint64_t)(uint32_t)tl_tag << 32);
        g_shader_clock[tl_wave * 2 + 0] = c_wave; g_shader_clock[tl_wave * 2 + 1] = __builtin_amdgcn_s_memtime();
        g_row_wait[tl_wave] = tl_rows;
        g_phase[tl_wave * 4 + 0] = s_tl_entry[0]; g_phase[tl_wave * 4 + 1] = s_tl_entry[1];
        g_phase[tl_wave * 4 + 2] = t_info; g_phase[tl_wave * 4 + 3] = t_loop_end;
    }
#endif
}

// The same for the grouped cut (fot_math.hpp): the workgroup's GROUP_TILES waves take the tiles of one group, wave `sub`
// the tile `tile`; they build the rows of ALL the group's profiles together, each walks its own tile.  Nothing is derived here
// that no lane decides: it comes out of the group's header (GroupHead, built by k_frenet_state), which the caller has put
// into LDS behind the rows, all waves behind a barrier.  The per-lane set-up is issued BEFORE the rows are built -- it
// reads none -- so that its loads (the step ranges, the horizon's matrices) and integer divisions run under the build.
template <bool LEAN, bool FLAT = false, int W = 1>
__device__ __forceinline__ void evaluate_group_tile(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc,
                                                    const TileStep *__restrict__ wave_rng, const f2 *__restrict__ ent32,
                                                    const EvalKernArgs &a, const SplineView &sp_lds, double *my_rows,
                                                    int inst, int tile, int sub, int lane, int tl_tag, TilePart &tp, bool full)
{
    if (!full) return;                                           // (GROUP_HEAD_EMPTY: the whole workgroup)
    const DevParams &P = *Pp;
    const InstDesc &D = desc[inst];                             // (an address: read by the rare branches and behind the loop)
    const GroupHead *head = (const GroupHead *)(my_rows + GROUP_ROWS * ROW_FIELDS);
    const auto uni = [](const int32_t &v) { return __builtin_amdgcn_readfirstlane(v); };   // wave-uniform: a scalar register
    const LonInfo *info_tab = head->info;
    const int *row0_tab = head->row0;
    const int n_total = uni(head->n_total), total_rows = uni(head->total_rows), slot_lo = uni(head->slot_lo);
    const int cand0 = uni(head->t_cand0[sub]), n = uni(head->t_n[sub]), n_loop = uni(head->t_n_loop[sub]);
    const int inst_tile0 = uni(head->tile0), ent_cap = uni(head->ent_cap);
#ifdef FOT_TIMELINE
    const uint64_t t_blk = __builtin_amdgcn_s_memrealtime(), t_info = t_blk;
#endif
    // lane l holds the strip range of time step l (read back with v_readlane): loaded while every lane of the wave is
    // still active, lanes without a candidate included
    TileStep my_step = { 0u, 0.0f, 0.0f, 0u };
    if (n > 0 && ent_cap != 0 && lane < n_total && !(a.ablate & 1))
        my_step = wave_rng[(int64_t)(inst_tile0 + tile) * n_total + lane];
    const uint32_t my_rng = my_step.rng;
    const float my_thr_fatal = LEAN ? 0.0f : uni(head->max_viol) == 0 ? my_step.thr_sure : -1.0f;   // (LEAN: not read)
    SegState g;
    seg_init(g);
    LonInfo L;
    StagedTabT<FLAT> tab;
    LoopConst lc;
    int64_t slot = 0;
    double q[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };              // lateral quintic of the lane's candidate
    // (lanes 0 .. n_total-1 enter both regions below, candidate or not: see evaluate_tile)
    const bool has_cand = lane < n;
    const bool walks = has_cand || lane < n_total;
    if (n > 0 && walks) {
        const int idx = cand0 + (has_cand ? lane : 0);           // candidate index inside the instance
        slot = (int64_t)uni(head->cand_off) + idx;
        const CandDecode cd = decode_candidate(*head, *head, head->frenet0, idx);
        const int p = cd.lon_slot - slot_lo;
        L = info_tab[p];
        if (!has_cand) L.n_t = 0;
        tab.lds_row0 = (int)(my_rows - s_lon) + row0_tab[p] * ROW_FIELDS;
        tab.k_max = row0_tab[p + 1] - row0_tab[p] - 1;           // (profile_rows() of the slot, less one)
        tab.info = info_tab + p;
        lat_coeffs(head->frenet0, cd.di, cd.brake ? P.brake[cd.ti] : P.ti[cd.ti], q);
        asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]));   // (vector registers: see evaluate_tile)
        lc.dt = head->dt; lc.road_lim = head->road_lim;
        lc.lim_speed = head->lim_speed; lc.lim_accel = head->lim_accel; lc.lim_curv = head->lim_curv; lc.lim_lat = head->lim_lat;
        asm volatile("" : "+v"(lc.dt), "+v"(lc.lim_speed), "+v"(lc.lim_accel), "+v"(lc.lim_curv), "+v"(lc.lim_lat),
                          "+v"(lc.road_lim));
        tab.dt = lc.dt;
    }
#ifdef FOT_TIMELINE
    uint64_t tl_rows = 0;
    int tl_chunks = (int)(my_rng & 0xffffu) - (int)(my_rng >> 16);
    for (int o = 32; o > 0; o >>= 1) tl_chunks += __shfl_xor(tl_chunks, o);
#endif
    // the rows of the group's profiles, all waves together
    {
        const double dt = head->dt, ego_x = head->ego_x, ego_y = head->ego_y;
        for (int i = sub * WAVE + lane; i < total_rows; i += GROUP_TILES * WAVE) {
            int p = 0;                                           // (row0 is total_rows from n_stage on; no read waits for another)
#pragma unroll
            for (int pp = 1; pp < GROUP_MAX_PROFILES; ++pp) p += i >= row0_tab[pp] ? 1 : 0;
            const int k = i - row0_tab[p];
            const LonInfo Lp = info_tab[p];
            LonSample ls;
            double sddd;
            make_lon_sample(sp_lds, Lp, k, dt, ls, sddd);        // (k == n_eval of a brake profile: its hold state)
            double *r = my_rows + (int64_t)i * ROW_FIELDS;
            r[0] = ls.sd; r[1] = ls.sdd; r[2] = ls.rx - ego_x; r[3] = ls.ry - ego_y;   // (instance-local: see evaluate_tile)
            r[4] = ls.cos_r; r[5] = ls.sin_r; r[6] = ls.kr; r[7] = ls.dkr; r[8] = ls.inv_sd;
        }
    }
    __syncthreads();
    if (n <= 0) return;                                          // (a padding tile, or one past a standing ego's lattice)
#ifdef FOT_TIMELINE
    const uint64_t t_wave = __builtin_amdgcn_s_memrealtime();
    const uint64_t c_wave = __builtin_amdgcn_s_memtime();
    const int tl_wave = inst_tile0 + tile;
#endif
    bool hit = false;
    // the steps before any candidate of the tile holds (ne_min of evaluate_segment; the general form has no scalar registers
    // to spare for that walk): every lane of the wave is here, the ones that walk the empty path do not count
    constexpr bool SREG = LEAN;
    const int ne_min = SREG ? wave_min_i32(has_cand ? L.n_eval : INT_MAX) : 0;
    if (walks) {
        // the walk's wave-uniform state is set up HERE: scalar values do not survive the join of the region above
        FusedSink<LEAN, W> sink;
        sink.Pp = Pp; sink.Dp = &D;
        sink.my_rng = my_rng;
        sink.my_thr = my_step.thr; sink.my_thr_sure = my_step.thr_sure; sink.thr = 0.0f; sink.thr_fatal = -1.0f;
        sink.my_thr_fatal = my_thr_fatal;
        sink.step_base = 0; sink.step_row = inst_tile0 + tile; sink.lane_id = lane;
        const int64_t ent_off = ((int64_t)uni(((const int32_t *)&head->ent_off)[1]) << 32) | (uint32_t)uni(((const int32_t *)&head->ent_off)[0]);
        sink.chunks = (const f2x8 *)(ent32 + ent_off);
        sink.chunks_per_k = ent_cap / ENT_CHUNK;
        sink.hit_mask = typename FusedSink<LEAN, W>::Mask(); sink.viol = 0; sink.hit = false; sink.n_chunks = 0; sink.c_lo = 0; sink.pf = 0;
        sink.no_warm = (a.ablate & 2) != 0;
        lc.n_circ_fp = 0;
        if constexpr (!LEAN) {                                   // (LEAN: the single centre circle, never read)
            lc.n_circ_fp = uni(head->n_circ_fp);
            asm volatile("" : "+s"(lc.n_circ_fp));
        }
        evaluate_segment<LEAN, SREG, FLAT>(P, lc, L, tab, q, 0, n_loop, sink, g, ne_min);
        hit = sink.hit;
#ifdef FOT_TIMELINE
        tl_rows = tab.t_rows;
#endif
    }
#ifdef FOT_TIMELINE
    const uint64_t t_loop_end = __builtin_amdgcn_s_memrealtime();
#endif
    tile_results(P, D, tab, L, q, g, hit, has_cand, slot, cand0, lane, tp);
#ifdef FOT_TIMELINE
    tl_rows = (uint64_t)__shfl((unsigned long long)tl_rows, 0);
    if (tl_wave < 16384 && lane == 0) {
        g_timeline[tl_wave * 4 + 0] = t_blk; g_timeline[tl_wave * 4 + 1] = t_wave;
        g_timeline[tl_wave * 4 + 2] = __builtin_amdgcn_s_memrealtime();
        g_timeline[tl_wave * 4 + 3] = (uint64_t)(uint32_t)tl_chunks | ((uint64_t)(uint32_t)tl_tag << 32);
        g_shader_clock[tl_wave * 2 + 0] = c_wave; g_shader_clock[tl_wave * 2 + 1] = __builtin_amdgcn_s_memtime();
        g_row_wait[tl_wave] = tl_rows;
        g_phase[tl_wave * 4 + 0] = s_tl_entry[0]; g_phase[tl_wave * 4 + 1] = s_tl_entry[1];
        g_phase[tl_wave * 4 + 2] = t_info; g_phase[tl_wave * 4 + 3] = t_loop_end;
    }
#endif
}

// ---------------------------------------------------------------------------
// selection + output (reference: frenet_planner.py:294-324, 1235-1259)
// ---------------------------------------------------------------------------

// One wave selects for one instance: stop-distance filter, rejection histogram, first-minimum arg-min (lowest index
// wins ties), the selected path rebuilt from its profile, the record written.  Run by the wave that finishes the
// instance's LAST tile (tile_done below) -- no separate launch behind the evaluation, and the selections of the
// instances that finish early overlap with the evaluation of the others.  A real function: its registers (final_sample
// holds an arc tangent) must not count against the time-step loop's.
__device__ __forceinline__ TilePart tile_part_empty()
{
    TilePart t;
    t.cost = INFINITY; t.idx = -1; t.keep = 0;
    for (int c = 0; c < 8; ++c) t.cnt[c] = 0;
    return t;
}

__device__ __forceinline__ void select_instance_wave(int inst, int lane)
{
    const EvalKernArgs &KA = eval_kernargs();
    const InstDesc &D = KA.desc[inst];
    const DevParams &P = KA.Pp[KA.mixed ? D.scen : 0];
    const InstState &S = KA.state[inst];
    fot_result &R = KA.out[inst];
    // The record's header starts out all zero, and so do the first n_total entries of its 15 path arrays wherever no
    // path sample lands (this wave alone writes the record: program order is enough).  Entries from n_total on are never
    // touched: the arrays' stride is FOT_MAX_NT whatever the planner's horizon, the work here is not.
    constexpr int HEADER_WORDS = (int)(offsetof(fot_result, t) / sizeof(unsigned long long));
    static_assert(offsetof(fot_result, t) % sizeof(unsigned long long) == 0, "the header is zeroed in 8-byte words");
    if (lane < HEADER_WORDS) ((unsigned long long *)&R)[lane] = 0ull;
    static_assert(HEADER_WORDS <= WAVE, "one word per lane");
    const auto zero_samples = [&](int k0) {                       // entries [k0, n_total) of every array
        for (int k = k0 + lane; k < P.n_total; k += WAVE)
#pragma unroll
            for (int f = 0; f < 15; ++f) R.t[f * FOT_MAX_NT + k] = 0.0;
    };
    if (!S.c2f_ok) {
        zero_samples(0);
        if (lane == 0) {
            R.status = FOT_PLAN_C2F_FAILED; R.best_index = -1; R.n_cand = 0; R.n_keep = 0;
            R.cost = INFINITY; R.stats_valid = 0;
            R.new_last_kappa = D.ego.last_kappa; R.new_prev_s = S.new_prev_s;
            for (int i = 0; i < 6; ++i) { R.frenet0[i] = NAN; R.ref0[i] = NAN; }
        }
        return;
    }
    // over the instance's tiles (lane = tile): histogram summed, first-minimum arg-min (lowest index wins ties)
    int cnt[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    ScanBest best = { INFINITY, -1 };
    int keep_l = 0;
    for (int t = lane; t < D.n_tiles; t += WAVE) {
        const TilePart *tpp = KA.parts + D.tile0 + t;
        const double c_t = ld_agent(&tpp->cost);
        const int i_t = ld_agent(&tpp->idx), k_t = ld_agent(&tpp->keep);
#pragma unroll
        for (int c = 0; c < 8; ++c) cnt[c] += ld_agent(&tpp->cnt[c]);
        const ScanBest o = { c_t, i_t };
        const int before = best.idx;
        scan_merge(best, o);
        if (best.idx != before) keep_l = k_t;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
        for (int off = 32; off >= 1; off >>= 1) cnt[c] += __shfl_xor(cnt[c], off, WAVE);
    {
        const int mine_idx = best.idx;
        best = wave_argmin(best);
        // the keep of the winning tile: held by the lane whose own best it is
        const unsigned long long who = __ballot(mine_idx == best.idx && best.idx >= 0);
        keep_l = who ? __shfl(keep_l, __ffsll((long long)who) - 1, WAVE) : 0;
    }
    if (lane == 0) {
        R.status = best.idx >= 0 ? FOT_PLAN_OK : FOT_PLAN_NO_PATH;
        R.best_index = best.idx;
        R.n_cand = S.n_cand;
        R.cost = best.idx >= 0 ? best.dist : INFINITY;
        for (int c = 0; c < 8; ++c) R.stats[c] = cnt[c];
        R.stats_valid = 1;
        R.new_prev_s = S.new_prev_s;
        for (int i = 0; i < 6; ++i) { R.frenet0[i] = S.frenet0[i]; R.ref0[i] = S.ref0[i]; }
    }
    if (best.idx < 0) {
        zero_samples(0);
        if (lane == 0) { R.n_keep = 0; R.new_last_kappa = D.ego.last_kappa; }
        return;
    }
    const int keep = keep_l;
    const CandDecode cd = decode_candidate(P, D, S.frenet0, best.idx);
    const LonInfo L = profile_info(P, D, S.frenet0, cd.lon_slot, false);
    ComputeTab tab;
    tab.sp = KA.mixed ? load_const(KA.sp_table, D.scen) : KA.sp; tab.L = L; tab.dt = P.dt;
    double q[6];
    lat_coeffs(S.frenet0, cd.di, cd.brake ? P.brake[cd.ti] : P.ti[cd.ti], q);
#ifndef FOT_SEL_NO_PATH
    for (int k = lane; k < keep; k += WAVE) {                              // (more than 64 samples: two rounds)
        double o[15];
        final_sample(P, L, tab, q, k, o);
        R.t[k] = o[0]; R.s[k] = o[1]; R.s_d[k] = o[2]; R.s_dd[k] = o[3]; R.s_ddd[k] = o[4];
        R.d[k] = o[5]; R.d_d[k] = o[6]; R.d_dd[k] = o[7]; R.d_ddd[k] = o[8];
        R.x[k] = o[9]; R.y[k] = o[10]; R.yaw[k] = o[11]; R.v[k] = o[12]; R.a[k] = o[13];
        R.c[k] = o[14];
        if (k == 1) R.new_last_kappa = o[14];                              // frenet_planner.py:301-302
    }
#endif
    zero_samples(keep);
    if (lane == 0) {
        R.n_keep = keep;
        if (keep <= 1) R.new_last_kappa = D.ego.last_kappa;
    }
}

// The record of `inst` is complete: tell a host that polls for it (a synchronous small call, fot_host.cpp wait_records).
// The release is at system scope -- the record lies in pinned host memory --, the flag follows it.
__device__ __forceinline__ void record_written(int inst, int lane)
{
    const EvalKernArgs &KA = eval_kernargs();
    if (!KA.done_flag) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (lane == 0) __hip_atomic_store(KA.done_flag + inst, KA.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A wave is done with tile `tile` of instance `inst`: it leaves what it found (tp; empty for a tile without candidates)
// and counts itself.  Every tile of the instance arrives exactly once; the wave that completes the count selects.
// k_frenet_state zeroes the counters.  The partial results travel as agent-coherent stores / loads (st_agent,
// ld_agent): once this wave's stores are acknowledged (vmcnt) they are visible to every CU, so the count needs no fence.
__device__ __forceinline__ void tile_done(int inst, int tile, int lane, const TilePart &tp)
{
    const EvalKernArgs &KA = eval_kernargs();
    if (lane == 0) {
        TilePart *dst = KA.parts + KA.desc[inst].tile0 + tile;
        st_agent(&dst->cost, tp.cost); st_agent(&dst->idx, tp.idx); st_agent(&dst->keep, tp.keep);
#pragma unroll
        for (int c = 0; c < 8; ++c) st_agent(&dst->cnt[c], tp.cnt[c]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // this wave's stores, before the count
    int last = 0;
    // (-DFOT_SAFE_SELECT: the textbook form -- an acquire-release count at agent scope, i.e. an L2 write-back before and
    //  an invalidate behind it in EVERY wave: +45 % on the launch when measured; the shipped form relies on the sc1
    //  stores / loads above and below, which scripts/isa_check_async.py verifies in the ISA of every build)
#ifdef FOT_SAFE_SELECT
    constexpr int COUNT_ORDER = __ATOMIC_ACQ_REL;
#else
    constexpr int COUNT_ORDER = __ATOMIC_RELAXED;
#endif
    if (lane == 0)
        last = __hip_atomic_fetch_add(&KA.inst_done[inst], 1, COUNT_ORDER, __HIP_MEMORY_SCOPE_AGENT)
               == KA.desc[inst].n_tiles - 1 ? 1 : 0;
    last = __builtin_amdgcn_readfirstlane(last);
    asm volatile("" ::: "memory");                                // no load of the partials may be hoisted above the count
    if (!last) return;
    select_instance_wave(inst, lane);
    record_written(inst, lane);
}

// the degenerate launch: a batch without a single tile (no horizons, no brake ladder) still gets its records
__global__ void __launch_bounds__(WAVE)
k_select_only(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, const InstState *__restrict__ state,
              const int32_t *__restrict__ tile_cand0, const int32_t *__restrict__ tile_n,
              const TileStep *__restrict__ wave_rng, const f2 *__restrict__ ent32, const EvalKernArgs a)
{
    if ((int)blockIdx.x < a.n_inst) {
        select_instance_wave((int)blockIdx.x, (int)threadIdx.x);
        record_written((int)blockIdx.x, (int)threadIdx.x);
    }
}

#define FOT_EVAL_WORDS 1
#define FOT_EVAL_LEAN false
#define FOT_EVAL_FLAT false
#define FOT_EVAL_KERNEL(name) name
#include "fot_eval_kernels.inc"
#undef FOT_EVAL_LEAN
#undef FOT_EVAL_KERNEL
#define FOT_EVAL_LEAN true
#define FOT_EVAL_KERNEL(name) name##_lean
#include "fot_eval_kernels.inc"
#undef FOT_EVAL_FLAT
#undef FOT_EVAL_KERNEL
// the flat forms of the lean kernels: every path of the launch is exactly straight (TileTable::flat, enqueue_lane)
#define FOT_EVAL_FLAT true
#define FOT_EVAL_KERNEL(name) name##_lean_flat
#include "fot_eval_kernels.inc"
#undef FOT_EVAL_LEAN
#undef FOT_EVAL_FLAT
#undef FOT_EVAL_KERNEL
#undef FOT_EVAL_WORDS
// the wide forms (FusedSink<., WIDE_MASK_WORDS>): a launch with an instance of more than FOT_MAX_SAMPLES samples, on a
// handle whose sample capacity was raised (TileTable::wide, enqueue_lane).  No flat form.
#define FOT_EVAL_WORDS WIDE_MASK_WORDS
#define FOT_EVAL_FLAT false
#define FOT_EVAL_LEAN false
#define FOT_EVAL_KERNEL(name) name##_wide
// (the diagnostic -DFOT_TIMELINE build keeps its time stamps in registers beside the four mask words: k_evaluate_group_wide
//  then does not fit the 128 registers of four waves per SIMD without scratch, and runs three -- that build only)
#if defined(FOT_TIMELINE) && FOT_GROUP_WAVES > 3
#define FOT_EVAL_GROUP_WAVES 3
#endif
#include "fot_eval_kernels.inc"
#undef FOT_EVAL_LEAN
#undef FOT_EVAL_KERNEL
#define FOT_EVAL_LEAN true
#define FOT_EVAL_KERNEL(name) name##_lean_wide
#include "fot_eval_kernels.inc"
#undef FOT_EVAL_LEAN
#undef FOT_EVAL_FLAT
#undef FOT_EVAL_KERNEL
#undef FOT_EVAL_WORDS

// ---------------------------------------------------------------------------
// collision broad phase: entry lists
// ---------------------------------------------------------------------------

// One workgroup of CULL_KG waves per (instance, group of CULL_KG consecutive time steps); wave w owns step k0 + w.  The caller's prediction tensor is
// [S][P][T][2]: the T samples of one pedestrian are contiguous, so a lane that takes obstacle (s, p) reads its
// CULL_KG consecutive samples as one contiguous run -- every fetched sector is used -- and classifies it against the
// boxes of the group's time steps.  Entries of step k: the static obstacles and the dynamic obstacles of time row
// min(k, T-1) that lie inside the candidates' bounding box of k (merged over the instance's longitudinal profiles)
// grown by the collision radius, ordered by bin along the longer side of the box (counting sort through LDS
// atomics), FAR32-padded to chunk pairs.  Then, per tile of the instance (k_evaluate's unit of work), the chunk range
// its own profiles' boxes can reach (strip_range) -- the only thing k_evaluate reads per time step.
// Groups of FOUR steps: 62.4 us solo against 61.4 with eight (the step-independent solves are repeated by twice as many
// workgroups), but a 256-thread workgroup with 16 KB of LDS finds room beside the evaluation's workgroups where a
// 512-thread one with 29 KB does not -- the step with four plan calls in flight is 1.5 % shorter (scripts/ab_kg.sh;
// sixteen steps: 79 us, two: 77 us).
#ifndef FOT_CULL_KG
#define FOT_CULL_KG 4
#endif
constexpr int CULL_KG = FOT_CULL_KG;    // time steps (= waves) of a group in k_cull
constexpr int CULL_LIST = 256;          // kept obstacles per time step remembered between the two passes
constexpr int CULL_PBOX = 96;           // profiles per instance whose boxes are kept in LDS (more: recomputed)
constexpr uint32_t CULL_IDX_MASK = 0xFFFFFu;   // obstacle index (< 2^20, fot_setup.hpp) | bin << 20
constexpr int CULL_VER = 256;           // pedestrian tracks a group checks for NaN (the ones inside its boxes), [S][P][T] layout
constexpr int CULL_BAD = 32;            // ... and tracks found to hold one, remembered by the group
constexpr uint32_t CULL_DEAD = 0xFFFFFFFFu;    // a remembered obstacle that turned out to be such a track

// One group: KG waves, the KG consecutive time steps from k0 of instance `inst`.  `sp`: the reference path as the caller
// staged it; `dyn_lds`: (n_ti + n_brake) * (KG * 2 + 9) doubles of dynamic LDS (launch_cull).
template <typename T, int KG>
__device__ __forceinline__ void
cull_group(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, const InstState *__restrict__ state,
           const SplineView &sp, double *dyn_lds, const T *__restrict__ static_xy, const T *__restrict__ dyn_xy,
           int32_t *__restrict__ ent_cnt, f2 *__restrict__ ent32, d2 *__restrict__ ent64, uint8_t *__restrict__ ent_sid,
           TileStep *__restrict__ wave_rng, const int32_t *__restrict__ tile_cand0, const int32_t *__restrict__ tile_n,
           const int32_t *__restrict__ tile_span, const uint8_t *__restrict__ nan_flag, int ablate, int inst, int k0)
{
    __shared__ int s_cnt[KG][CULL_BINS + 1];                // pass 1: entries per bin; pass 2: write cursors
    __shared__ int s_start[KG][CULL_BINS + 1];
    __shared__ int s_nin[KG];
    __shared__ uint32_t s_list[KG][CULL_LIST];              // kept obstacles of each step: index | bin << 20
    __shared__ uint32_t s_ver[CULL_VER];                    // (lazy NaN check) tracks inside some box of the group
    __shared__ uint32_t s_bad[CULL_BAD];                    // ... those that hold a NaN
    __shared__ int s_nver, s_nbad;
    __shared__ Box32 s_box[KG];                             // per-step constants
    __shared__ BinMap s_bm[KG];
    __shared__ float s_margin[KG];
    __shared__ Box32 s_pbox[KG][CULL_PBOX];                 // boxes of the instance's profiles at the group's steps
    // what the boxes need of the instance that does not depend on the step, solved once per workgroup: the quartic of
    // every profile (and its horizon's index), the quintics of the two extreme lateral targets of every horizon
    __shared__ LonQuartic s_linfo[CULL_PBOX];
    __shared__ uint8_t s_lext[CULL_PBOX];
    const DevParams &P = *Pp;
    // dynamic LDS, sized by the planner's horizons (launch_cull): the lateral extent per horizon / brake-ladder entry
    // and step, and the two extreme lateral quintics of every horizon
    const int n_ext_cap = P.n_ti + P.n_brake;
    double *s_ext = dyn_lds;                                     // [KG][n_ext_cap][2]
    double *s_latq = s_ext + KG * n_ext_cap * 2;                 // [n_ext_cap][9]
    const InstDesc &D = desc[inst];
    const InstState &S = state[inst];
    if (D.ent_cap == 0) return;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);   // this wave's time step inside the group
    const int nk = P.n_total - k0 < KG ? P.n_total - k0 : KG;
    const int n_grid_lon = P.n_ti * D.n_tv;
    const int n_prof = S.c2f_ok ? n_grid_lon + S.n_brake : 0;
    const double sq_dyn = D.dyn_mode == FOT_DYN_SINGLE ? P.sq_r_dyn : P.sq_r;
    const double sq_max = sq_dyn > P.sq_r ? sq_dyn : P.sq_r;
    const FilterConst fc = filter_const(sq_max, sq_dyn < P.sq_r ? sq_dyn : P.sq_r);
    const float slack = box_footprint_slack(P);
    const int n_ext = P.n_ti + (S.c2f_ok ? S.n_brake : 0);
    for (int w = tid; w < n_prof && w < CULL_PBOX; w += KG * WAVE) {
        s_linfo[w] = lon_quartic(profile_info(P, D, S.frenet0, w, false));
        s_lext[w] = (uint8_t)extent_index(P, D, w);
    }
    if (S.c2f_ok && tid < n_ext) {                               // (n_ext <= FOT_MAX_TI + FOT_MAX_BRAKE < the workgroup)
        const bool brake = tid >= P.n_ti;
        lateral_extent_coeffs(P, S.frenet0, brake, brake ? P.brake[tid - P.n_ti] : P.ti[tid], s_latq + tid * 9);
    }
    __syncthreads();
    if (ablate & 16) return;                                     // (timing diagnostics: launch + per-instance constants)

    struct Raw { T x, y; };                                       // as stored: widened only when it is classified
    const bool dyn_on = D.dyn_mode != FOT_DYN_NONE;
    const int n_dyn = dyn_on ? D.S * D.P : 0;
    const int total = D.n_static + n_dyn;
    const bool tmajor = D.dyn_tmajor != 0;                       // [T][S][P][2] instead of the caller's [S][P][T][2]
    // The instance's prediction tensor is a wave-uniform base plus per-lane byte offsets, and these fit 32 bits unless
    // the tensor reaches 2 GiB (2^20 obstacles x 128 steps of float64 do): an address is then one 32-bit add and a
    // load with a scalar base, not 64-bit multiply-adds and selects.  Larger tensors keep the 64-bit forms.
    const char *dyn_base = (const char *)(dyn_xy + 2 * D.dyn_off);
    const bool off32 = offsets_fit32((int64_t)n_dyn * D.T * (int64_t)sizeof(Raw));
    auto dyn_offset = [&](int j, int row) {                      // (off32) byte offset of track j's sample at `row`
        return (uint32_t)(tmajor ? row * n_dyn + j : j * D.T + row) * (uint32_t)sizeof(Raw);
    };

    // Pass-1 lane roles.  Caller layout: lane = (obstacle slot, step) -- the KG lanes of one obstacle read its KG
    // consecutive samples, a contiguous run of the [S][P][T][2] tensor (32 bytes at KG = 4, float32), so a wave-wide load touches 64 / KG such runs
    // instead of 64 scattered cache lines; the group's 8 waves share the obstacles.  T-major layout: the obstacles of
    // one time row are contiguous, so wave w takes step k0 + w alone and its lanes read 64 consecutive obstacles.
    const int kl = tmajor ? wv : (lane & (KG - 1));          // this lane's step inside the group
    const int i_first = tmajor ? lane : wv * (WAVE / KG) + lane / KG;
    constexpr int STRIDE = WAVE;                                  // obstacles between two of a lane's loads
    const int row_l = k0 + kl < D.T - 1 ? k0 + kl : D.T - 1;
    // Branch-free: an index past the end is clamped (classify() ignores its value) and static / dynamic is a select
    // between two addresses, so the UNROLL loads of a lane are issued back to back -- behind a branch each one would
    // wait for the one before it, one gather in flight per lane, and the pass would crawl along at memory latency.
    auto fetch = [&](int i, Raw &o) {
        const int ic = i < total ? i : total - 1;                 // (total > 0 inside the loop)
        const int j = ic - D.n_static;                            // = s * P + p when dynamic
        const T *ps = static_xy + 2 * ((int64_t)D.static_off + ic);
        const T *pd = off32 ? (const T *)(dyn_base + dyn_offset(j, row_l))     // (a static index: not dereferenced)
                            : dyn_xy + 2 * (D.dyn_off + (tmajor ? (int64_t)row_l * n_dyn + j : (int64_t)j * D.T + row_l));
        const Raw *src = (const Raw *)(ic < D.n_static ? ps : pd);
        o = *src;
    };
    // Boxes of the group's time steps over all longitudinal profiles of the instance.  The (step, horizon) lateral
    // extents and then the (step, profile) boxes are spread over ALL threads of the workgroup -- full waves of float64
    // work instead of waves with a third of their lanes busy --, then wave wv merges the boxes of step k0 + wv.
    if (!(ablate & 8)) {
        for (int i = tid; i < nk * n_ext; i += KG * WAVE) {
            const int ks = small_quotient(i, n_ext, KG), e = i - ks * n_ext;   // (i < nk * n_ext: no division)
            const bool brake = e >= P.n_ti;
            const int n_eval = brake ? P.brake[e - P.n_ti].n_t : P.ti[e].n_t;
            double *ext = s_ext + (ks * n_ext_cap + e) * 2;
            lateral_extent_q(s_latq + e * 9, brake, k0 + ks, n_eval, P.dt, ext[0], ext[1]);
        }
        __syncthreads();
        const int n_tab = n_prof < CULL_PBOX ? n_prof : CULL_PBOX;
        const float sp_scale = spline_guess_scale(sp);           // (segment lookups start from a guess: fot_math.hpp)
        for (int i = tid; i < nk * n_tab; i += KG * WAVE) {
            const int ks = small_quotient(i, n_tab, KG), w = i - ks * n_tab;
            const double *ext = s_ext + (ks * n_ext_cap + s_lext[w]) * 2;
            s_pbox[ks][w] = profile_box_from_guess(s_linfo[w], D, sp, sp_scale, k0 + ks, P.dt, ext[0], ext[1]);   // read again below, per tile
        }
        __syncthreads();
    }
    {
        Box32 bw = box_empty();
        if (wv < nk && !(ablate & 8)) {
            for (int w = lane; w < n_prof; w += WAVE) {
                if (w < CULL_PBOX) {
                    box_merge(bw, s_pbox[wv][w]);
                } else {                                            // (more profiles than the table holds: on the spot)
                    const double *ext = s_ext + (wv * n_ext_cap + extent_index(P, D, w)) * 2;
                    box_merge(bw, profile_box_at(P, D, S.frenet0, sp, w, k0 + wv, ext[0], ext[1]));
                }
            }
        }
        bw.x0 = wave_min_nonan_f32(bw.x0); bw.y0 = wave_min_nonan_f32(bw.y0);   // (segment_box skips NaN points)
        bw.x1 = wave_max_nonan_f32(bw.x1); bw.y1 = wave_max_nonan_f32(bw.y1);
        const float mw = cull_margin(sq_max, bw) + slack;
        if (lane == 0) { s_box[wv] = bw; s_margin[wv] = mw; s_bm[wv] = bin_map(bw, mw); s_nin[wv] = 0; }
        if (lane <= CULL_BINS) s_cnt[wv][lane] = 0;
        if (tid == 0) { s_nver = 0; s_nbad = 0; }
    }
    __syncthreads();

    // Which pedestrian tracks hold a NaN (NanScan, fot_kernels.h).  Time-major tensors: the flags k_frenet_state's scan
    // blocks left.  The caller's [S][P][T][2] layout: LAZILY, here -- only a track that lies inside some box of the group
    // can become an entry, its T samples are one contiguous run (408 bytes at T = 51: one wave-wide load) and the group's
    // first pass has the KG lanes of a track side by side, so the group collects the few dozen tracks its boxes touch
    // (s_ver), its waves share them out and look through them, and nobody reads the tensor a second time just to find
    // NaNs: the whole tensor crosses HBM once per plan call instead of twice.  (Every wave looking through its OWN
    // tracks right behind its gathers, one barrier less, was 8 us slower: the slowest wave sets the pace.)
    const bool lazy = dyn_on && !tmajor && !(ablate & 128);       // (128: NanScan::eager, the flags are there)
    const Raw *tracks = (const Raw *)(dyn_xy + 2 * D.dyn_off);   // [n_dyn][T] in the caller's layout
    auto track_has_nan = [&](int j) {                            // one lane on its own (the paths that did not fit)
        bool bad = false;
#pragma clang loop vectorize(disable) unroll(disable)
        for (int t = 0; t < D.T; ++t) { const Raw p = tracks[(int64_t)j * D.T + t]; bad |= (p.x != p.x) | (p.y != p.y); }
        return bad;
    };
    auto track_bad = [&](int i) {                                // obstacle i, by whatever this instance's layout offers
        if (i < D.n_static) return false;
        return lazy ? track_has_nan(i - D.n_static) : nan_flag[D.nan_off + (i - D.n_static)] != 0;
    };

    // pass 1: histogram per step, kept obstacles remembered
    {
        const Box32 bl = s_box[kl];
        const float ml = s_margin[kl];
        const BinMap bml = s_bm[kl];
        const bool live_l = kl < nk && bl.x0 <= bl.x1 && !(ablate & 4);
        auto classify = [&](int i, const Raw &o) {
            const float fx = (float)((double)o.x - D.ego.x), fy = (float)((double)o.y - D.ego.y);
            const bool in = i < total && live_l && cull_inside(bl, ml, fx, fy);
            if (lazy) {
                // remembered, not yet counted: its track is looked through first.  The KG lanes of an obstacle are
                // neighbours (lane & (KG - 1) = step): the first of them enters the track once for the whole group
                // (which lanes those are is worked out on the scalar side from the ballot and handed back as a lane
                // mask: no lane arithmetic per gather)
                uint64_t m = __builtin_amdgcn_ballot_w64(in && i >= D.n_static);
#pragma unroll
                for (int s = 1; s < KG; s <<= 1) m |= m >> s;              // bit l: some lane of l .. l + KG - 1 is in
                constexpr uint64_t FIRST = ~0ull / ((1ull << KG) - 1ull);  // the first lane of every group of KG
                if (__builtin_amdgcn_inverse_ballot_w64(m & FIRST)) {
                    const int v = atomicAdd(&s_nver, 1);
                    if (v < CULL_VER) s_ver[v] = (uint32_t)i;
                }
                if (in) {
                    const int j = atomicAdd(&s_nin[kl], 1);
                    if (j < CULL_LIST) s_list[kl][j] = (uint32_t)i | ((uint32_t)bin_of(bml, fx, fy) << 20);
                }
                return;
            }
            if (in) {
                // a pedestrian whose track holds a NaN anywhere is no obstacle at any step (NanScan; asked for the few
                // obstacles inside the box only)
                if (i >= D.n_static && nan_flag[D.nan_off + (i - D.n_static)]) return;
                const int bin = bin_of(bml, fx, fy);
                atomicAdd(&s_cnt[kl][bin], 1);
                const int j = atomicAdd(&s_nin[kl], 1);
                if (j < CULL_LIST) s_list[kl][j] = (uint32_t)i | ((uint32_t)bin << 20);
            }
        };
#ifndef FOT_CULL_UNROLL
#define FOT_CULL_UNROLL 4
#endif
        constexpr int UNROLL = FOT_CULL_UNROLL;                   // gathers in flight per lane
        if (ablate & 64) {                                        // (timing diagnostics: no gathers)
        } else if (D.n_static == 0 && off32) {
            // only the prediction tensor (the usual case): a lane's obstacles are a fixed number of bytes apart, so the
            // offset runs along, one add per gather.  Past the end it is clamped to the tensor's last point (ignored),
            // which also keeps a wrapped offset inside the tensor: every multiple of the point size below is.
            const uint32_t step = (uint32_t)(tmajor ? STRIDE : STRIDE * D.T) * (uint32_t)sizeof(Raw);
            const uint32_t o_last = (uint32_t)((int64_t)n_dyn * D.T * (int64_t)sizeof(Raw)) - (uint32_t)sizeof(Raw);
            uint32_t off = dyn_offset(i_first, row_l);
            for (int ib = i_first; ib < total; ib += UNROLL * STRIDE) {
                Raw o[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const uint32_t ou = off + (uint32_t)u * step;
                    o[u] = *(const Raw *)(dyn_base + (ou < o_last ? ou : o_last));
                }
                off += (uint32_t)UNROLL * step;
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) classify(ib + u * STRIDE, o[u]);
            }
        } else if (D.n_static == 0) {
            // only the prediction tensor (the usual case): a lane's obstacles are a fixed number of bytes apart, so the
            // address is a running pointer instead of two 64-bit multiply-adds and a select per gather
            const char *p0 = (const char *)(dyn_xy + 2 * (D.dyn_off + (tmajor ? (int64_t)row_l * n_dyn + i_first
                                                                              : (int64_t)i_first * D.T + row_l)));
            const int64_t step = (int64_t)(tmajor ? STRIDE : STRIDE * D.T) * (int64_t)(2 * sizeof(T));
            const char *p = p0;
            for (int ib = i_first; ib < total; ib += UNROLL * STRIDE) {
                Raw o[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {                // (past the end: the lane's first obstacle again, ignored)
                    o[u] = *(const Raw *)(ib + u * STRIDE < total ? p : p0);
                    p += step;
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) classify(ib + u * STRIDE, o[u]);
            }
        } else {
            for (int ib = i_first; ib < total; ib += UNROLL * STRIDE) {
                Raw o[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) fetch(ib + u * STRIDE, o[u]);
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) classify(ib + u * STRIDE, o[u]);
            }
        }
    }
    __syncthreads();
    if (lazy) {
        // the tracks inside the group's boxes, one wave-wide load each (lane = sample), VU of them in flight per wave
#ifndef FOT_CULL_VU
#define FOT_CULL_VU 4
#endif
        constexpr int VU = FOT_CULL_VU;
        const int n_ver = s_nver < CULL_VER ? s_nver : CULL_VER;
        for (int v0 = wv; v0 < n_ver; v0 += VU * KG) {
            Raw p[VU];
#pragma unroll
            for (int u = 0; u < VU; ++u) {
                const int v = v0 + u * KG < n_ver ? v0 + u * KG : v0;
                const int j = (int)s_ver[v] - D.n_static, t = lane < D.T ? lane : D.T - 1;
                p[u] = off32 ? *(const Raw *)(dyn_base + (uint32_t)(j * D.T + t) * (uint32_t)sizeof(Raw))
                             : tracks[(int64_t)j * D.T + t];
            }
#pragma unroll
            for (int u = 0; u < VU; ++u) {
                const int v = v0 + u * KG;
                if (v >= n_ver) break;
                bool bad = (p[u].x != p[u].x) | (p[u].y != p[u].y);
                for (int t = WAVE + lane; t < D.T; t += WAVE) {   // (more than 64 samples per track)
                    const Raw q = tracks[(int64_t)((int)s_ver[v] - D.n_static) * D.T + t];
                    bad |= (q.x != q.x) | (q.y != q.y);
                }
                if (__ballot(bad) != 0ull && lane == 0) {
                    const int nb = atomicAdd(&s_nbad, 1);
                    if (nb < CULL_BAD) s_bad[nb] = s_ver[v];
                }
            }
        }
        __syncthreads();
    }
    // wave wv: everything else of time step k0 + wv
    if (wv >= nk) return;
    const int kk = wv, k = k0 + wv;
    // lazy: did everything fit (the remembered obstacles of this step, the group's tracks, the NaN tracks among them)?
    const bool listed = !lazy || (s_nin[kk] <= CULL_LIST && s_nver <= CULL_VER && s_nbad <= CULL_BAD);
    const Box32 bk = s_box[kk];
    const BinMap bmk = s_bm[kk];
    const float mk = s_margin[kk];
    const bool live_k = bk.x0 <= bk.x1;
    const int row = k < D.T - 1 ? k : D.T - 1;
    auto point = [&](int i, d2 &o, int &sid) {                                      // obstacle i at step k
        sid = SID_STATIC;
        if (i < D.n_static) {
            const int64_t in = D.static_off + i;
            o.x = (double)static_xy[2 * in]; o.y = (double)static_xy[2 * in + 1];
        } else {
            const int j = i - D.n_static;
            if (off32) {
                const Raw r = *(const Raw *)(dyn_base + dyn_offset(j, row));
                o.x = (double)r.x; o.y = (double)r.y;
            } else {
                const int64_t in = D.dyn_off + (tmajor ? (int64_t)row * n_dyn + j : (int64_t)j * D.T + row);
                o.x = (double)dyn_xy[2 * in]; o.y = (double)dyn_xy[2 * in + 1];
            }
            sid = (int)div_by_magic((uint32_t)j, (uint32_t)D.P, D.p_magic);   // = j / D.P
        }
    };
    if (lazy) {
        // the histogram of this step, now that the NaN tracks are known: over the remembered obstacles, or -- something
        // did not fit -- over the whole row again, every kept track looked through by its own lane
        if (listed) {
            const int n_bad = s_nbad;
            for (int j = lane; j < s_nin[kk]; j += WAVE) {
                const uint32_t e = s_list[kk][j];
                bool bad = false;
                // (n_bad is 0 nearly always: as a vectorised loop its set-up alone cost every wave dozens of instructions)
#pragma clang loop vectorize(disable) unroll(disable)
                for (int b = 0; b < n_bad; ++b) bad |= s_bad[b] == (e & CULL_IDX_MASK);
                if (bad) s_list[kk][j] = CULL_DEAD;
                else atomicAdd(&s_cnt[kk][e >> 20], 1);
            }
        } else {
            for (int i0 = 0; i0 < total; i0 += WAVE) {
                const int i = i0 + lane;
                if (i >= total) continue;
                d2 o; int sid;
                point(i, o, sid);
                const float fx = (float)(o.x - D.ego.x), fy = (float)(o.y - D.ego.y);
                if (live_k && cull_inside(bk, mk, fx, fy) && !track_bad(i)) atomicAdd(&s_cnt[kk][bin_of(bmk, fx, fy)], 1);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    {   // exclusive prefix over the bins (lane = bin; entry CULL_BINS ends with the total); cursors = starts
        const int c = lane < CULL_BINS ? s_cnt[kk][lane] : 0;
        const int incl = wave_prefix_sum_i32(c);
        if (lane <= CULL_BINS) { s_start[kk][lane] = incl - c; s_cnt[kk][lane] = incl - c; }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");       // this wave's LDS writes (other lanes') before the reads below
    __builtin_amdgcn_wave_barrier();
    const int64_t base = D.ent_off + (int64_t)k * D.ent_cap;
    TileStep *rng = wave_rng + (int64_t)D.tile0 * P.n_total + k;                   // + tile * n_total
    const int count = s_start[kk][CULL_BINS];
    // pass 2: scatter into the list (order inside a bin is irrelevant)
    if (lazy ? listed : count <= CULL_LIST) {                    // straight from the remembered indices
        for (int j = lane; j < ((ablate & 2) ? 0 : (lazy ? s_nin[kk] : count)); j += WAVE) {
            const uint32_t e = s_list[kk][j];
            if (e == CULL_DEAD) continue;
            const int i = (int)(e & CULL_IDX_MASK), bin = (int)(e >> 20);
            d2 o; int sid;
            point(i, o, sid);
            const int pos = atomicAdd(&s_cnt[kk][bin], 1);
            ent32_store(ent32, base + pos, (float)(o.x - D.ego.x), (float)(o.y - D.ego.y));
            ent64[base + pos] = o;
            ent_sid[base + pos] = (uint8_t)sid;
        }
    } else {                                                     // more kept than remembered: classify the row again
        for (int i0 = 0; i0 < total; i0 += WAVE) {
            const int i = i0 + lane;
            if (i >= total) continue;
            d2 o; int sid;
            point(i, o, sid);
            const float fx = (float)(o.x - D.ego.x), fy = (float)(o.y - D.ego.y);
            if (live_k && cull_inside(bk, mk, fx, fy) && !track_bad(i)) {
                const int bin = bin_of(bmk, fx, fy);
                const int pos = atomicAdd(&s_cnt[kk][bin], 1);
                ent32_store(ent32, base + pos, fx, fy);
                ent64[base + pos] = o;
                ent_sid[base + pos] = (uint8_t)sid;
            }
        }
    }
    const int padded = (count + 2 * ENT_CHUNK - 1) & ~(2 * ENT_CHUNK - 1);        // whole chunk pairs (k_evaluate)
    if (lane < padded - count) {
        d2 o; o.x = INFINITY; o.y = INFINITY;
        ent32_store(ent32, base + count + lane, FAR32, FAR32);
        ent64[base + count + lane] = o;
        ent_sid[base + count + lane] = SID_STATIC;
    }
    if (lane == 0) ent_cnt[(int64_t)inst * P.n_total + k] = padded;
    // chunk range of every tile of the instance
    for (int w = lane; w < D.n_tiles; w += WAVE) {
        TileStep r = { 0u, 0.0f, 0.0f, 0u };
        const int idx0 = tile_cand0[D.shape_off + w];
        if (live_k && idx0 < S.n_cand && tile_n[D.shape_off + w] > 0 && !(ablate & 1)) {   // (not a padding tile)
            // its profiles, from the table (a standing ego has no brake ladder: the span ends with its last profile)
            const uint32_t sp01 = (uint32_t)tile_span[D.shape_off + w];
            const int s0 = (int)(sp01 >> 16), s1 = (int)(sp01 & 0xffffu) < n_prof - 1 ? (int)(sp01 & 0xffffu) : n_prof - 1;
            Box32 wb = box_empty();
            for (int sl = s0; sl <= s1; ++sl) {
                if (sl < CULL_PBOX) { box_merge(wb, s_pbox[kk][sl]); continue; }
                const double *ext = s_ext + (kk * n_ext_cap + extent_index(P, D, sl)) * 2;
                box_merge(wb, profile_box_at(P, D, S.frenet0, sp, sl, k, ext[0], ext[1]));
            }
            const float wm = cull_margin(sq_max, wb) + slack;
            r.rng = strip_range(bmk, wb, wm, [&](int bb) { return s_start[kk][bb]; });
            box_thresholds(fc, wb, wm, r.thr, r.thr_sure);
        }
        rng[(int64_t)w * P.n_total] = r;
    }
}

// One workgroup of CULL_KG waves per (instance, group of CULL_KG consecutive time steps).
template <typename T>
__global__ void __launch_bounds__(CULL_KG * WAVE)
k_cull(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, const InstState *__restrict__ state,
       int n_inst, SplineView sp_hbm, const SplineView *__restrict__ sp_table, int mixed, int lds_knots,
       const T *__restrict__ static_xy, const T *__restrict__ dyn_xy,
       int32_t *__restrict__ ent_cnt, f2 *__restrict__ ent32, d2 *__restrict__ ent64, uint8_t *__restrict__ ent_sid,
       TileStep *__restrict__ wave_rng, const int32_t *__restrict__ tile_cand0, const int32_t *__restrict__ tile_n,
       const int32_t *__restrict__ tile_span, const uint8_t *__restrict__ nan_flag,
       int ablate)
{
    if (ablate & 32) return;                                     // (timing diagnostics: the launch alone)
    const int groups = (Pp->n_total + CULL_KG - 1) / CULL_KG;   // (n_total: one time grid for every scenario)
    // workgroups go round-robin over the 8 XCDs: all groups of instance i run back to back on XCD i mod 8, so the
    // runs that neighbouring groups cut out of the same cache lines of the prediction tensor meet in one L2
    const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
    const int inst = xcd + 8 * (seq / groups), k0 = (seq % groups) * CULL_KG;
    if (inst >= n_inst) return;                                  // (the whole workgroup)
    if (mixed) { Pp += desc[inst].scen; sp_hbm = load_const(sp_table, desc[inst].scen); }
    const SplineView sp = stage_spline(sp_hbm, lds_knots);      // every wave, before any of them leaves
    cull_group<T, CULL_KG>(Pp, desc, state, sp, s_spl + 9 * lds_knots, static_xy, dyn_xy, ent_cnt, ent32, ent64, ent_sid,
                           wave_rng, tile_cand0, tile_n, tile_span, nan_flag, ablate, inst, k0);
}

// ---------------------------------------------------------------------------
// one candidate's full (untruncated) arrays, for fot_debug_candidate_path
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(WAVE)
k_debug_path(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, const InstState *__restrict__ state,
             SplineView sp, int inst, int idx,
             double *__restrict__ out /* [15][FOT_MAX_NT] */, int32_t *__restrict__ meta /* n_t, valid */)
{
    const DevParams &P = *Pp;
    const InstDesc &D = desc[inst];
    const InstState &S = state[inst];
    const int lane = threadIdx.x;
    if (!S.c2f_ok || idx < 0 || idx >= S.n_cand) { if (lane == 0) { meta[0] = 0; meta[1] = 0; } return; }
    const CandDecode cd = decode_candidate(P, D, S.frenet0, idx);
    const LonInfo L = profile_info(P, D, S.frenet0, cd.lon_slot, false);
    ComputeTab tab;
    tab.sp = sp; tab.L = L; tab.dt = P.dt;
    double q[6];
    lat_coeffs(S.frenet0, cd.di, cd.brake ? P.brake[cd.ti] : P.ti[cd.ti], q);
    for (int k = lane; k < L.n_t; k += WAVE) {
        double o[15];
        final_sample(P, L, tab, q, k, o);
        for (int f = 0; f < 15; ++f) out[f * FOT_MAX_NT + k] = o[f];
    }
    if (lane == 0) { meta[0] = L.n_t; meta[1] = 1; }
}

// ---------------------------------------------------------------------------
// epsilon-band report of one instance of the last plan call (fot_debug_margins): one thread per candidate
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(WAVE)
k_debug_margins(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, const InstState *__restrict__ state,
                SplineView sp, int inst, const int32_t *__restrict__ ent_cnt, const d2 *__restrict__ ent64,
                const uint8_t *__restrict__ ent_sid, int cap, double *__restrict__ out /* [cap][MARGIN_CATS] */)
{
    const DevParams &P = *Pp;
    const InstDesc &D = desc[inst];
    const InstState &S = state[inst];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (!S.c2f_ok || idx >= S.n_cand || idx >= cap) return;
    const CandDecode cd = decode_candidate(P, D, S.frenet0, idx);
    const LonInfo L = profile_info(P, D, S.frenet0, cd.lon_slot, false);
    ComputeTab tab;
    tab.sp = sp; tab.L = L; tab.dt = P.dt;
    double q[6];
    lat_coeffs(S.frenet0, cd.di, cd.brake ? P.brake[cd.ti] : P.ti[cd.ti], q);
    MarginEntries ent;
    ent.cnt = D.ent_cap != 0 ? ent_cnt + (int64_t)inst * P.n_total : nullptr;
    ent.e64 = ent64 + D.ent_off; ent.sid = ent_sid + D.ent_off; ent.ent_cap = D.ent_cap;
    double m[MARGIN_CATS];
    candidate_margins(P, D, L, tab, q, ent, m);
    for (int c = 0; c < MARGIN_CATS; ++c) out[(int64_t)idx * MARGIN_CATS + c] = m[c];
}

// ---------------------------------------------------------------------------
// wire form of the records (fot_pack_records_device): one wave per record
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(WAVE)
k_pack_wire(int n, int n_total, int stride, const fot_result *__restrict__ src, unsigned char *__restrict__ dst)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const fot_result &R = src[i];
    unsigned char *w = dst + (int64_t)i * stride;
    fot_wire_header *H = (fot_wire_header *)w;
    if (lane == 0) {
        H->status = R.status; H->best_index = R.best_index; H->n_cand = R.n_cand; H->n_keep = R.n_keep;
        H->cost = R.cost; H->stats_valid = R.stats_valid; H->n_total = n_total;
        H->new_last_kappa = R.new_last_kappa; H->new_prev_s = R.new_prev_s;
    }
    if (lane < 8) H->stats[lane] = R.stats[lane];
    if (lane < 6) { H->frenet0[lane] = R.frenet0[lane]; H->ref0[lane] = R.ref0[lane]; }
    float *path = (float *)(w + sizeof(fot_wire_header));
    const double *arr = R.t;                                  // the 15 arrays are contiguous, FOT_MAX_NT doubles each
    // s, x and y travel as offsets from the record's own start state (s0, reference point): float32 then resolves the
    // path to 2^-24 of its LENGTH (4e-6 m at 70 m), wherever in the world it lies; samples past n_keep are zero
    const int keep = R.n_keep;
    for (int f = 0; f < 15; ++f) {
        const double base = f == 1 ? R.frenet0[0] : f == 9 ? R.ref0[1] : f == 10 ? R.ref0[2] : 0.0;
        for (int k = lane; k < n_total; k += WAVE)
            path[f * n_total + k] = k < keep ? (float)(arr[f * FOT_MAX_NT + k] - base) : 0.0f;
    }
    // padding bytes stay as they are (never read)
}

// ---------------------------------------------------------------------------
// spline evaluation (fot_spline_eval)
// ---------------------------------------------------------------------------

__global__ void k_spline_eval(SplineView sp, int n, const double *__restrict__ s, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SplinePt p;
    spline_point(sp, s[i], p);
    double cr, sr, kappa, dkappa;
    spline_frame(p, cr, sr, kappa, dkappa);
    out[0 * (int64_t)n + i] = p.x;
    out[1 * (int64_t)n + i] = p.y;
    out[2 * (int64_t)n + i] = atan2(p.dy, p.dx);
    out[3 * (int64_t)n + i] = kappa;
    out[4 * (int64_t)n + i] = dkappa;
}

// external paths (fot_check_collision_paths / fot_check_paths): one lane per path, arrays [n_paths][FOT_MAX_NT]
// in the caller's row-major layout, obstacles straight from the caller's layout (exact float64 test)
struct PathArraySource {
    const double *x, *y, *yaw, *t;      // this path's rows
    double dt;
    const double *circ_off;
    int has_footprint;
    __device__ __forceinline__ int tindex(int k) const { return (int)nearbyint(t[k] / dt); }
    __device__ __forceinline__ void get(int k, int ci, double &px, double &py) const
    {
        if (has_footprint) {                 // frenet_planner.py:1162-1167
            px = x[k] + circ_off[ci] * cos(yaw[k]);
            py = y[k] + circ_off[ci] * sin(yaw[k]);
        } else {
            px = x[k]; py = y[k];
        }
    }
};

// mode 0: collision only (status_out = 1 free / 0 hit); mode 1: _check_paths categories (FOT_ST_*).
// rule_len[n_paths][FOT_CHECK_RULE_LENS]: n_geo and the lengths of d, v, a, c, s (mode 1), each 0..FOT_MAX_NT.
__global__ void k_check_ext(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, int n_paths, int mode,
                            const int32_t *__restrict__ len, const int32_t *__restrict__ rule_len,
                            const double *__restrict__ arrays /* [9][n_paths][FOT_MAX_NT]: x y yaw v a c d s t */,
                            const double *__restrict__ static_xy, const double *__restrict__ dyn_xy,
                            int32_t *__restrict__ status_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_paths) return;
    const DevParams &P = *Pp;
    const InstDesc &D = desc[0];
    const int64_t plane = (int64_t)n_paths * FOT_MAX_NT;
    const double *row = arrays + (int64_t)i * FOT_MAX_NT;
    const double *ax = row, *ay = row + plane, *ayaw = row + 2 * plane, *av = row + 3 * plane, *aa = row + 4 * plane,
                 *ac = row + 5 * plane, *ad = row + 6 * plane, *as = row + 7 * plane, *at = row + 8 * plane;
    const int n = len[i];
    PathArraySource src;
    src.x = ax; src.y = ay; src.yaw = ayaw; src.t = at; src.dt = P.dt;
    src.circ_off = P.circ_off; src.has_footprint = P.has_footprint;
    ObstacleView obs;
    obs.stat = static_xy; obs.dyn = dyn_xy; obs.dtype = FOT_F64;
    // a NaN in any collision point makes the reference's path box NaN, which no obstacle is inside (np.min / np.max
    // propagate it, frenet_planner.py:1177-1178): such a path collides with nothing, at any of its samples
    bool nan_point = false;
    const int n_circ = P.has_footprint ? P.n_circ : 1;
    for (int k = 0; k < n; ++k)
        for (int ci = 0; ci < n_circ; ++ci) {
            double px, py;
            src.get(k, ci, px, py);
            nan_point |= isnan(px) || isnan(py);
        }
    if (mode == 0) {
        const bool hit = n > 0 && !nan_point && collide_candidate(P, D, obs, n, src);
        status_out[i] = hit ? 0 : 1;
        return;
    }
    const int32_t *rl = rule_len + (int64_t)i * FOT_CHECK_RULE_LENS;
    const int n_geo = rl[0] < n ? rl[0] : n, n_d = rl[1], n_v = rl[2], n_a = rl[3], n_c = rl[4], n_s = rl[5];
    int n_loop = n;
    n_loop = n_d > n_loop ? n_d : n_loop; n_loop = n_v > n_loop ? n_v : n_loop;
    n_loop = n_a > n_loop ? n_a : n_loop; n_loop = n_c > n_loop ? n_c : n_loop;
    CheckAcc acc;
    check_init(acc);
    const LoopConst lc = loop_const(P, D);
    for (int k = 0; k < n_loop && n > 0; ++k) {
        const uint32_t has = (k < n ? RL_XY : 0u) | (k < n_v ? RL_V : 0u) | (k < n_a ? RL_A : 0u) | (k < n_c ? RL_C : 0u) |
                             (k < n_d ? RL_D : 0u) | (k < n_geo ? RL_GEO : 0u);
        PathSample ps;
        ps.x = ax[k]; ps.y = ay[k]; ps.cos_t = cos(ayaw[k]); ps.sin_t = sin(ayaw[k]);
        ps.kappa = ac[k]; ps.v = av[k]; ps.a = aa[k]; ps.d = ad[k];
        check_sample_ext(lc, acc, k, ps, has, [&] { return fabs(as[k] - as[k - 1]); });
    }
    int st = check_status(D, acc, n);
    if (st == ST_PENDING && n > 0 && !nan_point && collide_candidate(P, D, obs, n, src)) st = FOT_ST_COLLISION;
    // the stop filter reads the last entries of v and s as the caller gave them (:317-318): no v never stops, no s is no travel
    if (n > 0) st = final_status(st, n_v > 0 ? av[n_v - 1] : NAN, n_s > 0 ? as[n_s - 1] - as[0] : 0.0, D.max_stop);
    status_out[i] = st;
}

// The same against a distribution of more than FOT_MAX_SAMPLES samples (a handle with a raised sample capacity):
// collide_candidate counts in a SampleMask4.  A copy of the body above, not a template both kernels share: k_check_ext
// is then, instruction for instruction, the kernel it was before this one existed (scripts/isa_compare.py).
__global__ void k_check_ext_wide(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, int n_paths, int mode,
                                 const int32_t *__restrict__ len, const int32_t *__restrict__ rule_len,
                                 const double *__restrict__ arrays, const double *__restrict__ static_xy,
                                 const double *__restrict__ dyn_xy, int32_t *__restrict__ status_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_paths) return;
    const DevParams &P = *Pp;
    const InstDesc &D = desc[0];
    const int64_t plane = (int64_t)n_paths * FOT_MAX_NT;
    const double *row = arrays + (int64_t)i * FOT_MAX_NT;
    const double *ax = row, *ay = row + plane, *ayaw = row + 2 * plane, *av = row + 3 * plane, *aa = row + 4 * plane,
                 *ac = row + 5 * plane, *ad = row + 6 * plane, *as = row + 7 * plane, *at = row + 8 * plane;
    const int n = len[i];
    PathArraySource src;
    src.x = ax; src.y = ay; src.yaw = ayaw; src.t = at; src.dt = P.dt;
    src.circ_off = P.circ_off; src.has_footprint = P.has_footprint;
    ObstacleView obs;
    obs.stat = static_xy; obs.dyn = dyn_xy; obs.dtype = FOT_F64;
    // a NaN in any collision point makes the reference's path box NaN, which no obstacle is inside (np.min / np.max
    // propagate it, frenet_planner.py:1177-1178): such a path collides with nothing, at any of its samples
    bool nan_point = false;
    const int n_circ = P.has_footprint ? P.n_circ : 1;
    for (int k = 0; k < n; ++k)
        for (int ci = 0; ci < n_circ; ++ci) {
            double px, py;
            src.get(k, ci, px, py);
            nan_point |= isnan(px) || isnan(py);
        }
    if (mode == 0) {
        const bool hit = n > 0 && !nan_point && collide_candidate_wide(P, D, obs, n, src);
        status_out[i] = hit ? 0 : 1;
        return;
    }
    const int32_t *rl = rule_len + (int64_t)i * FOT_CHECK_RULE_LENS;
    const int n_geo = rl[0] < n ? rl[0] : n, n_d = rl[1], n_v = rl[2], n_a = rl[3], n_c = rl[4], n_s = rl[5];
    int n_loop = n;
    n_loop = n_d > n_loop ? n_d : n_loop; n_loop = n_v > n_loop ? n_v : n_loop;
    n_loop = n_a > n_loop ? n_a : n_loop; n_loop = n_c > n_loop ? n_c : n_loop;
    CheckAcc acc;
    check_init(acc);
    const LoopConst lc = loop_const(P, D);
    for (int k = 0; k < n_loop && n > 0; ++k) {
        const uint32_t has = (k < n ? RL_XY : 0u) | (k < n_v ? RL_V : 0u) | (k < n_a ? RL_A : 0u) | (k < n_c ? RL_C : 0u) |
                             (k < n_d ? RL_D : 0u) | (k < n_geo ? RL_GEO : 0u);
        PathSample ps;
        ps.x = ax[k]; ps.y = ay[k]; ps.cos_t = cos(ayaw[k]); ps.sin_t = sin(ayaw[k]);
        ps.kappa = ac[k]; ps.v = av[k]; ps.a = aa[k]; ps.d = ad[k];
        check_sample_ext(lc, acc, k, ps, has, [&] { return fabs(as[k] - as[k - 1]); });
    }
    int st = check_status(D, acc, n);
    if (st == ST_PENDING && n > 0 && !nan_point && collide_candidate_wide(P, D, obs, n, src)) st = FOT_ST_COLLISION;
    // the stop filter reads the last entries of v and s as the caller gave them (:317-318): no v never stops, no s is no travel
    if (n > 0) st = final_status(st, n_v > 0 ? av[n_v - 1] : NAN, n_s > 0 ? as[n_s - 1] - as[0] : 0.0, D.max_stop);
    status_out[i] = st;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

#define FOT_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int launch_frenet_state(const DevParams *P, const PathSet &ps, const InstDesc *desc, InstState *state, int n_inst,
                        MetaImport imp, NanScan scan, int32_t *inst_done, hipStream_t st, GroupHeadOut gh)
{
    if (n_inst <= 0) return 0;
    const int lds_knots = ps.fit_knots(SPLINE_LDS_KNOTS);
    const int64_t grid = (int64_t)n_inst * (1 + (scan.flag ? scan.blocks_per_inst : 0));
    if (grid > 0x7fffffffLL) return (int)hipErrorInvalidConfiguration;
    // FOT_FRENET_WAVES=all: every nearest-point block keeps its four waves to its end (tests, A/B runs)
    static const int all_waves = getenv("FOT_FRENET_WAVES") && !std::strcmp(getenv("FOT_FRENET_WAVES"), "all") ? 1 : 0;
    k_frenet_state<<<(unsigned)grid, FRENET_WG, sizeof(double) * 9 * (size_t)lds_knots, st>>>(
        P, ps.one, ps.table, ps.mixed, lds_knots, desc, state, n_inst, imp, scan, inst_done, gh, all_waves);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_cull(const DevParams *P, const InstDesc *desc, const InstState *state, int n_inst, int n_total, int n_ext,
                const PathSet &ps, const void *static_xy, const void *dyn_xy, int dtype, EntryArrays e, TileTable tiles,
                hipStream_t st)
{
    if (n_inst <= 0 || n_total <= 0) return 0;
    const unsigned grid = (unsigned)((int64_t)((n_inst + 7) / 8 * 8) * ((n_total + CULL_KG - 1) / CULL_KG));
    static const int ablate_env = getenv("FOT_CULL_ABLATE") ? atoi(getenv("FOT_CULL_ABLATE")) : 0;   // timing diagnostics
    const int ablate = (ablate_env & ~128) | (e.eager_nan ? 128 : 0);
    const int lds_knots = ps.fit_knots(64);                                 // a short spline rides along in LDS
    // + per horizon / brake-ladder entry: lateral extents of the group's steps, the two extreme lateral quintics
    const size_t lds = sizeof(double) * (9 * (size_t)lds_knots + (size_t)n_ext * (CULL_KG * 2 + 9));
    if (dtype == FOT_F32)
        k_cull<float><<<grid, CULL_KG * WAVE, lds, st>>>(P, desc, state, n_inst, ps.one, ps.table, ps.mixed, lds_knots,
                                             (const float *)static_xy,
                                             (const float *)dyn_xy, e.cnt, e.e32, e.e64, e.sid, e.rng, tiles.cand0, tiles.n, tiles.span,
                                             e.nan_flag, ablate);
    else
        k_cull<double><<<grid, CULL_KG * WAVE, lds, st>>>(P, desc, state, n_inst, ps.one, ps.table, ps.mixed, lds_knots,
                                              (const double *)static_xy,
                                              (const double *)dyn_xy, e.cnt, e.e32, e.e64, e.sid, e.rng, tiles.cand0,
                                              tiles.n, tiles.span, e.nan_flag, ablate);
    FOT_LAUNCH_CHECK();
    return 0;
}

// time segments per tile of a batch's evaluation (1: whole tiles)
static int eval_segments_of(const TileTable &tiles)
{
    int n_seg = tiles.n_tiles <= 2304 ? SEG_MAX : 1;       // (scripts/segment_sweep.py: four segments win up to ~64 egos)
    if (tiles.eval_segments >= 1 && tiles.eval_segments <= SEG_MAX) n_seg = tiles.eval_segments;
    return n_seg;
}

bool evaluate_in_groups(const TileTable &tiles)
{
    return tiles.n_tiles > 0 && eval_segments_of(tiles) == 1 && tiles.grouped;
}

bool evaluate_flat(const TileTable &tiles)
{
    return tiles.flat && tiles.n_tiles > 0 && (eval_segments_of(tiles) > 1 || tiles.grouped);
}

int launch_evaluate(const DevParams *P, const PathSet &ps, const InstDesc *desc, const InstState *state, int n_total,
                    int n_inst, TileTable tiles, EntryArrays e, CandArrays c, fot_result *out, int32_t *inst_done,
                    hipStream_t st)
{
    if (n_inst <= 0) return 0;
    static const int ablate = getenv("FOT_EVAL_ABLATE") ? atoi(getenv("FOT_EVAL_ABLATE")) : 0;
    const int lds_knots = ps.fit_knots(28);                                 // a short spline rides along (2 KB at most)
    // Three launch shapes, 8 queues each (workgroup b serves the instances b mod 8):
    //  * a handful of egos: every tile one workgroup, cut into time segments (k_evaluate_split);
    //  * the grouped cut: one workgroup per group of four tiles (k_evaluate_group, four waves per SIMD);
    //  * the per-wave cut: four independent tiles per workgroup (k_evaluate, three waves per SIMD).
    // Each in its lean form (FusedSink) when the host found the launch eligible (tiles.lean: enqueue_lane), and the lean
    // form in its flat form when every path of the launch is exactly straight (tiles.flat, which implies tiles.lean) --
    // the split and the grouped shape; the per-wave shape has none (evaluate_flat).
    const int n_seg = eval_segments_of(tiles);
    static const int force_wpw = getenv("FOT_EVAL_WPW") ? atoi(getenv("FOT_EVAL_WPW")) : 0;      // diagnostics
    int wpw = n_seg > 1 ? 1 : tiles.n_tiles >= 1024 ? EVAL_WG / WAVE : 1;
    if (n_seg == 1 && force_wpw >= 1 && force_wpw <= EVAL_WG / WAVE) wpw = force_wpw;
    const int64_t per_queue = (int64_t)((n_inst + N_XCD - 1) / N_XCD) * tiles.max_tiles;
    const int64_t n_blocks = (per_queue + wpw - 1) / wpw * N_XCD;
    if (n_blocks > 0x7fffffffLL) return (int)hipErrorInvalidConfiguration;
    // (wide: an instance of more than FOT_MAX_SAMPLES samples -- the *_wide kernels, whose general form hands four mask
    //  words from segment to segment; no flat form)
    const int seg_d = seg_doubles(tiles.wide && !tiles.lean ? WIDE_MASK_WORDS : 1);
    const size_t lds = sizeof(double) * ((size_t)eval_wave_doubles(tiles.row_budget) * wpw + 9 * (size_t)lds_knots
                                         + (n_seg > 1 ? (size_t)(SEG_MAX - 1) * seg_d : 0));
    if (tiles.wide && tiles.flat) return (int)hipErrorInvalidValue;
    EvalKernArgs a;
    a.Pp = P; a.sp = ps.one; a.desc = desc; a.state = state;
    a.sp_table = ps.table; a.mixed = ps.mixed;
    a.row_budget = tiles.row_budget; a.lds_knots = lds_knots; a.ablate = ablate;
    a.n_inst = n_inst; a.max_tiles = tiles.max_tiles;
    a.tile_cand0 = tiles.cand0;
    a.wave_rng = e.rng; a.ent32 = e.e32; a.ent64 = e.e64; a.ent_sid = e.sid;
    a.cand_cost = c.cost; a.cand_status = c.status; a.cand_keep = c.keep; a.parts = c.parts;
    a.out = out; a.inst_done = inst_done; a.done_flag = c.done_flag; a.done_seq = c.done_seq;
    a.heads = tiles.heads;
    if (tiles.n_tiles <= 0) {
        k_select_only<<<(unsigned)n_inst, WAVE, 0, st>>>(P, desc, state, tiles.cand0, tiles.n, e.rng, e.e32, a);
    } else if (tiles.wide) {
        if (n_seg > 1) {
            (tiles.lean ? k_evaluate_split_lean_wide : k_evaluate_split_wide)<<<(unsigned)n_blocks, n_seg * WAVE, lds, st>>>(
                P, desc, state, tiles.cand0, tiles.n, e.rng, e.e32, a);
        } else if (tiles.grouped) {
            if (!tiles.heads) return (int)hipErrorInvalidValue;
            const int per_q = (n_inst + N_XCD - 1) / N_XCD * (tiles.max_tiles / GROUP_TILES);
            const size_t g_lds = sizeof(double) * ((size_t)eval_group_doubles() + 9 * (size_t)lds_knots);
            (tiles.lean ? k_evaluate_group_lean_wide : k_evaluate_group_wide)<<<(unsigned)(per_q * N_XCD), GROUP_TILES * WAVE, g_lds, st>>>(
                P, desc, state, tiles.cand0, tiles.n, e.rng, e.e32, a);
        } else {
            (tiles.lean ? k_evaluate_lean_wide : k_evaluate_wide)<<<(unsigned)n_blocks, wpw * WAVE, lds, st>>>(
                P, desc, state, tiles.cand0, tiles.n, e.rng, e.e32, a);
        }
    } else if (n_seg > 1) {
        (tiles.flat ? k_evaluate_split_lean_flat : tiles.lean ? k_evaluate_split_lean : k_evaluate_split)<<<(unsigned)n_blocks, n_seg * WAVE, lds, st>>>(
            P, desc, state, tiles.cand0, tiles.n, e.rng, e.e32, a);
    } else if (tiles.grouped) {                                            // one workgroup per group of tiles
        if (!tiles.heads) return (int)hipErrorInvalidValue;                // (evaluate_in_groups(): the caller builds them)
        const int per_q = (n_inst + N_XCD - 1) / N_XCD * (tiles.max_tiles / GROUP_TILES);
        const size_t g_lds = sizeof(double) * ((size_t)eval_group_doubles() + 9 * (size_t)lds_knots);
        (tiles.flat ? k_evaluate_group_lean_flat : tiles.lean ? k_evaluate_group_lean : k_evaluate_group)<<<(unsigned)(per_q * N_XCD), GROUP_TILES * WAVE, g_lds, st>>>(
            P, desc, state, tiles.cand0, tiles.n, e.rng, e.e32, a);
    } else {
        (tiles.lean ? k_evaluate_lean : k_evaluate)<<<(unsigned)n_blocks, wpw * WAVE, lds, st>>>(
            P, desc, state, tiles.cand0, tiles.n, e.rng, e.e32, a);
    }
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_debug_path(const DevParams *P, const InstDesc *desc, const InstState *state,
                      SplineView sp, int inst, int idx, double *out, int32_t *meta, hipStream_t st)
{
    k_debug_path<<<1, WAVE, 0, st>>>(P, desc, state, sp, inst, idx, out, meta);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_debug_margins(const DevParams *P, const InstDesc *desc, const InstState *state, SplineView sp, int inst,
                         EntryArrays e, int cap, double *out, hipStream_t st)
{
    if (cap <= 0) return 0;
    k_debug_margins<<<(cap + WAVE - 1) / WAVE, WAVE, 0, st>>>(P, desc, state, sp, inst, e.cnt, e.e64, e.sid, cap, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_pack_wire(int n, int n_total, int stride, const fot_result *src, unsigned char *dst, hipStream_t st)
{
    if (n <= 0) return 0;
    k_pack_wire<<<n, WAVE, 0, st>>>(n, n_total, stride, src, dst);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_spline_eval(SplineView sp, int n, const double *s, double *out, hipStream_t st)
{
    if (n <= 0) return 0;
    k_spline_eval<<<(n + 255) / 256, 256, 0, st>>>(sp, n, s, out);
    FOT_LAUNCH_CHECK();
    return 0;
}

int launch_check_ext(const DevParams *P, const InstDesc *desc, int n_paths, int mode, const int32_t *len,
                     const int32_t *rule_len, const double *arrays, const double *static_xy, const double *dyn_xy,
                     int32_t *status_out, hipStream_t st, int wide)
{
    if (n_paths <= 0) return 0;
    (wide ? k_check_ext_wide : k_check_ext)<<<(n_paths + 63) / 64, 64, 0, st>>>(P, desc, n_paths, mode, len, rule_len, arrays,
                                                                                static_xy, dyn_xy, status_out);
    FOT_LAUNCH_CHECK();
    return 0;
}

}  // namespace fot
