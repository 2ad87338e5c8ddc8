// fot_sgan.hip -- the kernels of fot_sgan_sample (gfx950): Social-GAN sample generation for many scenes at once.
// The arithmetic, the order of every sum and the device image of the weights are fot_sgan.hpp's.
//
//   k_sgan_encode   16 pedestrians per workgroup, all obs_len steps of the encoder LSTM with the state in LDS
//   k_sgan_pool     one workgroup per (scene, sample): 16 neighbours j at a time, u_j in LDS, then every pair (i, j)
//   k_sgan_mlp      4 rows per workgroup through a two-layer MLP, input and middle layer in LDS
//   k_sgan_decode   16 (sample, pedestrian) rows per workgroup: all pred_len steps in one launch, or -- with pooling at
//                   every step -- one step per launch, the state in HBM between the launches
//   k_sgan_noise    fot_sgan_noise: one thread per (sample, row, block of four noise dimensions), fot_noise.hpp's Philox
//   k_sgan_window   the resident loop's observer window [obs_len][rows][2] float32 out of the recording in HBM
// A thread owns an output element and adds its terms in index order; several rows share one read of a weight.  Plain
// float32 VALU: the f32-input MFMA forms of gfx950 run at the vector rate.
#include <hip/hip_runtime.h>

#include "fot_sgan.h"

namespace fot {

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_RT = 16;                    // rows of an LSTM tile ...
constexpr int SG_RG = 4;                     // ... of which a thread carries 4
constexpr int SG_JT = 16;                    // neighbours of a pool tile (the lanes a pair's max is folded over)
constexpr int SG_MT = 4;                     // rows of an MLP tile
constexpr int MAXE = FOT_SGAN_MAX_EMBEDDING, MAXH = FOT_SGAN_MAX_HIDDEN, NH = SG_POOL_HIDDEN;
constexpr int MAXK = FOT_SGAN_MAX_HIDDEN + FOT_SGAN_MAX_BOTTLENECK, MAXM = FOT_SGAN_MAX_MLP;
static_assert(SG_THREADS % SG_JT == 0 && SG_JT == 16, "a pair's neighbours sit in 16 adjacent lanes");
static_assert(SG_RT * 2 <= SG_THREADS && SG_RT % SG_RG == 0, "tile shapes");

// (rows padded by one word: threads of a wave that carry different row groups read different banks)
struct LstmTile {
    float x[SG_RT][MAXE + 1];
    float h[2][SG_RT][MAXH + 1];
    float c[SG_RT][MAXH + 1];
};

// one LSTM step of the tile: (x, h) -> hn, c in place.  The caller puts a barrier in front and behind.
__device__ void sg_lstm_tile(const float *__restrict__ wih_t, const float *__restrict__ whh_t, const float *__restrict__ b,
                             int E, int H, const float (*x)[MAXE + 1], const float (*h)[MAXH + 1], float (*hn)[MAXH + 1],
                             float (*c)[MAXH + 1])
{
    const int H4 = 4 * H;
    for (int idx = threadIdx.x; idx < H * (SG_RT / SG_RG); idx += SG_THREADS) {
        const int k = idx % H, r0 = idx / H * SG_RG;
        float acc[4][SG_RG];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float bg = b[g * H + k];
#pragma unroll
            for (int r = 0; r < SG_RG; ++r) acc[g][r] = bg;
        }
        for (int e = 0; e < E; ++e) {
            const float *wr = wih_t + (size_t)e * H4 + k;
            const float w0 = wr[0], w1 = wr[H], w2 = wr[2 * H], w3 = wr[3 * H];
#pragma unroll
            for (int r = 0; r < SG_RG; ++r) {
                const float v = x[r0 + r][e];
                acc[0][r] += w0 * v; acc[1][r] += w1 * v; acc[2][r] += w2 * v; acc[3][r] += w3 * v;
            }
        }
        for (int j = 0; j < H; ++j) {
            const float *wr = whh_t + (size_t)j * H4 + k;
            const float w0 = wr[0], w1 = wr[H], w2 = wr[2 * H], w3 = wr[3 * H];
#pragma unroll
            for (int r = 0; r < SG_RG; ++r) {
                const float v = h[r0 + r][j];
                acc[0][r] += w0 * v; acc[1][r] += w1 * v; acc[2][r] += w2 * v; acc[3][r] += w3 * v;
            }
        }
#pragma unroll
        for (int r = 0; r < SG_RG; ++r)
            hn[r0 + r][k] = sg_lstm_cell(acc[0][r], acc[1][r], acc[2][r], acc[3][r], &c[r0 + r][k]);
    }
}

__global__ __launch_bounds__(SG_THREADS) void k_sgan_encode(const float *__restrict__ img, SgDevLstm l, int E, int H, int T, int N,
                                                            const float *__restrict__ obs, float *__restrict__ henc)
{
    __shared__ LstmTile t;
    const int row0 = blockIdx.x * SG_RT;
    for (int i = threadIdx.x; i < SG_RT * (MAXH + 1); i += SG_THREADS) { (&t.h[0][0][0])[i] = 0.0f; (&t.c[0][0])[i] = 0.0f; }
    int cur = 0;
    for (int step = 0; step < T; ++step) {
        for (int idx = threadIdx.x; idx < SG_RT * E; idx += SG_THREADS) {
            const int r = idx / E, e = idx % E, row = row0 + r;
            float rx = 0.0f, ry = 0.0f;
            if (row < N && step > 0) {
                const float *now = obs + ((size_t)step * N + row) * 2, *was = obs + ((size_t)(step - 1) * N + row) * 2;
                rx = now[0] - was[0]; ry = now[1] - was[1];
            }
            t.x[r][e] = sg_lin2(img[l.emb_w + 2 * e], img[l.emb_w + 2 * e + 1], img[l.emb_b + e], rx, ry);
        }
        __syncthreads();
        sg_lstm_tile(img + l.wih_t, img + l.whh_t, img + l.b, E, H, t.x, t.h[cur], t.h[cur ^ 1], t.c);
        __syncthreads();
        cur ^= 1;
    }
    for (int idx = threadIdx.x; idx < SG_RT * H; idx += SG_THREADS) {
        const int r = idx / H, k = idx % H, row = row0 + r;
        if (row < N) henc[(size_t)row * H + k] = t.h[cur][r][k];
    }
}

__global__ __launch_bounds__(SG_THREADS) void k_sgan_decode(SgDecode a)
{
    __shared__ LstmTile t;
    __shared__ float s_rel[SG_RT][2], s_pos[SG_RT][2], s_cum[SG_RT][2], s_start[SG_RT][2];
    const float *__restrict__ img = a.img;
    const int E = a.E, H = a.H, N = a.N;
    const int64_t total = (int64_t)a.S * N, R0 = (int64_t)blockIdx.x * SG_RT;
    for (int idx = threadIdx.x; idx < SG_RT * H; idx += SG_THREADS) {
        const int r = idx / H, k = idx % H;
        const int64_t R = R0 + r;
        float hv = 0.0f, cv = 0.0f;
        if (R < total) {
            if (a.init) {
                const int s = (int)(R / N), n = (int)(R % N);
                if (k < a.nc) hv = a.ctx[(size_t)n * a.nc + k];
                else hv = a.noise[((size_t)s * a.noise_rows + (a.row_scene ? a.row_scene[n] : n)) * a.nd + (k - a.nc)];
            } else {
                hv = a.h[(size_t)R * H + k]; cv = a.c[(size_t)R * H + k];
            }
        }
        t.h[0][r][k] = hv; t.c[r][k] = cv;
    }
    if (threadIdx.x < SG_RT * 2) {
        const int r = threadIdx.x >> 1, ax = threadIdx.x & 1;
        const int64_t R = R0 + r;
        float st = 0.0f, rel = 0.0f, pos = 0.0f, cum = 0.0f;
        if (R < total) {
            const int n = (int)(R % N);
            st = a.obs[((size_t)(a.obs_len - 1) * N + n) * 2 + ax];
            if (a.init) {
                pos = st;
                rel = a.obs_len > 1 ? st - a.obs[((size_t)(a.obs_len - 2) * N + n) * 2 + ax] : 0.0f;
            } else {
                pos = a.pos[(size_t)R * 2 + ax]; rel = a.rel[(size_t)R * 2 + ax]; cum = a.cum[(size_t)R * 2 + ax];
            }
        }
        s_start[r][ax] = st; s_rel[r][ax] = rel; s_pos[r][ax] = pos; s_cum[r][ax] = cum;
    }
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < a.n_steps; ++step) {
        for (int idx = threadIdx.x; idx < SG_RT * E; idx += SG_THREADS) {
            const int r = idx / E, e = idx % E;
            t.x[r][e] = sg_lin2(img[a.l.emb_w + 2 * e], img[a.l.emb_w + 2 * e + 1], img[a.l.emb_b + e], s_rel[r][0], s_rel[r][1]);
        }
        __syncthreads();
        sg_lstm_tile(img + a.l.wih_t, img + a.l.whh_t, img + a.l.b, E, H, t.x, t.h[cur], t.h[cur ^ 1], t.c);
        __syncthreads();
        cur ^= 1;
        if (threadIdx.x < SG_RT * 2) {                              // hidden2pos, the running position and the output
            const int r = threadIdx.x >> 1, ax = threadIdx.x & 1;
            const int64_t R = R0 + r;
            float acc = img[a.pos_b + ax];
            const float *w = img + a.pos_w + (size_t)ax * H;
            for (int k = 0; k < H; ++k) acc += w[k] * t.h[cur][r][k];
            s_rel[r][ax] = acc;
            s_pos[r][ax] = acc + s_pos[r][ax];
            const float cum = s_cum[r][ax] + acc;
            s_cum[r][ax] = cum;
            if (R < total) {
                const int s = (int)(R / N), n = (int)(R % N);
                a.out[(((size_t)s * a.pred_len + a.t0 + step) * N + n) * 2 + ax] = cum + s_start[r][ax];
            }
        }
        __syncthreads();
    }
    if (!a.save) return;
    for (int idx = threadIdx.x; idx < SG_RT * H; idx += SG_THREADS) {
        const int r = idx / H, k = idx % H;
        const int64_t R = R0 + r;
        if (R < total) { a.h[(size_t)R * H + k] = t.h[cur][r][k]; a.c[(size_t)R * H + k] = t.c[r][k]; }
    }
    if (threadIdx.x < SG_RT * 2) {
        const int r = threadIdx.x >> 1, ax = threadIdx.x & 1;
        const int64_t R = R0 + r;
        if (R < total) {
            a.pos[(size_t)R * 2 + ax] = s_pos[r][ax]; a.rel[(size_t)R * 2 + ax] = s_rel[r][ax]; a.cum[(size_t)R * 2 + ax] = s_cum[r][ax];
        }
    }
}

// pool_i = max_j relu(L2(relu(A (pos_j - pos_i) + u_j))), u_j = c0 + W1h h_j.  A thread carries one (i, j, block of 8
// outputs); the 16 lanes of one (i, block) hold 16 neighbours j, their max is folded with shuffles and lane 0 adds it to
// the output with an integer atomic max: the values are >= 0 behind the ReLU, where the integer order of the bit patterns
// is the order of the floats, and a max is the same in every order.
__global__ __launch_bounds__(SG_THREADS) void k_sgan_pool(const float *__restrict__ img, SgDevPool p, int N,
                                                          const int32_t *__restrict__ ped_off, const float *__restrict__ h,
                                                          const float *__restrict__ pos, float *__restrict__ out)
{
    __shared__ float s_u[SG_JT][NH + 1];
    __shared__ float s_h[SG_JT][MAXH + 1];
    __shared__ float s_a[2][NH];
    __shared__ float s_pj[SG_JT][2];
    const int scene = blockIdx.x, s = blockIdx.y;
    const int p0 = ped_off[scene], P = ped_off[scene + 1] - p0;
    if (P <= 0) return;
    const int H = p.h_dim, bp = p.b_pad;
    const size_t base = (size_t)s * N + p0;
    for (int i = threadIdx.x; i < 2 * NH; i += SG_THREADS) (&s_a[0][0])[i] = img[p.a + i];
    const float *__restrict__ w1h_t = img + p.w1h_t, *__restrict__ w2_t = img + p.w2_t, *__restrict__ b2 = img + p.b2;
    for (int j0 = 0; j0 < P; j0 += SG_JT) {
        const int nj = min(SG_JT, P - j0);
        __syncthreads();                                           // (the tile before this one has been read)
        for (int idx = threadIdx.x; idx < SG_JT * H; idx += SG_THREADS) {
            const int jj = idx / H, k = idx % H;
            s_h[jj][k] = jj < nj ? h[(base + j0 + jj) * H + k] : 0.0f;
        }
        if (threadIdx.x < SG_JT * 2) {
            const int jj = threadIdx.x >> 1, ax = threadIdx.x & 1;
            s_pj[jj][ax] = jj < nj ? pos[(base + j0 + jj) * 2 + ax] : 0.0f;
        }
        __syncthreads();
        for (int m = threadIdx.x; m < NH; m += SG_THREADS) {
            float acc[SG_JT];
            const float c0 = img[p.c0 + m];
#pragma unroll
            for (int jj = 0; jj < SG_JT; ++jj) acc[jj] = c0;
            for (int k = 0; k < H; ++k) {
                const float w = w1h_t[(size_t)k * NH + m];
#pragma unroll
                for (int jj = 0; jj < SG_JT; ++jj) acc[jj] += w * s_h[jj][k];
            }
#pragma unroll
            for (int jj = 0; jj < SG_JT; ++jj) s_u[jj][m] = acc[jj];
        }
        __syncthreads();
        const int total = (bp / SG_BPAD) * P * SG_JT;              // (<= 128 * 256 * 16)
        for (int idx = threadIdx.x; idx < total; idx += SG_THREADS) {
            const int jj = idx % SG_JT, i = (idx / SG_JT) % P, bb = idx / (SG_JT * P);
            float z[SG_BPAD];
#pragma unroll
            for (int q = 0; q < SG_BPAD; ++q) z[q] = 0.0f;
            if (jj < nj) {
                const float dx = s_pj[jj][0] - pos[(base + i) * 2], dy = s_pj[jj][1] - pos[(base + i) * 2 + 1];
                float acc[SG_BPAD];
#pragma unroll
                for (int q = 0; q < SG_BPAD; ++q) acc[q] = b2[bb * SG_BPAD + q];
                for (int m = 0; m < NH; ++m) {
                    const float y = sg_pool_hidden(s_a[0][m], s_a[1][m], s_u[jj][m], dx, dy);
                    const float4 *w = (const float4 *)(w2_t + (size_t)m * bp + bb * SG_BPAD);   // (16-byte aligned: sg_dev_image)
                    const float4 wa = w[0], wb = w[1];
                    acc[0] += wa.x * y; acc[1] += wa.y * y; acc[2] += wa.z * y; acc[3] += wa.w * y;
                    acc[4] += wb.x * y; acc[5] += wb.y * y; acc[6] += wb.z * y; acc[7] += wb.w * y;
                }
#pragma unroll
                for (int q = 0; q < SG_BPAD; ++q) z[q] = sg_relu(acc[q]);
            }
#pragma unroll
            for (int q = 0; q < SG_BPAD; ++q) {
                float v = z[q];
#pragma unroll
                for (int off = SG_JT / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, SG_JT));
                z[q] = v;
            }
            if (jj == 0) {
                int *dst = (int *)(out + (base + i) * bp + bb * SG_BPAD);
#pragma unroll
                for (int q = 0; q < SG_BPAD; ++q) atomicMax(dst + q, __float_as_int(z[q]));
            }
        }
    }
}

__global__ __launch_bounds__(SG_THREADS) void k_sgan_mlp(const float *__restrict__ img, SgDevMlp m, const float *a, int ka,
                                                         const float *__restrict__ b, int kb, int ldb, int64_t rows, float *out,
                                                         int ldo)
{
    __shared__ float s_x[SG_MT][MAXK];
    __shared__ float s_mid[SG_MT][MAXM];
    const int64_t row0 = (int64_t)blockIdx.x * SG_MT;
    const int K = ka + kb, M = m.m, O = m.o;
    for (int idx = threadIdx.x; idx < SG_MT * K; idx += SG_THREADS) {
        const int r = idx / K, k = idx % K;
        const int64_t row = row0 + r;
        float v = 0.0f;
        if (row < rows) v = k < ka ? a[(size_t)row * ka + k] : b[(size_t)row * ldb + (k - ka)];
        s_x[r][k] = v;
    }
    __syncthreads();
    const float *__restrict__ w1 = img + m.w1_t, *__restrict__ w2 = img + m.w2_t;
    for (int o = threadIdx.x; o < M; o += SG_THREADS) {
        float acc[SG_MT];
        const float b1 = img[m.b1 + o];
#pragma unroll
        for (int r = 0; r < SG_MT; ++r) acc[r] = b1;
        for (int k = 0; k < K; ++k) {
            const float w = w1[(size_t)k * M + o];
#pragma unroll
            for (int r = 0; r < SG_MT; ++r) acc[r] += w * s_x[r][k];
        }
#pragma unroll
        for (int r = 0; r < SG_MT; ++r) s_mid[r][o] = sg_relu(acc[r]);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < O; o += SG_THREADS) {
        float acc[SG_MT];
        const float b2 = img[m.b2 + o];
#pragma unroll
        for (int r = 0; r < SG_MT; ++r) acc[r] = b2;
        for (int k = 0; k < M; ++k) {
            const float w = w2[(size_t)k * O + o];
#pragma unroll
            for (int r = 0; r < SG_MT; ++r) acc[r] += w * s_mid[r][k];
        }
#pragma unroll
        for (int r = 0; r < SG_MT; ++r)
            if (row0 + r < rows) out[(size_t)(row0 + r) * ldo + o] = sg_relu(acc[r]);
    }
}

// One thread per (sample s, row r, block b): the numbers of dimensions 4 b .. 4 b + 3 of row r of sample s, a function of
// (seed, slot[r], step[r], index[r], s, b) alone -- no atomics, nothing of the launch shape.  The tables lie in pinned
// host memory or HBM.
__global__ __launch_bounds__(SG_THREADS) void k_sgan_noise(SgNoise a)
{
    const int64_t t = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
    const int64_t per_s = (int64_t)a.rows * a.n_blk;
    if (t >= per_s * a.S) return;
    const int s = (int)(t / per_s), r = (int)((t - s * per_s) / a.n_blk), b = (int)(t % a.n_blk);
    uint32_t v[4];
    noise_values(noise_block(a.seed, a.slot[r], a.step[r], a.index[r], s, b), a.kind, v);
    uint32_t *dst = a.out + ((int64_t)s * a.rows + r) * a.nd + 4 * b;
    for (int j = 0; j < 4; ++j)
        if (4 * b + j < a.nd) dst[j] = v[j];
}

// One thread per (window sample j, frame row q): the position of the row's pedestrian at replay frame frames[j], clamped
// to its slot's own recording and rounded to float32 as the observer hands it over (observer.py:134).
__global__ __launch_bounds__(SG_THREADS) void k_sgan_window(SgWindow a)
{
    const int64_t t = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
    if (t >= (int64_t)a.obs_len * a.rows) return;
    const int j = (int)(t / a.rows), q = (int)(t % a.rows);
    const int i = a.ped_ep[q], slot = a.ep_slot[i], p = q - a.ep_ped0[i];
    const int last_row = a.slot_frames[slot] - 1;
    const int row = min(max(a.frames.f[j], 0), last_row);
    const double2 v = ((const double2 *)a.pos)[(int64_t)row * a.n_cols + a.slot_ped0[slot] + p];
    float2 w; w.x = (float)v.x; w.y = (float)v.y;
    ((float2 *)a.out)[t] = w;
}

}  // namespace

#define FOT_SG_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int launch_sgan_encode(const float *img, const SgDevLstm &l, int E, int H, int obs_len, int N, const float *obs, float *henc,
                       hipStream_t st)
{
    if (N <= 0) return 0;
    k_sgan_encode<<<(N + SG_RT - 1) / SG_RT, SG_THREADS, 0, st>>>(img, l, E, H, obs_len, N, obs, henc);
    FOT_SG_LAUNCH_CHECK();
    return 0;
}

int launch_sgan_pool(const float *img, const SgDevPool &p, int n_scenes, int S, int N, const int32_t *ped_off, const float *h,
                     const float *pos, float *out, hipStream_t st)
{
    if (n_scenes <= 0 || S <= 0 || N <= 0) return 0;
    k_sgan_pool<<<dim3((unsigned)n_scenes, (unsigned)S), SG_THREADS, 0, st>>>(img, p, N, ped_off, h, pos, out);
    FOT_SG_LAUNCH_CHECK();
    return 0;
}

int launch_sgan_mlp(const float *img, const SgDevMlp &m, const float *a, int ka, const float *b, int kb, int ldb, int64_t rows,
                    float *out, int ldo, hipStream_t st)
{
    if (rows <= 0) return 0;
    k_sgan_mlp<<<(unsigned)((rows + SG_MT - 1) / SG_MT), SG_THREADS, 0, st>>>(img, m, a, ka, b, kb, ldb, rows, out, ldo);
    FOT_SG_LAUNCH_CHECK();
    return 0;
}

int launch_sgan_decode(const SgDecode &a, hipStream_t st)
{
    const int64_t total = (int64_t)a.S * a.N;
    if (total <= 0 || a.n_steps <= 0) return 0;
    k_sgan_decode<<<(unsigned)((total + SG_RT - 1) / SG_RT), SG_THREADS, 0, st>>>(a);
    FOT_SG_LAUNCH_CHECK();
    return 0;
}

int launch_sgan_noise(const SgNoise &a, hipStream_t st)
{
    const int64_t total = (int64_t)a.S * a.rows * a.n_blk;
    if (total <= 0) return 0;
    k_sgan_noise<<<(unsigned)((total + SG_THREADS - 1) / SG_THREADS), SG_THREADS, 0, st>>>(a);
    FOT_SG_LAUNCH_CHECK();
    return 0;
}

int launch_sgan_window(const SgWindow &a, hipStream_t st)
{
    const int64_t total = (int64_t)a.obs_len * a.rows;
    if (total <= 0) return 0;
    k_sgan_window<<<(unsigned)((total + SG_THREADS - 1) / SG_THREADS), SG_THREADS, 0, st>>>(a);
    FOT_SG_LAUNCH_CHECK();
    return 0;
}

}  // namespace fot
