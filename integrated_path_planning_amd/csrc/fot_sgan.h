// fot_sgan.h -- launchers of the Social-GAN kernels and of the resident loop's observer window (fot_sgan.hip) for the host
// side (fot_host_pred.cpp: the sampler; fot_host_loop.cpp: the resident loop's window and noise).
#pragma once

#include <hip/hip_runtime.h>

#include "fot_noise.hpp"
#include "fot_sgan.hpp"

namespace fot {

// One launch of the decoder: rows are (sample, pedestrian) pairs, row = s * N + n.  init: the state is built from the
// context and the noise (else read from h / c / pos / rel / cum); save: it is written back after n_steps steps.
struct SgDecode {
    const float *img;
    SgDevLstm l;
    int64_t pos_w, pos_b;
    int32_t E, H, N, S, obs_len, pred_len, t0, n_steps, init, save;
    const float *obs;                        // [obs_len][N][2]
    const float *ctx;                        // [N][nc]
    const float *noise;                      // [S][noise_rows][nd]
    const int32_t *row_scene;                // [N], NULL: the noise is per pedestrian
    int32_t nc, nd, noise_rows, _pad;
    float *h, *c, *pos, *rel, *cum;          // [S N][H] / [S N][2]
    float *out;                              // [S][pred_len][N][2]
};

// fot_sgan_noise: out[s][r][d] (32-bit words: float32, or the raw uint32 of NOISE_RAW), n_blk = ceil(nd / 4) blocks per row;
// row r is index[r] of slot[r] at that slot's step[r] (tables: pinned host memory or HBM)
struct SgNoise {
    uint64_t seed;
    int32_t kind, S, rows, nd, n_blk, _pad;
    const int32_t *slot, *step, *index;      // [rows]
    uint32_t *out;                           // [S][rows][nd]
};

// The observer's window of a resident step: sample j is replay frame frames.f[j]; row q of the compacted frame belongs
// to running episode ped_ep[q], which is slot ep_slot[.] with its first row at ep_ped0[.].
struct SgWindowFrames {
    int32_t f[FOT_SGAN_MAX_OBS_LEN];
};
struct SgWindow {
    const double *pos;                       // the recording [n_frames_max][n_cols][2]
    const int32_t *slot_ped0, *slot_frames;  // per slot: first column, recorded frames
    const int32_t *ped_ep, *ep_ped0;         // HBM (FrameDev)
    const int32_t *ep_slot;                  // pinned host memory (FrameStage)
    int32_t n_cols, rows, obs_len, _pad;
    SgWindowFrames frames;
    float *out;                              // [obs_len][rows][2]
};

int launch_sgan_noise(const SgNoise &a, hipStream_t st);
int launch_sgan_window(const SgWindow &a, hipStream_t st);
int launch_sgan_encode(const float *img, const SgDevLstm &l, int E, int H, int obs_len, int N, const float *obs, float *henc,
                       hipStream_t st);
// h [S][N][p.h_dim], pos [S][N][2] -> out [S][N][p.b_pad], which the caller has zeroed
int launch_sgan_pool(const float *img, const SgDevPool &p, int n_scenes, int S, int N, const int32_t *ped_off, const float *h,
                     const float *pos, float *out, hipStream_t st);
// out[row] = relu(L2(relu(L1([a[row][0 .. ka) ; b[row][0 .. kb)])))), b rows ldb apart, out rows ldo apart (out may be a)
int launch_sgan_mlp(const float *img, const SgDevMlp &m, const float *a, int ka, const float *b, int kb, int ldb, int64_t rows,
                    float *out, int ldo, hipStream_t st);
int launch_sgan_decode(const SgDecode &a, hipStream_t st);

}  // namespace fot
