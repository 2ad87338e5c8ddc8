// fot_sgan.h -- launchers of the Social-GAN kernels (fot_sgan.hip) for the host side (fot_host.cpp).
#pragma once

#include <hip/hip_runtime.h>

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
