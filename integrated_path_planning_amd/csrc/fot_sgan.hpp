// fot_sgan.hpp -- the arithmetic of fot_sgan_sample: float32 inference of the Social-GAN trajectory generator
// (reference src/prediction/sgan_vendor/models.py, TrajectoryGenerator.forward) followed by relative_to_abs, for many
// scenes at once.  Plain C++ shared by the kernels (fot_sgan.hip), the host (descriptor rules, the packed blob's order,
// the device image of the weights) and tests/emu/fot_sgan_emu.cpp, which evaluates a scene sequentially on the CPU.
//
// With rel[0] = 0, rel[t] = obs[t] - obs[t - 1], L(x) = W x + b a Linear (BatchNorm of eval mode already folded in) and
// lstm(x, h, c) one torch LSTM cell (gates i, f, g, o):
//   encoder        h = c = 0; for t < obs_len: (h, c) = lstm(L_emb(rel[t]), h, c)                      -> h_enc [He]
//   pool(h, pos)   pool_i = max_j relu(L_2(relu(L_1([L_sp(pos_j - pos_i) ; h_j]))))  over the scene's j  -> [B]
//   context        ctx = relu(L_c2(relu(L_c1([h_enc ; pool(h_enc, obs[-1])]))))                        -> [Hd - nd]
//                  (absent without noise, pooling and with He == Hd: ctx = h_enc)
//   decoder        h = [ctx ; z], c = 0, x = L_demb(rel[-1]), pos = obs[-1], cum = 0; for t < pred_len:
//                    (h, c) = lstm(x, h, c); r = L_pos(h); pos = r + pos; cum = cum + r; out[t] = cum + obs[-1];
//                    pool_every_timestep: h = relu(L_m2(relu(L_m1([h ; pool(h, pos)])))); x = L_demb(r)
// Everything up to ctx is computed once per pedestrian / scene; the S samples differ from the noise z on.
//
// The first pool layer is rearranged: with W_1 = [W_1e | W_1h], L_1([L_sp(d) ; h_j]) = A d + u_j, A = W_1e W_sp (512 x 2)
// and u_j = W_1h h_j + (W_1e b_sp + b_1): u_j once per pedestrian instead of once per pair.  A and the constant are
// formed in float64 when the weights are loaded and rounded once.
//
// Order of every sum: the bias first, then the terms in index order, one output element per thread -- so a scene's
// numbers do not depend on what else is in the launch; the pool's max is exact in any order.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fot.h"

#if defined(__HIPCC__)
#define FOT_SG_HD __host__ __device__ inline
#else
#define FOT_SG_HD inline
#endif

namespace fot {

constexpr int SG_POOL_HIDDEN = FOT_SGAN_POOL_HIDDEN;   // first layer of the pool net (fixed by the reference, models.py:159)
constexpr int SG_BPAD = 8;                             // the pool's second layer is laid out in blocks of 8 outputs

FOT_SG_HD float sg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
FOT_SG_HD float sg_tanh(float x) { return tanhf(x); }
FOT_SG_HD float sg_relu(float x) { return x > 0.0f ? x : 0.0f; }

// one LSTM cell from the four pre-activations (torch gate order i, f, g, o); returns h, updates c
FOT_SG_HD float sg_lstm_cell(float pi, float pf, float pg, float po, float *c)
{
    const float cn = sg_sigmoid(pf) * *c + sg_sigmoid(pi) * sg_tanh(pg);
    *c = cn;
    return sg_sigmoid(po) * sg_tanh(cn);
}

// y = b + w0 x + w1 y: every Linear(2, .) of the model
FOT_SG_HD float sg_lin2(float w0, float w1, float b, float x, float y) { return b + w0 * x + w1 * y; }

// first pool layer after the rearrangement: relu(A d + u)
FOT_SG_HD float sg_pool_hidden(float ax, float ay, float u, float dx, float dy) { return sg_relu(u + ax * dx + ay * dy); }

// ---- descriptor rules ------------------------------------------------------------------------------------------------
inline bool sg_pooled(const fot_sgan_desc &d) { return d.pooling_type == FOT_SGAN_POOL_NET; }
inline bool sg_pool_steps(const fot_sgan_desc &d) { return sg_pooled(d) && d.pool_every_timestep != 0; }
inline bool sg_has_context(const fot_sgan_desc &d)                   // mlp_decoder_needed (models.py:409)
{
    return d.noise_dim > 0 || sg_pooled(d) || d.encoder_h_dim != d.decoder_h_dim;
}

// FOT_OK, or the refusal with its reason
inline int sg_check_desc(const fot_sgan_desc &d, std::string &why)
{
    if (d.obs_len < 1 || d.pred_len < 1 || d.embedding_dim < 1 || d.encoder_h_dim < 1 || d.decoder_h_dim < 1 ||
        d.noise_dim < 0 || d.num_layers < 1 || !(d.dropout >= 0.0f) || d.pooling_type < 0 || d.pooling_type > FOT_SGAN_SPOOL ||
        (d.noise_mix_type != FOT_SGAN_NOISE_PED && d.noise_mix_type != FOT_SGAN_NOISE_GLOBAL)) {
        why = "fot_sgan_desc: a dimension below 1, or an unknown pooling / noise mix type";
        return FOT_ERR_INVALID;
    }
    if ((sg_has_context(d) || sg_pool_steps(d)) && d.mlp_dim < 1) { why = "fot_sgan_desc: mlp_dim < 1"; return FOT_ERR_INVALID; }
    if (sg_pooled(d) && d.bottleneck_dim < 1) { why = "fot_sgan_desc: bottleneck_dim < 1"; return FOT_ERR_INVALID; }
    if (d.noise_dim >= d.decoder_h_dim && sg_has_context(d)) { why = "fot_sgan_desc: noise_dim >= decoder_h_dim"; return FOT_ERR_INVALID; }
    if (d.pooling_type == FOT_SGAN_SPOOL) { why = "fot_sgan_desc: social pooling ('spool') is not supported"; return FOT_ERR_UNSUPPORTED; }
    if (d.num_layers > 1) { why = "fot_sgan_desc: num_layers > 1"; return FOT_ERR_UNSUPPORTED; }
    if (d.dropout > 0.0f) { why = "fot_sgan_desc: dropout"; return FOT_ERR_UNSUPPORTED; }
    if (d.embedding_dim > FOT_SGAN_MAX_EMBEDDING || d.encoder_h_dim > FOT_SGAN_MAX_HIDDEN || d.decoder_h_dim > FOT_SGAN_MAX_HIDDEN ||
        d.obs_len > FOT_SGAN_MAX_OBS_LEN || d.pred_len > FOT_MAX_PRED_LEN ||
        ((sg_has_context(d) || sg_pool_steps(d)) && d.mlp_dim > FOT_SGAN_MAX_MLP) ||
        (sg_pooled(d) && d.bottleneck_dim > FOT_SGAN_MAX_BOTTLENECK)) {
        why = "fot_sgan_desc: a dimension above its FOT_SGAN_MAX_* / FOT_MAX_PRED_LEN";
        return FOT_ERR_UNSUPPORTED;
    }
    return FOT_OK;
}

// ---- the packed blob (include/fot.h documents this order) and the device image ------------------------------------------
struct SgLstm { int64_t emb_w, emb_b, w_ih, w_hh, b_ih, b_hh; };          // offsets in floats
struct SgPool { int64_t sp_w, sp_b, w1, b1, w2, b2; };
struct SgMlp { int64_t w1, b1, w2, b2; };
struct SgBlob {
    SgLstm enc, dec;
    SgPool pool, dpool;
    SgMlp ctx, dmlp;
    int64_t pos_w, pos_b, total;
};

inline SgBlob sg_blob_layout(const fot_sgan_desc &d)
{
    SgBlob L{};
    int64_t at = 0;
    auto take = [&](int64_t n) { const int64_t o = at; at += n; return o; };
    const int E = d.embedding_dim, He = d.encoder_h_dim, Hd = d.decoder_h_dim, M = d.mlp_dim, B = sg_pooled(d) ? d.bottleneck_dim : 0;
    auto lstm = [&](SgLstm &l, int H) {
        l.emb_w = take(2 * E); l.emb_b = take(E);
        l.w_ih = take((int64_t)4 * H * E); l.w_hh = take((int64_t)4 * H * H); l.b_ih = take(4 * H); l.b_hh = take(4 * H);
    };
    auto pool = [&](SgPool &p, int H) {
        p.sp_w = take(2 * E); p.sp_b = take(E);
        p.w1 = take((int64_t)SG_POOL_HIDDEN * (E + H)); p.b1 = take(SG_POOL_HIDDEN);
        p.w2 = take((int64_t)B * SG_POOL_HIDDEN); p.b2 = take(B);
    };
    auto mlp = [&](SgMlp &m, int K, int O) {
        m.w1 = take((int64_t)M * K); m.b1 = take(M); m.w2 = take((int64_t)O * M); m.b2 = take(O);
    };
    lstm(L.enc, He);
    if (sg_pooled(d)) pool(L.pool, He);
    if (sg_has_context(d)) mlp(L.ctx, He + B, Hd - d.noise_dim);
    lstm(L.dec, Hd);
    L.pos_w = take(2 * Hd); L.pos_b = take(2);
    if (sg_pool_steps(d)) { pool(L.dpool, Hd); mlp(L.dmlp, Hd + B, Hd); }
    L.total = at;
    return L;
}

// The device image: every matrix transposed ([input][output], so that neighbouring threads read neighbouring words),
// the LSTM's two biases added, the pool's first layer rearranged, its second padded to a multiple of SG_BPAD outputs.
struct SgDevLstm { int64_t emb_w, emb_b, wih_t, whh_t, b; };              // emb_w [E][2]; wih_t [E][4H]; whh_t [H][4H]; b [4H]
struct SgDevPool { int64_t w1h_t, c0, a, w2_t, b2; int32_t h_dim, b_pad; };  // w1h_t [H][512]; c0 [512]; a [2][512]; w2_t [512][b_pad]
struct SgDevMlp { int64_t w1_t, b1, w2_t, b2; int32_t k, m, o, _pad; };   // w1_t [k][m]; w2_t [m][o]
struct SgDev {
    SgDevLstm enc, dec;
    SgDevPool pool, dpool;
    SgDevMlp ctx, dmlp;
    int64_t pos_w, pos_b, total;                                          // pos_w [2][Hd]
};

inline int sg_bpad(int B) { return (B + SG_BPAD - 1) / SG_BPAD * SG_BPAD; }

inline SgDev sg_dev_image(const fot_sgan_desc &d, const float *w, std::vector<float> &img)
{
    const SgBlob L = sg_blob_layout(d);
    SgDev D{};
    img.clear();
    const int E = d.embedding_dim, He = d.encoder_h_dim, Hd = d.decoder_h_dim, M = d.mlp_dim, B = sg_pooled(d) ? d.bottleneck_dim : 0;
    auto grow = [&](int64_t n) {                                  // (every array starts on 16 bytes: the pool reads float4)
        const int64_t o = ((int64_t)img.size() + 3) / 4 * 4;
        img.resize((size_t)(o + n), 0.0f);
        return o;
    };
    auto copy = [&](int64_t src, int64_t n) { const int64_t o = grow(n); for (int64_t i = 0; i < n; ++i) img[(size_t)(o + i)] = w[src + i]; return o; };
    auto transposed = [&](int64_t src, int rows, int cols, int col0, int ncols, int ld_out) {   // W [rows][cols] -> [ncols][ld_out]
        const int64_t o = grow((int64_t)ncols * ld_out);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < ncols; ++c) img[(size_t)(o + (int64_t)c * ld_out + r)] = w[src + (int64_t)r * cols + col0 + c];
        return o;
    };
    auto lstm = [&](const SgLstm &l, int H, SgDevLstm &o) {
        o.emb_w = copy(l.emb_w, 2 * E); o.emb_b = copy(l.emb_b, E);
        o.wih_t = transposed(l.w_ih, 4 * H, E, 0, E, 4 * H);
        o.whh_t = transposed(l.w_hh, 4 * H, H, 0, H, 4 * H);
        o.b = grow(4 * H);
        for (int i = 0; i < 4 * H; ++i) img[(size_t)(o.b + i)] = w[l.b_ih + i] + w[l.b_hh + i];
    };
    auto pool = [&](const SgPool &p, int H, SgDevPool &o) {
        const int K = E + H, bp = sg_bpad(B);
        o.h_dim = H; o.b_pad = bp;
        o.w1h_t = transposed(p.w1, SG_POOL_HIDDEN, K, E, H, SG_POOL_HIDDEN);
        o.c0 = grow(SG_POOL_HIDDEN);
        o.a = grow(2 * SG_POOL_HIDDEN);
        for (int m = 0; m < SG_POOL_HIDDEN; ++m) {
            double c0 = w[p.b1 + m], ax = 0.0, ay = 0.0;
            for (int e = 0; e < E; ++e) {
                const double w1e = w[p.w1 + (int64_t)m * K + e];
                c0 += w1e * (double)w[p.sp_b + e];
                ax += w1e * (double)w[p.sp_w + 2 * e];
                ay += w1e * (double)w[p.sp_w + 2 * e + 1];
            }
            img[(size_t)(o.c0 + m)] = (float)c0;
            img[(size_t)(o.a + m)] = (float)ax;
            img[(size_t)(o.a + SG_POOL_HIDDEN + m)] = (float)ay;
        }
        o.w2_t = transposed(p.w2, B, SG_POOL_HIDDEN, 0, SG_POOL_HIDDEN, bp);
        o.b2 = grow(bp);
        for (int b = 0; b < B; ++b) img[(size_t)(o.b2 + b)] = w[p.b2 + b];
    };
    auto mlp = [&](const SgMlp &m, int K, int O, SgDevMlp &o) {
        o.k = K; o.m = M; o.o = O; o._pad = 0;
        o.w1_t = transposed(m.w1, M, K, 0, K, M); o.b1 = copy(m.b1, M);
        o.w2_t = transposed(m.w2, O, M, 0, M, O); o.b2 = copy(m.b2, O);
    };
    lstm(L.enc, He, D.enc);
    if (sg_pooled(d)) pool(L.pool, He, D.pool);
    if (sg_has_context(d)) mlp(L.ctx, He + B, Hd - d.noise_dim, D.ctx);
    lstm(L.dec, Hd, D.dec);
    D.pos_w = copy(L.pos_w, 2 * Hd); D.pos_b = copy(L.pos_b, 2);
    if (sg_pool_steps(d)) { pool(L.dpool, Hd, D.dpool); mlp(L.dmlp, Hd + B, Hd, D.dmlp); }
    D.total = (int64_t)img.size();
    return D;
}

// ---- one scene evaluated sequentially (the host-side form of what the kernels compute, for the emulation) -------------
namespace sg_seq {

inline void lstm_step(const float *img, const SgDevLstm &l, int E, int H, const float *x, std::vector<float> &h, std::vector<float> &c)
{
    std::vector<float> hn((size_t)H);
    for (int k = 0; k < H; ++k) {
        float pre[4];
        for (int g = 0; g < 4; ++g) {
            float acc = img[l.b + g * H + k];
            for (int e = 0; e < E; ++e) acc += img[l.wih_t + (int64_t)e * 4 * H + g * H + k] * x[e];
            for (int j = 0; j < H; ++j) acc += img[l.whh_t + (int64_t)j * 4 * H + g * H + k] * h[(size_t)j];
            pre[g] = acc;
        }
        hn[(size_t)k] = sg_lstm_cell(pre[0], pre[1], pre[2], pre[3], &c[(size_t)k]);
    }
    h = hn;
}

inline void embed(const float *img, const SgDevLstm &l, int E, float rx, float ry, std::vector<float> &x)
{
    x.resize((size_t)E);
    for (int e = 0; e < E; ++e) x[(size_t)e] = sg_lin2(img[l.emb_w + 2 * e], img[l.emb_w + 2 * e + 1], img[l.emb_b + e], rx, ry);
}

// h [P][H], pos [P][2] -> pool [P][B]
inline void pool(const float *img, const SgDevPool &p, int P, int B, const std::vector<float> &h, const std::vector<float> &pos,
                 std::vector<float> &out)
{
    const int H = p.h_dim, NH = SG_POOL_HIDDEN;
    std::vector<float> u((size_t)P * NH), y((size_t)NH);
    for (int j = 0; j < P; ++j)
        for (int m = 0; m < NH; ++m) {
            float acc = img[p.c0 + m];
            for (int k = 0; k < H; ++k) acc += img[p.w1h_t + (int64_t)k * NH + m] * h[(size_t)j * H + k];
            u[(size_t)j * NH + m] = acc;
        }
    out.assign((size_t)P * B, 0.0f);
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            const float dx = pos[(size_t)2 * j] - pos[(size_t)2 * i], dy = pos[(size_t)2 * j + 1] - pos[(size_t)2 * i + 1];
            for (int m = 0; m < NH; ++m)
                y[(size_t)m] = sg_pool_hidden(img[p.a + m], img[p.a + NH + m], u[(size_t)j * NH + m], dx, dy);
            for (int b = 0; b < B; ++b) {
                float acc = img[p.b2 + b];
                for (int m = 0; m < NH; ++m) acc += img[p.w2_t + (int64_t)m * p.b_pad + b] * y[(size_t)m];
                acc = sg_relu(acc);
                if (acc > out[(size_t)i * B + b]) out[(size_t)i * B + b] = acc;
            }
        }
}

// x [k] -> out [o]
inline void mlp(const float *img, const SgDevMlp &m, const float *x, float *out)
{
    std::vector<float> mid((size_t)m.m);
    for (int o = 0; o < m.m; ++o) {
        float acc = img[m.b1 + o];
        for (int k = 0; k < m.k; ++k) acc += img[m.w1_t + (int64_t)k * m.m + o] * x[k];
        mid[(size_t)o] = sg_relu(acc);
    }
    for (int o = 0; o < m.o; ++o) {
        float acc = img[m.b2 + o];
        for (int k = 0; k < m.m; ++k) acc += img[m.w2_t + (int64_t)k * m.o + o] * mid[(size_t)k];
        out[o] = sg_relu(acc);
    }
}

}  // namespace sg_seq

// obs [obs_len][N][2] (the whole launch; the scene's rows are p0 .. p0 + P - 1), noise: sample s of row r at
// noise[(s * noise_rows + r) * nd], out [S][pred_len][N][2]
inline void sg_scene_forward(const fot_sgan_desc &d, const SgDev &D, const float *img, int N, int p0, int P, int scene,
                             const float *obs, int S, const float *noise, int noise_rows, float *out)
{
    using namespace sg_seq;
    if (P <= 0) return;
    const int E = d.embedding_dim, He = d.encoder_h_dim, Hd = d.decoder_h_dim, nd = d.noise_dim, T = d.obs_len;
    const int B = sg_pooled(d) ? d.bottleneck_dim : 0;
    auto ob = [&](int t, int p, int ax) { return obs[((size_t)t * N + p0 + p) * 2 + ax]; };
    std::vector<float> henc((size_t)P * He), x, last((size_t)P * 2), lrel((size_t)P * 2, 0.0f);
    for (int p = 0; p < P; ++p) {
        std::vector<float> h((size_t)He, 0.0f), c((size_t)He, 0.0f);
        for (int t = 0; t < T; ++t) {
            const float rx = t ? ob(t, p, 0) - ob(t - 1, p, 0) : 0.0f, ry = t ? ob(t, p, 1) - ob(t - 1, p, 1) : 0.0f;
            embed(img, D.enc, E, rx, ry, x);
            lstm_step(img, D.enc, E, He, x.data(), h, c);
            if (t == T - 1) { lrel[(size_t)2 * p] = rx; lrel[(size_t)2 * p + 1] = ry; }
        }
        for (int k = 0; k < He; ++k) henc[(size_t)p * He + k] = h[(size_t)k];
        last[(size_t)2 * p] = ob(T - 1, p, 0); last[(size_t)2 * p + 1] = ob(T - 1, p, 1);
    }
    const int nc = sg_has_context(d) ? Hd - nd : He;
    std::vector<float> ctx((size_t)P * nc), pl;
    if (sg_pooled(d)) pool(img, D.pool, P, B, henc, last, pl);
    for (int p = 0; p < P; ++p) {
        if (!sg_has_context(d)) { for (int k = 0; k < He; ++k) ctx[(size_t)p * nc + k] = henc[(size_t)p * He + k]; continue; }
        std::vector<float> in((size_t)(He + B));
        for (int k = 0; k < He; ++k) in[(size_t)k] = henc[(size_t)p * He + k];
        for (int b = 0; b < B; ++b) in[(size_t)(He + b)] = pl[(size_t)p * B + b];
        mlp(img, D.ctx, in.data(), &ctx[(size_t)p * nc]);
    }
    for (int s = 0; s < S; ++s) {
        std::vector<float> h((size_t)P * Hd), c((size_t)P * Hd, 0.0f), pos = last, cum((size_t)P * 2, 0.0f), rel = lrel;
        for (int p = 0; p < P; ++p) {
            for (int k = 0; k < nc; ++k) h[(size_t)p * Hd + k] = ctx[(size_t)p * nc + k];
            const int row = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL ? scene : p0 + p;
            for (int k = nc; k < Hd; ++k) h[(size_t)p * Hd + k] = noise[((size_t)s * noise_rows + row) * nd + (k - nc)];
        }
        for (int t = 0; t < d.pred_len; ++t) {
            for (int p = 0; p < P; ++p) {
                std::vector<float> hp(h.begin() + (size_t)p * Hd, h.begin() + (size_t)(p + 1) * Hd);
                std::vector<float> cp(c.begin() + (size_t)p * Hd, c.begin() + (size_t)(p + 1) * Hd);
                embed(img, D.dec, E, rel[(size_t)2 * p], rel[(size_t)2 * p + 1], x);
                lstm_step(img, D.dec, E, Hd, x.data(), hp, cp);
                for (int ax = 0; ax < 2; ++ax) {
                    float acc = img[D.pos_b + ax];
                    for (int k = 0; k < Hd; ++k) acc += img[D.pos_w + (int64_t)ax * Hd + k] * hp[(size_t)k];
                    rel[(size_t)2 * p + ax] = acc;
                    pos[(size_t)2 * p + ax] = acc + pos[(size_t)2 * p + ax];
                    cum[(size_t)2 * p + ax] = cum[(size_t)2 * p + ax] + acc;
                    out[(((size_t)s * d.pred_len + t) * N + p0 + p) * 2 + ax] = cum[(size_t)2 * p + ax] + last[(size_t)2 * p + ax];
                }
                for (int k = 0; k < Hd; ++k) { h[(size_t)p * Hd + k] = hp[(size_t)k]; c[(size_t)p * Hd + k] = cp[(size_t)k]; }
            }
            if (sg_pool_steps(d)) {
                pool(img, D.dpool, P, B, h, pos, pl);
                std::vector<float> in((size_t)(Hd + B));
                for (int p = 0; p < P; ++p) {
                    for (int k = 0; k < Hd; ++k) in[(size_t)k] = h[(size_t)p * Hd + k];
                    for (int b = 0; b < B; ++b) in[(size_t)(Hd + b)] = pl[(size_t)p * B + b];
                    mlp(img, D.dmlp, in.data(), &h[(size_t)p * Hd]);
                }
            }
        }
    }
}

}  // namespace fot
