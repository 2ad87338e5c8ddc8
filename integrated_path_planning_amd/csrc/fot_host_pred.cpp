// fot_host_pred.cpp -- the entry points of libfot.so that predict or score without keeping loop state: the resampler and
// the constant-velocity predictor, the safety metrics, the prediction scores, the Social-GAN sampler, the open-loop
// evaluation, the footprint re-verification, the fidelity statistics and the extraction of encounters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fot_host.hpp"
#include "fot_loop_kernels.h"
#include "fot_sgan.h"

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

// Shared body of fot_prediction_scores and fot_loop_prediction_scores: `tensor` is device memory, or host memory of
// tensor_bytes bytes to be copied first (tensor_bytes > 0).  Checks every origin before anything is enqueued or written.
int prediction_scores_impl(fot_handle *h, const char *who, int32_t n, const fot_pred_origin *desc, const void *tensor,
                           size_t tensor_bytes, int32_t dtype, int32_t stride, int32_t E, const double *truth,
                           fot_pred_score *out, hipStream_t st)
{
    const std::string w(who);
    if (stride < 1 || E < 1) return fail(h, FOT_ERR_INVALID, w + ": stride and E must be positive");
    if (E > FOT_MAX_PRED_LEN) return fail(h, FOT_ERR_UNSUPPORTED, w + ": E > FOT_MAX_PRED_LEN");
    size_t rows = 0;
    bool any = false, wide = false;                                // wide: an origin of more than FOT_MAX_SAMPLES samples
    for (int i = 0; i < n; ++i) {
        const fot_pred_origin &d = desc[i];
        if (d.S < 1 || d.P < 0 || d.T < 1 || d.offset < 0 || (d.skip != 0 && d.skip != 1) ||
            (d.layout != 0 && d.layout != FOT_DYN_LAYOUT_TSP))
            return fail(h, FOT_ERR_INVALID, w + ": an origin's S / P / T / offset / skip / layout");
        if (!ps_horizon_fits(stride, E, d.T, d.skip))
            return fail(h, FOT_ERR_INVALID, w + ": stride E - 1 reaches past an origin's dense track (T - skip)");
        if (d.S > h->sample_cap) return refuse_samples(h, w + ": ", d.S);
        wide = wide || d.S > FOT_MAX_SAMPLES;
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
    LAUNCH_TRY(h, launch_pred_scores(pd, n, d_tensor, dtype, stride, E, pt, (fot_pred_score *)h->hScoreOut.p, st, wide ? 1 : 0));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));
    std::memcpy(out, h->hScoreOut.p, sizeof(fot_pred_score) * (size_t)n);
    return FOT_OK;
}

// The work arrays sgan_enqueue grows on demand, brought to the size of N pedestrians and S samples up front: a call that
// enqueues several chunks then frees nothing (hipFree waits for the device) between them.
int sgan_reserve(fot_handle *h, int model, int N, int S)
{
    fot_handle::Sgan &G = h->sgan[model];
    const fot_sgan_desc &d = G.desc;
    const bool pooled = sg_pooled(d), steps = sg_pool_steps(d), context = sg_has_context(d);
    const int nc = context ? d.decoder_h_dim - d.noise_dim : d.encoder_h_dim;
    const size_t rows = (size_t)S * N;
    HIP_TRY(h, G.dHenc.ensure(sizeof(float) * (size_t)N * d.encoder_h_dim));
    if (pooled) HIP_TRY(h, G.dPool.ensure(sizeof(float) * (steps ? rows : (size_t)N) * G.dev.pool.b_pad));
    if (context) HIP_TRY(h, G.dCtx.ensure(sizeof(float) * (size_t)N * nc));
    if (steps) {
        HIP_TRY(h, G.dH.ensure(sizeof(float) * rows * d.decoder_h_dim));
        HIP_TRY(h, G.dC.ensure(sizeof(float) * rows * d.decoder_h_dim));
        HIP_TRY(h, G.dXY.ensure(sizeof(float) * rows * 6));
    }
    return FOT_OK;
}

}  // namespace

// ---- the helper fot_host.hpp declares for the resident loop's sampler step (fot_host_loop.cpp loop_run_step)
// The launches of fot_sgan_sample behind its inputs, enqueue only (no copy from host memory, no synchronisation): all S
// samples of the N > 0 pedestrians of n_scenes scenes from the loaded model `model`, in its own work arrays.  d_off [n_scenes + 1] and d_scene [N] (the scene of every pedestrian;
// nullptr unless the noise is per scene) are device memory, as are the tensors.
int fot::host::sgan_enqueue(fot_handle *h, int model, int n_scenes, int N, int S, const int32_t *d_off, const int32_t *d_scene,
                            const float *d_obs, const float *d_noise, float *d_out, hipStream_t st)
{
    fot_handle::Sgan &G = h->sgan[model];
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

extern "C" {

int fot_resample_n_dense(const fot_resample_params *rp, int32_t pred_len)
{
    if (!rp || !(rp->sim_dt > 0.0) || !(rp->sgan_dt > 0.0) || pred_len < 1) return FOT_ERR_INVALID;
    return resample_n_dense(rp->sgan_dt, rp->sim_dt, rp->plan_horizon, pred_len);
}

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
        desc[(size_t)e] = fot_pred_origin{ L.blk_off[(size_t)e], L.count_of((size_t)e), L.ped_off[(size_t)e + 1] - L.ped_off[(size_t)e],
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

// ---- several models per handle: fot_sgan_load / fot_sgan_unload / fot_sgan_sample are the _model entries with model = 0
int32_t fot_sgan_max_models(void) { return SGAN_MAX_MODELS; }

static int sgan_load_impl(fot_handle *h, const std::string &who, int32_t model, const fot_sgan_desc *desc, int64_t n, const float *weights)
{
    if (!h) return FOT_ERR_INVALID;
    if (model < 0 || model >= SGAN_MAX_MODELS) return fail(h, FOT_ERR_INVALID, who + ": model lies outside 0 .. fot_sgan_max_models() - 1");
    if (!desc || !weights) return fail(h, FOT_ERR_INVALID, who + ": desc / weights is NULL");
    if (h->loop.replay.set && h->loop.replay.smp.on) return fail(h, FOT_ERR_INVALID, who + ": the resident loop's sampler uses the handle's models (fot_loop_set_sampler)");
    std::string why;
    const int rc = sg_check_desc(*desc, why);
    if (rc != FOT_OK) return fail(h, rc, why);
    if (n != sg_blob_layout(*desc).total) return fail(h, FOT_ERR_INVALID, who + ": n is not fot_sgan_weight_count of the descriptor");
    std::vector<float> img;
    const SgDev dev = sg_dev_image(*desc, weights, img);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                   // (a sample call of the model before this one is synchronous anyway)
    fot_handle::Sgan &G = h->sgan[model];
    G.loaded = false;
    HIP_TRY(h, G.dImg.ensure(sizeof(float) * img.size()));
    HIP_TRY(h, hipMemcpy(G.dImg.p, img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice));
    G.desc = *desc;
    G.dev = dev;
    G.loaded = true;
    return FOT_OK;
}

int fot_sgan_load(fot_handle *h, const fot_sgan_desc *desc, int64_t n, const float *weights)
{
    return sgan_load_impl(h, "fot_sgan_load", 0, desc, n, weights);
}

int fot_sgan_load_model(fot_handle *h, int32_t model, const fot_sgan_desc *desc, int64_t n, const float *weights)
{
    return sgan_load_impl(h, "fot_sgan_load_model", model, desc, n, weights);
}

static int sgan_unload_impl(fot_handle *h, const std::string &who, int32_t model, bool must_be_loaded)
{
    if (!h) return FOT_ERR_INVALID;
    if (model < 0 || model >= SGAN_MAX_MODELS) return fail(h, FOT_ERR_INVALID, who + ": model lies outside 0 .. fot_sgan_max_models() - 1");
    if (h->loop.replay.set && h->loop.replay.smp.on) return fail(h, FOT_ERR_INVALID, who + ": the resident loop's sampler uses the handle's models (fot_loop_set_sampler)");
    if (must_be_loaded && !h->sgan[model].loaded) return fail(h, FOT_ERR_INVALID, who + ": the model is not loaded (fot_sgan_load_model)");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->sgan[model].loaded = false;
    h->sgan[model].release();
    return FOT_OK;
}

int fot_sgan_unload(fot_handle *h) { return sgan_unload_impl(h, "fot_sgan_unload", 0, false); }   // (no model: nothing to drop)

int fot_sgan_unload_model(fot_handle *h, int32_t model) { return sgan_unload_impl(h, "fot_sgan_unload_model", model, true); }

static int sgan_sample_impl(fot_handle *h, const std::string &who, int32_t model, int32_t n_scenes, const int32_t *ped_off, const void *obs,
                            int32_t S, const void *noise, int32_t flags, void *out, void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (model < 0 || model >= SGAN_MAX_MODELS) return fail(h, FOT_ERR_INVALID, who + ": model lies outside 0 .. fot_sgan_max_models() - 1");
    fot_handle::Sgan &G = h->sgan[model];
    if (!G.loaded) return fail(h, FOT_ERR_INVALID, who + ": no model loaded (fot_sgan_load)");
    if (n_scenes < 0 || !ped_off) return fail(h, FOT_ERR_INVALID, who + ": n_scenes / ped_off (one offset even for no scene)");
    if (S < 1) return fail(h, FOT_ERR_INVALID, who + ": S < 1");
    if (flags & ~(FOT_OUT_DEVICE | FOT_SGAN_OBS_DEVICE | FOT_SGAN_NOISE_DEVICE)) return fail(h, FOT_ERR_INVALID, who + ": flags");
    if (ped_off[0] != 0) return fail(h, FOT_ERR_INVALID, who + ": ped_off must start at 0 and be non-decreasing");
    int widest = 0;
    for (int i = 0; i < n_scenes; ++i) {
        if (ped_off[i + 1] < ped_off[i]) return fail(h, FOT_ERR_INVALID, who + ": ped_off must start at 0 and be non-decreasing");
        widest = std::max(widest, ped_off[i + 1] - ped_off[i]);
    }
    if (S > h->sample_cap) return refuse_samples(h, who + ": ", S);
    if (widest > FOT_SGAN_MAX_PEDS) return fail(h, FOT_ERR_UNSUPPORTED, who + ": a scene of more than FOT_SGAN_MAX_PEDS pedestrians");
    const fot_sgan_desc &d = G.desc;
    const int N = ped_off[n_scenes];
    const bool global_noise = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL;
    const int nd = d.noise_dim, noise_rows = global_noise ? n_scenes : N;
    if (N == 0) return FOT_OK;
    if (!obs || !out || (nd > 0 && !noise)) return fail(h, FOT_ERR_INVALID, who + ": NULL tensor");
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
    { int r = sgan_enqueue(h, model, n_scenes, N, S, G.dOff.as<int32_t>(), global_noise && nd > 0 ? G.dScene.as<int32_t>() : nullptr, d_obs,
                           d_noise, d_out, st); if (r != FOT_OK) return r; }
    if (!(flags & FOT_OUT_DEVICE)) HIP_TRY(h, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

int fot_sgan_sample(fot_handle *h, int32_t n_scenes, const int32_t *ped_off, const void *obs, int32_t S, const void *noise,
                    int32_t flags, void *out, void *stream)
{
    return sgan_sample_impl(h, "fot_sgan_sample", 0, n_scenes, ped_off, obs, S, noise, flags, out, stream);
}

int fot_sgan_sample_model(fot_handle *h, int32_t model, int32_t n_scenes, const int32_t *ped_off, const void *obs, int32_t S,
                          const void *noise, int32_t flags, void *out, void *stream)
{
    return sgan_sample_impl(h, "fot_sgan_sample_model", model, n_scenes, ped_off, obs, S, noise, flags, out, stream);
}

int fot_sgan_noise(fot_handle *h, uint64_t seed, int32_t kind, int32_t S, int32_t rows, int32_t noise_dim,
                   const int32_t *row_slot, const int32_t *row_step, const int32_t *row_index, int32_t flags, void *out,
                   void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (kind < 0 || kind >= FOT_NOISE_KINDS) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: kind");
    if (flags & ~FOT_OUT_DEVICE) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: flags");
    if (S < 1 || rows < 0 || noise_dim < 0) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: S < 1 / rows < 0 / noise_dim < 0");
    if (S > h->sample_cap) return refuse_samples(h, "fot_sgan_noise: ", S);
    if (rows == 0 || noise_dim == 0) return FOT_OK;
    if (!row_slot || !row_step || !row_index || !out) return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: NULL table / out");
    for (int r = 0; r < rows; ++r)
        if (row_slot[r] < 0 || row_step[r] < 0 || row_index[r] < 0 || row_index[r] > 0xFFFF)
            return fail(h, FOT_ERR_INVALID, "fot_sgan_noise: a negative table entry, or a row_index above 65535");
    fot_handle::Sgan &G = h->sgan[0];                              // (its table block and noise scratch: no model is read)
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

// ---- open-loop prediction evaluation of a scene (include/fot.h; the shared rules: fot_openloop.hpp) -------------------------
int fot_openloop_eval(fot_handle *h, const fot_openloop_params *p, const void *scene, const int32_t *win_frame0,
                      const int32_t *ped_off, const int32_t *row_col, const void *noise, fot_pred_score *records,
                      void *raw_out, fot_openloop_totals *totals, void *stream)
{
    static_assert(sizeof(OlTotals) == sizeof(fot_openloop_totals) && offsetof(OlTotals, flags) == offsetof(fot_openloop_totals, flags),
                  "OlTotals is fot_openloop_totals");
    if (!h) return FOT_ERR_INVALID;
    const std::string who = "fot_openloop_eval: ";
    auto refuse = [&](int bad, const char *why) { return fail(h, bad == OL_BAD_UNSUPPORTED ? FOT_ERR_UNSUPPORTED : FOT_ERR_INVALID, who + why); };
    if (!p || !totals) return fail(h, FOT_ERR_INVALID, who + "p / totals is NULL");
    if (p->method != FOT_OPENLOOP_CV && p->method != FOT_OPENLOOP_SGAN) return fail(h, FOT_ERR_INVALID, who + "method");
    if (p->flags & ~(FOT_OPENLOOP_SCENE_DEVICE | FOT_OPENLOOP_NOISE_DEVICE)) return fail(h, FOT_ERR_INVALID, who + "flags");
    if (p->scene_dtype != FOT_F32 && p->scene_dtype != FOT_F64) return fail(h, FOT_ERR_INVALID, who + "scene_dtype");
    if (!(p->dt > 0.0)) return fail(h, FOT_ERR_INVALID, who + "dt must be positive");
    if (p->max_rows < 0 || p->win_id0 < 0) return fail(h, FOT_ERR_INVALID, who + "max_rows / win_id0 is negative");
    const bool cv = p->method == FOT_OPENLOOP_CV;
    const int W = p->n_windows, obs_len = p->obs_len, pred_len = p->pred_len, S = p->S;
    const char *why = "";
    { const int bad = ol_check_lengths(p->n_frames, p->n_cols, W, obs_len, pred_len, S, cv, &why); if (bad) return refuse(bad, why); }
    if (cv && raw_out) return fail(h, FOT_ERR_INVALID, who + "raw_out: the constant-velocity predictor has no raw samples");
    int nd = 0;
    bool global_noise = false;
    if (!cv) {
        if (p->model < 0 || p->model >= SGAN_MAX_MODELS) return fail(h, FOT_ERR_INVALID, who + "model lies outside 0 .. fot_sgan_max_models() - 1");
        const fot_handle::Sgan &G = h->sgan[p->model];
        if (!G.loaded) return fail(h, FOT_ERR_INVALID, who + "no model loaded in the slot (fot_sgan_load_model)");
        if (G.desc.obs_len != obs_len || G.desc.pred_len != pred_len) return fail(h, FOT_ERR_INVALID, who + "the model's obs_len / pred_len differ from the call's");
        nd = G.desc.noise_dim;
        global_noise = G.desc.noise_mix_type == FOT_SGAN_NOISE_GLOBAL;
        if (nd > 0 && !noise && (p->noise_kind <= FOT_NOISE_RAW || p->noise_kind >= FOT_NOISE_KINDS)) return fail(h, FOT_ERR_INVALID, who + "noise_kind");
        if ((int64_t)p->win_id0 + W > (int64_t)INT32_MAX) return fail(h, FOT_ERR_INVALID, who + "win_id0 + n_windows exceeds the counter's slot word");
    }
    int widest = 0;
    { const int bad = ol_check_table(p->n_frames, p->n_cols, W, obs_len, pred_len, win_frame0, ped_off, row_col, &widest, &why); if (bad) return refuse(bad, why); }
    const int max_rows = p->max_rows > 0 ? p->max_rows : OL_DEFAULT_MAX_ROWS;
    if (widest > max_rows) return fail(h, FOT_ERR_INVALID, who + "max_rows lies below the largest window");
    const int n_dense = resample_n_dense(p->dt, p->dt, (double)pred_len * p->dt, pred_len);
    if (!ps_horizon_fits(1, pred_len, n_dense, 0) || n_dense > FOT_MAX_NT) return fail(h, FOT_ERR_INVALID, who + "dt: the dense grid does not hold pred_len steps");
    const int R_all = ped_off[W];
    const size_t elem = p->scene_dtype == FOT_F32 ? 4 : 8;
    if (R_all > 0 && !scene) return fail(h, FOT_ERR_INVALID, who + "scene is NULL");
    if (R_all > 0 && (p->flags & FOT_OPENLOOP_SCENE_DEVICE) && ((uintptr_t)scene % (2 * elem)) != 0) return fail(h, FOT_ERR_INVALID, who + "a device scene is aligned to one point");
    OlTotals tot = ol_totals_zero();
    if (W == 0) { std::memcpy(totals, &tot, sizeof tot); return FOT_OK; }
    // the chunks: runs of whole windows of at most max_rows rows
    std::vector<int32_t> chunk_w;                                  // first window of every chunk, then W
    int cap_rows = 0, cap_win = 0;
    for (int64_t w0 = 0; w0 < W;) {
        const int64_t w1 = ol_chunk_end(ped_off, W, w0, max_rows);
        chunk_w.push_back((int32_t)w0);
        cap_rows = std::max(cap_rows, ped_off[w1] - ped_off[w0]);
        cap_win = std::max(cap_win, (int)(w1 - w0));
        w0 = w1;
    }
    const int n_chunks = (int)chunk_w.size();
    chunk_w.push_back(W);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    fot_handle::OpenLoop &O = h->ol;
    // the call's tables, built in pinned memory and copied to HBM once: per row its column, first frame, window within
    // its chunk, index within its window and noise slot; a run of zeros (the noise's step word, a scene row's index); per
    // window its noise slot and its origin; per chunk the windows' first rows and first points, relative to the chunk
    const size_t R_al = align256(sizeof(int32_t) * (size_t)std::max(R_all, 1)), W_al = align256(sizeof(int32_t) * (size_t)W);
    const size_t zero_al = std::max(R_al, W_al), off_al = align256(sizeof(int32_t) * ((size_t)W + n_chunks));
    const size_t blk_al = align256(sizeof(int64_t) * ((size_t)W + n_chunks)), desc_al = align256(sizeof(PredOriginDev) * (size_t)W);
    const size_t tab_bytes = 5 * R_al + zero_al + W_al + off_al + blk_al + desc_al;
    HIP_TRY(h, hipStreamSynchronize(h->stream));                   // (the pinned tables: nothing of an earlier call reads them)
    HIP_TRY(h, O.hTab.ensure(tab_bytes));
    HIP_TRY(h, O.dTab.ensure(tab_bytes));
    HIP_TRY(h, O.hRec.ensure(sizeof(fot_pred_score) * (size_t)W));
    char *ht = (char *)O.hTab.p;
    int32_t *t_col = (int32_t *)ht, *t_f0 = (int32_t *)(ht + R_al), *t_win = (int32_t *)(ht + 2 * R_al);
    int32_t *t_idx = (int32_t *)(ht + 3 * R_al), *t_slot = (int32_t *)(ht + 4 * R_al), *t_zero = (int32_t *)(ht + 5 * R_al);
    int32_t *t_wslot = (int32_t *)(ht + 5 * R_al + zero_al), *t_off = (int32_t *)(ht + 5 * R_al + zero_al + W_al);
    int64_t *t_blk = (int64_t *)(ht + 5 * R_al + zero_al + W_al + off_al);
    PredOriginDev *t_desc = (PredOriginDev *)(ht + 5 * R_al + zero_al + W_al + off_al + blk_al);
    std::memset(t_zero, 0, zero_al);
    if (R_all > 0) std::memcpy(t_col, row_col, sizeof(int32_t) * (size_t)R_all);
    const double scott = ps_scott(S);
    for (int c = 0; c < n_chunks; ++c) {
        const int w0 = chunk_w[(size_t)c], w1 = chunk_w[(size_t)c + 1], r0 = ped_off[w0];
        for (int w = w0; w <= w1; ++w) {                           // (w1: the chunk's end)
            t_off[w + c] = ped_off[w] - r0;
            t_blk[w + c] = (int64_t)S * (ped_off[w] - r0) * n_dense;
        }
        for (int w = w0; w < w1; ++w) {
            const int P = ped_off[w + 1] - ped_off[w];
            t_wslot[w] = p->win_id0 + w;
            t_desc[w] = PredOriginDev{ t_blk[w + c], (int64_t)(ped_off[w] - r0), scott, S, P, n_dense, 0, 0, 0 };
            for (int q = 0; q < P; ++q) {
                const int r = ped_off[w] + q;
                t_f0[r] = win_frame0[w]; t_win[r] = w - w0; t_idx[r] = q; t_slot[r] = p->win_id0 + w;
            }
        }
    }
    // the work arrays of the largest chunk
    HIP_TRY(h, O.dObs.ensure(sizeof(float) * 2 * (size_t)obs_len * std::max(cap_rows, 1)));
    HIP_TRY(h, O.dAnchor.ensure(sizeof(double) * 2 * (size_t)std::max(cap_rows, 1)));
    HIP_TRY(h, O.dTruth.ensure(sizeof(double) * 2 * (size_t)std::max(cap_rows, 1) * pred_len));
    HIP_TRY(h, O.dDyn.ensure(sizeof(double) * 2 * (size_t)S * std::max(cap_rows, 1) * n_dense));
    const bool with_noise = !cv && nd > 0;
    if (!cv && cap_rows > 0) {
        HIP_TRY(h, O.dRaw.ensure(sizeof(float) * 2 * (size_t)S * pred_len * cap_rows));
        if (with_noise) HIP_TRY(h, O.dNoise.ensure(sizeof(float) * (size_t)S * (global_noise ? cap_win : cap_rows) * nd));
        { int r = sgan_reserve(h, p->model, cap_rows, S); if (r != FOT_OK) return r; }
    }
    const size_t noise_rows_all = global_noise ? (size_t)W : (size_t)R_all;
    const bool given_noise = with_noise && noise && noise_rows_all > 0;
    const bool noise_up = given_noise && !(p->flags & FOT_OPENLOOP_NOISE_DEVICE);
    const size_t scene_bytes = elem * 2 * (size_t)p->n_frames * (size_t)p->n_cols;
    const bool scene_up = R_all > 0 && !(p->flags & FOT_OPENLOOP_SCENE_DEVICE);
    if (scene_up) HIP_TRY(h, O.dScene.ensure(scene_bytes));
    if (noise_up) HIP_TRY(h, O.dNoiseAll.ensure(sizeof(float) * (size_t)S * noise_rows_all * nd));
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipMemcpyAsync(O.dTab.p, O.hTab.p, tab_bytes, hipMemcpyHostToDevice, st));
    const void *d_scene = scene;
    if (scene_up) { HIP_TRY(h, hipMemcpyAsync(O.dScene.p, scene, scene_bytes, hipMemcpyHostToDevice, st)); d_scene = O.dScene.p; }
    const float *d_noise_all = (const float *)noise;
    if (noise_up) {
        HIP_TRY(h, hipMemcpyAsync(O.dNoiseAll.p, noise, sizeof(float) * (size_t)S * noise_rows_all * nd, hipMemcpyHostToDevice, st));
        d_noise_all = O.dNoiseAll.as<float>();
    }
    const char *dt_ = (const char *)O.dTab.p;
    auto dev = [&](const void *host_ptr) { return dt_ + ((const char *)host_ptr - ht); };
    const int32_t *d_col = (const int32_t *)dev(t_col), *d_f0 = (const int32_t *)dev(t_f0), *d_win = (const int32_t *)dev(t_win);
    const int32_t *d_idx = (const int32_t *)dev(t_idx), *d_slot = (const int32_t *)dev(t_slot), *d_zero = (const int32_t *)dev(t_zero);
    const int32_t *d_wslot = (const int32_t *)dev(t_wslot), *d_off = (const int32_t *)dev(t_off);
    const int64_t *d_blk = (const int64_t *)dev(t_blk);
    const PredOriginDev *d_desc = (const PredOriginDev *)dev(t_desc);
    fot_pred_score *rec = (fot_pred_score *)O.hRec.p;
    // per chunk: gather -> noise -> generator | constant velocity -> resampler -> scorer, nothing synchronised in between
    for (int c = 0; c < n_chunks; ++c) {
        const int w0 = chunk_w[(size_t)c], w1 = chunk_w[(size_t)c + 1], nw = w1 - w0, r0 = ped_off[w0], R = ped_off[w1] - r0;
        if (R > 0) {
            OpenLoopRows g{};
            g.scene = d_scene; g.row_col = d_col + r0; g.row_f0 = d_f0 + r0;
            g.dtype = p->scene_dtype; g.n_cols = p->n_cols; g.rows = R; g.obs_len = obs_len; g.pred_len = pred_len;
            g.obs = O.dObs.as<float2>(); g.anchor = O.dAnchor.as<double2>(); g.truth = O.dTruth.as<double2>();
            LAUNCH_TRY(h, launch_openloop_rows(g, st));
            if (cv) {
                // k_resample's float32-observation path (cv = 2): the velocity from the window's last two rows
                const float *prev = obs_len >= 2 ? O.dObs.as<float>() + 2 * (size_t)(obs_len - 2) * R : nullptr;
                LAUNCH_TRY(h, launch_resample(p->dt, p->dt, 0.0, 1, pred_len, R, n_dense, 1, 0, 2, prev, FOT_F32, O.dAnchor.as<double>(),
                                              nullptr, O.dDyn.p, FOT_F64, 0, st, d_win + r0, d_off + w0 + c, d_blk + w0 + c));
            } else {
                if (given_noise) {                                 // the chunk's rows of every sample of the call's tensor
                    const size_t first = global_noise ? (size_t)w0 : (size_t)r0, n = global_noise ? (size_t)nw : (size_t)R;
                    HIP_TRY(h, hipMemcpy2DAsync(O.dNoise.p, sizeof(float) * n * nd, d_noise_all + first * nd, sizeof(float) * noise_rows_all * nd,
                                                sizeof(float) * n * nd, (size_t)S, hipMemcpyDeviceToDevice, st));
                } else if (with_noise) {
                    SgNoise a{};
                    a.seed = p->seed; a.kind = p->noise_kind; a.S = S; a.rows = global_noise ? nw : R; a.nd = nd; a.n_blk = (nd + 3) / 4;
                    a.slot = global_noise ? d_wslot + w0 : d_slot + r0; a.step = d_zero; a.index = global_noise ? d_zero : d_idx + r0;
                    a.out = (uint32_t *)O.dNoise.p;
                    LAUNCH_TRY(h, launch_sgan_noise(a, st));
                }
                { int r = sgan_enqueue(h, p->model, nw, R, S, d_off + w0 + c, global_noise && nd > 0 ? d_win + r0 : nullptr, O.dObs.as<float>(),
                                       O.dNoise.as<float>(), O.dRaw.as<float>(), st); if (r != FOT_OK) return r; }
                if (raw_out)
                    HIP_TRY(h, hipMemcpy2DAsync((float *)raw_out + 2 * (size_t)r0, sizeof(float) * 2 * (size_t)R_all, O.dRaw.p, sizeof(float) * 2 * (size_t)R,
                                                sizeof(float) * 2 * (size_t)R, (size_t)S * pred_len, hipMemcpyDeviceToHost, st));
                LAUNCH_TRY(h, launch_resample(p->dt, p->dt, 0.0, S, pred_len, R, n_dense, 1, 0, 0, O.dRaw.p, FOT_F32, O.dAnchor.as<double>(),
                                              nullptr, O.dDyn.p, FOT_F64, 0, st, d_win + r0, d_off + w0 + c, d_blk + w0 + c));
            }
        }
        LAUNCH_TRY(h, launch_pred_scores(d_desc + w0, nw, O.dDyn.p, FOT_F64, 1, pred_len, O.dTruth.as<double>(), rec + w0, st));
    }
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));
    for (int w = 0; w < W; ++w)
        ol_fold(tot, rec[w].ade_scene, rec[w].fde_scene, rec[w].ade_agent_sum, rec[w].fde_agent_sum, rec[w].log_lik_sum, rec[w].n_peds,
                rec[w].nll_count, rec[w].flags);
    if (records) std::memcpy(records, rec, sizeof(fot_pred_score) * (size_t)W);
    std::memcpy(totals, &tot, sizeof tot);
    return FOT_OK;
}

// ---- footprint re-verification of trajectories (include/fot.h; the shared arithmetic and checks: fot_footprint_obs.hpp) ------
int fot_footprint_recheck(fot_handle *h, const fot_footprint_geom *geom, int32_t n_traj, const int32_t *step_off,
                          const double *xy, const double *yaw, const int32_t *ped_off, const double *ped_xy,
                          fot_footprint_step *series, double *yaw_out, fot_footprint_obs *out)
{
    static_assert(sizeof(FpoStep) == sizeof(fot_footprint_step) && sizeof(FpoRecord) == sizeof(fot_footprint_obs) &&
                  offsetof(FpoRecord, steps_with_peds) == offsetof(fot_footprint_obs, steps_with_peds),
                  "FpoStep / FpoRecord are fot_footprint_step / fot_footprint_obs");
    if (!h) return FOT_ERR_INVALID;
    const std::string who = "fot_footprint_recheck: ";
    if (!geom || !out) return fail(h, FOT_ERR_INVALID, who + "geom / out is NULL");
    const char *why = "";
    if (fpo_check_geom(geom->vehicle_length, geom->vehicle_width, geom->ped_radius, geom->legacy_radius, geom->n_circles, &why))
        return fail(h, FOT_ERR_INVALID, who + why);
    if (fpo_check_tables(n_traj, step_off, ped_off, yaw != nullptr, &why)) return fail(h, FOT_ERR_INVALID, who + why);
    if (n_traj == 0) return FOT_OK;
    const size_t steps = (size_t)step_off[n_traj], n_ped = (size_t)ped_off[steps];
    if (!xy || (n_ped > 0 && !ped_xy)) return fail(h, FOT_ERR_INVALID, who + "xy / ped_xy is NULL");
    // the inputs as one block: the geometry | step_off | ped_off | xy | yaw (if given) | ped_xy
    const size_t geom_b = align256(sizeof(FpoGeom)), soff_b = align256(sizeof(int32_t) * ((size_t)n_traj + 1));
    const size_t poff_b = align256(sizeof(int32_t) * (steps + 1)), xy_b = align256(sizeof(double) * 2 * steps);
    const size_t yaw_b = yaw ? align256(sizeof(double) * steps) : 0, ped_b = align256(sizeof(double) * 2 * std::max<size_t>(n_ped, 1));
    const size_t tab_b = soff_b + poff_b + xy_b + yaw_b + ped_b, out_b = sizeof(FpoRecord) * (size_t)n_traj;
    const bool small = geom_b + tab_b <= SMALL_CALL_BYTES && out_b <= SMALL_CALL_BYTES;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    fot_handle::Footprint &F = h->fp;
    // the geometry always goes through the pinned block; a small call's tables too: the kernels read them in place
    HIP_TRY(h, h->hSmallIn.ensure(geom_b + (small ? tab_b : 0)));
    if (small) HIP_TRY(h, h->hSmallOut.ensure(out_b));
    else { HIP_TRY(h, F.dIn.ensure(tab_b)); HIP_TRY(h, F.dOut.ensure(out_b)); }
    if (!yaw) HIP_TRY(h, F.dYaw.ensure(sizeof(double) * steps));
    HIP_TRY(h, F.dSeries.ensure(sizeof(FpoStep) * steps));
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const FpoGeom G = fpo_geom(geom->vehicle_length, geom->vehicle_width, geom->ped_radius, geom->legacy_radius, geom->n_circles);
    std::memcpy(h->hSmallIn.p, &G, sizeof G);
    const FpoGeom *d_geom = (const FpoGeom *)h->hSmallIn.p;
    char *base = small ? (char *)h->hSmallIn.p + geom_b : (char *)F.dIn.p;
    char *b_soff = base, *b_poff = b_soff + soff_b, *b_xy = b_poff + poff_b, *b_yaw = b_xy + xy_b, *b_ped = b_yaw + yaw_b;
    auto put = [&](char *dst, const void *src, size_t bytes) -> hipError_t {
        if (bytes == 0) return hipSuccess;
        if (small) { std::memcpy(dst, src, bytes); return hipSuccess; }
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    };
    HIP_TRY(h, put(b_soff, step_off, sizeof(int32_t) * ((size_t)n_traj + 1)));
    HIP_TRY(h, put(b_poff, ped_off, sizeof(int32_t) * (steps + 1)));
    HIP_TRY(h, put(b_xy, xy, sizeof(double) * 2 * steps));
    if (yaw) HIP_TRY(h, put(b_yaw, yaw, sizeof(double) * steps));
    HIP_TRY(h, put(b_ped, ped_xy, sizeof(double) * 2 * n_ped));
    const double *d_yaw = (const double *)b_yaw;
    if (!yaw) {
        LAUNCH_TRY(h, launch_footprint_yaw(n_traj, (const int32_t *)b_soff, (const double *)b_xy, F.dYaw.as<double>(), st));
        d_yaw = F.dYaw.as<double>();
    }
    FpoRecord *d_out = small ? (FpoRecord *)h->hSmallOut.p : F.dOut.as<FpoRecord>();
    LAUNCH_TRY(h, launch_footprint_steps(d_geom, (int)steps, (const double *)b_xy, 2, d_yaw, 1, (const int32_t *)b_poff,
                                         (const double *)b_ped, F.dSeries.as<FpoStep>(), st));
    LAUNCH_TRY(h, launch_footprint_fold(d_geom, n_traj, (const int32_t *)b_soff, (const int32_t *)b_poff, F.dSeries.as<FpoStep>(),
                                        d_out, st));
    if (series) HIP_TRY(h, hipMemcpyAsync(series, F.dSeries.p, sizeof(FpoStep) * steps, hipMemcpyDeviceToHost, st));
    if (yaw_out && !yaw) HIP_TRY(h, hipMemcpyAsync(yaw_out, F.dYaw.p, sizeof(double) * steps, hipMemcpyDeviceToHost, st));
    if (!small) HIP_TRY(h, hipMemcpyAsync(out, F.dOut.p, out_b, hipMemcpyDeviceToHost, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));
    if (small) std::memcpy(out, h->hSmallOut.p, out_b);
    if (yaw_out && yaw && yaw_out != yaw) std::memcpy(yaw_out, yaw, sizeof(double) * steps);
    return FOT_OK;
}

// ---- fidelity statistics of encounters (include/fot.h; the shared arithmetic and checks: fot_fidelity.hpp) ---------------------
int fot_fidelity_eval(fot_handle *h, const fot_fidelity_params *p, int32_t n_enc, const int32_t *step_off, const int32_t *n_ped,
                      const double *dt, const double *ego_xy, const double *ped_xy, const double *ped_vel,
                      const double *truth_xy, double *sep_series, double *onset_dist, int32_t *onset_step,
                      fot_fidelity_enc *out)
{
    static_assert(sizeof(FidParams) == sizeof(fot_fidelity_params) && sizeof(FidEnc) == sizeof(fot_fidelity_enc) &&
                  offsetof(FidEnc, closest_step) == offsetof(fot_fidelity_enc, closest_step) &&
                  offsetof(FidEnc, err_count) == offsetof(fot_fidelity_enc, err_count),
                  "FidParams / FidEnc are fot_fidelity_params / fot_fidelity_enc");
    if (!h) return FOT_ERR_INVALID;
    const std::string who = "fot_fidelity_eval: ";
    if (!p || !ego_xy || !ped_xy || !out) return fail(h, FOT_ERR_INVALID, who + "p / ego_xy / ped_xy / out is NULL");
    FidParams P;
    P.accel_threshold = p->accel_threshold; P.max_distance = p->max_distance; P.interaction_distance = p->interaction_distance;
    const char *why = "";
    if (fid_check_params(P, &why) || fid_check_tables(n_enc, step_off, n_ped, dt, &why)) return fail(h, FOT_ERR_INVALID, who + why);
    if (n_enc == 0) return FOT_OK;
    // the row and pedestrian offsets, in 64 bits: an encounter's rows are T_e N_e
    std::vector<int64_t> off64(2 * ((size_t)n_enc + 1));
    int64_t *row_off = off64.data(), *ped_base = row_off + n_enc + 1;
    row_off[0] = ped_base[0] = 0;
    for (int e = 0; e < n_enc; ++e) {
        row_off[e + 1] = row_off[e] + (int64_t)(step_off[e + 1] - step_off[e]) * n_ped[e];
        ped_base[e + 1] = ped_base[e] + n_ped[e];
    }
    const size_t ne = (size_t)n_enc, steps = (size_t)step_off[n_enc], rows = (size_t)row_off[n_enc], peds = (size_t)ped_base[n_enc];
    // the inputs as one block: step_off | n_ped | dt | row_off, ped_base | ego | ped_xy | ped_vel | truth
    const size_t soff_b = align256(sizeof(int32_t) * (ne + 1)), nped_b = align256(sizeof(int32_t) * ne);
    const size_t dt_b = align256(sizeof(double) * ne), o64_b = align256(sizeof(int64_t) * off64.size());
    const size_t ego_b = align256(sizeof(double) * 2 * steps), arr_b = align256(sizeof(double) * 2 * std::max<size_t>(rows, 1));
    const size_t in_b = soff_b + nped_b + dt_b + o64_b + ego_b + arr_b * (1 + (ped_vel ? 1 : 0) + (truth_xy ? 1 : 0));
    // what the kernels write: series | onset_dist | ped_sum | onset_step | ped_keep | out
    const size_t ser_b = align256(sizeof(double) * steps), pd_b = align256(sizeof(double) * std::max<size_t>(peds, 1));
    const size_t pi_b = align256(sizeof(int32_t) * std::max<size_t>(peds, 1)), rec_b = sizeof(FidEnc) * ne;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    fot_handle::Fidelity &F = h->fid;
    HIP_TRY(h, F.dIn.ensure(in_b));
    HIP_TRY(h, F.dOut.ensure(ser_b + 2 * pd_b + 2 * pi_b + rec_b));
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    char *b_soff = (char *)F.dIn.p, *b_nped = b_soff + soff_b, *b_dt = b_nped + nped_b, *b_o64 = b_dt + dt_b;
    char *b_ego = b_o64 + o64_b, *b_xy = b_ego + ego_b, *b_vel = b_xy + arr_b, *b_truth = b_vel + (ped_vel ? arr_b : 0);
    auto put = [&](char *dst, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    HIP_TRY(h, put(b_soff, step_off, sizeof(int32_t) * (ne + 1)));
    HIP_TRY(h, put(b_nped, n_ped, sizeof(int32_t) * ne));
    HIP_TRY(h, put(b_dt, dt, sizeof(double) * ne));
    HIP_TRY(h, put(b_o64, off64.data(), sizeof(int64_t) * off64.size()));
    HIP_TRY(h, put(b_ego, ego_xy, sizeof(double) * 2 * steps));
    HIP_TRY(h, put(b_xy, ped_xy, sizeof(double) * 2 * rows));
    if (ped_vel) HIP_TRY(h, put(b_vel, ped_vel, sizeof(double) * 2 * rows));
    if (truth_xy) HIP_TRY(h, put(b_truth, truth_xy, sizeof(double) * 2 * rows));
    char *o_ser = (char *)F.dOut.p, *o_dist = o_ser + ser_b, *o_sum = o_dist + pd_b, *o_step = o_sum + pd_b;
    char *o_keep = o_step + pi_b, *o_rec = o_keep + pi_b;
    FidelityArgs A;
    A.n_enc = n_enc; A.n_steps = (int64_t)steps; A.n_peds = (int64_t)peds;
    A.step_off = (const int32_t *)b_soff; A.n_ped = (const int32_t *)b_nped; A.dt = (const double *)b_dt;
    A.row_off = (const int64_t *)b_o64; A.ped_base = A.row_off + n_enc + 1;
    A.ego = (const double *)b_ego; A.ped_xy = (const double *)b_xy;
    A.ped_vel = ped_vel ? (const double *)b_vel : nullptr; A.truth = truth_xy ? (const double *)b_truth : nullptr;
    A.p = P;
    A.series = (double *)o_ser; A.onset_dist = (double *)o_dist; A.ped_sum = (double *)o_sum;
    A.onset_step = (int32_t *)o_step; A.ped_keep = (int32_t *)o_keep; A.out = (FidEnc *)o_rec;
    LAUNCH_TRY(h, launch_fidelity(A, st));
    if (sep_series) HIP_TRY(h, hipMemcpyAsync(sep_series, o_ser, sizeof(double) * steps, hipMemcpyDeviceToHost, st));
    if (onset_dist && peds) HIP_TRY(h, hipMemcpyAsync(onset_dist, o_dist, sizeof(double) * peds, hipMemcpyDeviceToHost, st));
    if (onset_step && peds) HIP_TRY(h, hipMemcpyAsync(onset_step, o_step, sizeof(int32_t) * peds, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(out, o_rec, rec_b, hipMemcpyDeviceToHost, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));             // (off64 and the caller's arrays are read until here)
    return FOT_OK;
}

// ---- encounters cut out of a recorded clip (include/fot.h; the shared arithmetic and checks: fot_encounter.hpp) ---------------
int fot_encounters_extract(fot_handle *h, const fot_encounter_params *p, int32_t T, int32_t A, int32_t K, const double *ped_xy,
                           const double *ped_vel, const double *ego_xy, const double *ego_psi, const double *ego_vel,
                           int32_t max_spans, int64_t max_rows, int32_t *n_spans, int64_t *n_rows, fot_encounter_span *spans,
                           int32_t *cols, double *cruise, double *goals, double *onset_dist, int32_t *onset_step,
                           double *sep_series, int64_t max_steps)
{
    static_assert(sizeof(EncParams) == sizeof(fot_encounter_params) && sizeof(EncSpan) == sizeof(fot_encounter_span) &&
                  offsetof(EncParams, min_len) == offsetof(fot_encounter_params, min_len) &&
                  offsetof(EncSpan, real) == offsetof(fot_encounter_span, real) &&
                  offsetof(EncSpan, row_base) == offsetof(fot_encounter_span, row_base) &&
                  offsetof(EncSpan, min_col) == offsetof(fot_encounter_span, min_col),
                  "EncParams / EncSpan are fot_encounter_params / fot_encounter_span");
    if (!h) return FOT_ERR_INVALID;
    const std::string who = "fot_encounters_extract: ";
    if (!p || !n_spans || !n_rows || !spans || !cols) return fail(h, FOT_ERR_INVALID, who + "p / n_spans / n_rows / spans / cols is NULL");
    EncParams P;
    std::memcpy(&P, p, sizeof P);
    const char *why = "";
    if (enc_check_params(P, &why)) return fail(h, FOT_ERR_INVALID, who + why);
    if (T < 0 || A < 0 || K < 0 || max_spans < 0 || max_rows < 0 || (sep_series && max_steps < 0))
        return fail(h, FOT_ERR_INVALID, who + "a negative size or capacity");
    const bool cruise_on = P.cruise_mode != ENC_CRUISE_NONE, freewalk = P.cruise_mode == ENC_CRUISE_FREEWALK;
    const bool measure = (P.flags & ENC_MEASURE_REAL) != 0, on_device = (P.flags & ENC_SCENE_DEVICE) != 0;
    if (cruise_on && (!cruise || !goals)) return fail(h, FOT_ERR_INVALID, who + "cruise / goals is NULL with a cruise mode");
    const bool any = T > 0 && A > 0 && K > 0;
    if (any && (!ped_xy || !ego_xy || !ego_psi || !ego_vel)) return fail(h, FOT_ERR_INVALID, who + "ped_xy / ego_xy / ego_psi / ego_vel is NULL");
    if (on_device && (((uintptr_t)ped_xy | (uintptr_t)ped_vel) & 15)) return fail(h, FOT_ERR_INVALID, who + "a device scene is not aligned to 16 bytes");
    if (!any) { *n_spans = 0; *n_rows = 0; return FOT_OK; }
    // the candidate spans, and which of them go on to the device
    std::vector<EncSpan> rec;
    std::vector<int32_t> go_tab, go_rec;                           // [n_go][4]: vehicle, frame0, frame1, 0 | the span's record
    for (int32_t k = 0; k < K; ++k)
        enc_find_spans(T, ego_xy + 2 * (size_t)k * T, ego_psi + (size_t)k * T, ego_vel + (size_t)k * T, [&](int32_t f0, int32_t f1) {
            EncSpan s{};
            s.min_separation = NAN; s.real.closest = NAN; s.real.closest_step = -1; s.row_base = -1;
            s.status = ENC_SHORT; s.vehicle = k; s.frame0 = f0; s.frame1 = f1; s.min_step = -1; s.min_col = -1;
            if (f1 - f0 >= P.min_len) { go_tab.insert(go_tab.end(), { k, f0, f1, 0 }); go_rec.push_back((int32_t)rec.size()); }
            rec.push_back(s);
        });
    if (rec.size() > (size_t)max_spans) return fail(h, FOT_ERR_UNSUPPORTED, who + "needs max_spans >= " + std::to_string(rec.size()));
    const size_t n_go = go_rec.size();
    auto deliver = [&](int64_t rows) {
        if (!rec.empty()) std::memcpy(spans, rec.data(), sizeof(EncSpan) * rec.size());
        *n_spans = (int32_t)rec.size(); *n_rows = rows;
        return FOT_OK;
    };
    if (n_go == 0) return deliver(0);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    fot_handle::Encounters &E = h->enc;
    // the clip in HBM: a host scene is copied once (positions | velocities); the ego rows | the spans' table
    const size_t scene_b = align256(sizeof(double) * 2 * (size_t)T * A), ego_b = align256(sizeof(double) * 2 * (size_t)K * T);
    const size_t go_b = align256(sizeof(int32_t) * go_tab.size());
    const size_t col_b = align256(sizeof(EncCol) * n_go * A), cols_b = align256(sizeof(int32_t) * n_go * A), so_b = sizeof(EncSpanOut) * n_go;
    if (!on_device) HIP_TRY(h, E.dScene.ensure(scene_b * (ped_vel ? 2 : 1)));
    HIP_TRY(h, E.dIn.ensure(ego_b + go_b));
    HIP_TRY(h, E.dWork.ensure(col_b + cols_b + so_b));
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    EncScene S;
    S.T = T; S.A = A; S.dt = P.dt; S.ped_xy = ped_xy; S.ped_vel = ped_vel;
    if (!on_device) {
        char *d = (char *)E.dScene.p;
        HIP_TRY(h, hipMemcpyAsync(d, ped_xy, sizeof(double) * 2 * (size_t)T * A, hipMemcpyHostToDevice, st));
        S.ped_xy = (const double *)d;
        if (ped_vel) {
            HIP_TRY(h, hipMemcpyAsync(d + scene_b, ped_vel, sizeof(double) * 2 * (size_t)T * A, hipMemcpyHostToDevice, st));
            S.ped_vel = (const double *)(d + scene_b);
        }
    }
    char *b_ego = (char *)E.dIn.p, *b_go = b_ego + ego_b;
    HIP_TRY(h, hipMemcpyAsync(b_ego, ego_xy, sizeof(double) * 2 * (size_t)K * T, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(b_go, go_tab.data(), sizeof(int32_t) * go_tab.size(), hipMemcpyHostToDevice, st));
    S.ego_xy = (const double *)b_ego;
    char *w_col = (char *)E.dWork.p, *w_cols = w_col + col_b, *w_out = w_cols + cols_b;
    EncSpansArgs SA;
    SA.s = S; SA.n_go = (int32_t)n_go; SA.span = (const int32_t *)b_go;
    SA.col = (EncCol *)w_col; SA.cols = (int32_t *)w_cols; SA.out = (EncSpanOut *)w_out;
    LAUNCH_TRY(h, launch_enc_spans(SA, st));
    std::vector<EncSpanOut> so(n_go);
    HIP_TRY(h, hipMemcpyAsync(so.data(), w_out, so_b, hipMemcpyDeviceToHost, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));             // the first wait: the populations size everything below
    // the kept spans in fot_fidelity_eval's tables
    std::vector<int32_t> kept_tab, step_off(1, 0), n_ped;
    std::vector<int64_t> off64(1, 0), ped_base(1, 0);
    std::vector<int32_t> kept_rec;
    for (size_t g = 0; g < n_go; ++g) {
        EncSpan &s = rec[(size_t)go_rec[g]];
        const EncMin &m = so[g].m;
        s.n_ped = so[g].n_ped;
        s.min_separation = s.n_ped == 0 ? (double)INFINITY : m.nan ? (double)NAN : m.v;
        if (s.n_ped > 0 && !m.nan) { s.min_step = m.step; s.min_col = m.col; }
        s.status = enc_status(s.n_ped, s.min_separation, P.min_sep_threshold);
        if (s.status != ENC_KEPT) continue;
        const int64_t L = s.frame1 - s.frame0;
        if ((int64_t)step_off.back() + L > 0x7fffffffLL) return fail(h, FOT_ERR_UNSUPPORTED, who + "more kept steps than int32 offsets hold");
        s.row_base = ped_base.back();
        kept_tab.insert(kept_tab.end(), { s.vehicle, s.frame0, (int32_t)g, 0 });
        kept_rec.push_back(go_rec[g]);
        step_off.push_back(step_off.back() + (int32_t)L);
        n_ped.push_back(s.n_ped);
        off64.push_back(off64.back() + L * s.n_ped);
        ped_base.push_back(ped_base.back() + s.n_ped);
    }
    const size_t ne = kept_rec.size(), steps = (size_t)step_off.back(), cells = (size_t)off64.back(), rows = (size_t)ped_base.back();
    if ((int64_t)rows > max_rows) return fail(h, FOT_ERR_UNSUPPORTED, who + "needs max_rows >= " + std::to_string(rows));
    if (sep_series && measure && (int64_t)steps > max_steps) return fail(h, FOT_ERR_UNSUPPORTED, who + "needs max_steps >= " + std::to_string(steps));
    if (ne == 0) return deliver(0);
    // the tables as one block: kept | step_off | n_ped | dt | row_off, ped_base | the kept spans' ego rows
    off64.insert(off64.end(), ped_base.begin(), ped_base.end());
    std::vector<double> dts(ne, P.dt), ego_rows(2 * steps);
    for (size_t e = 0; e < ne; ++e) {
        const EncSpan &s = rec[(size_t)kept_rec[e]];
        std::memcpy(ego_rows.data() + 2 * (size_t)step_off[e], ego_xy + 2 * ((size_t)s.vehicle * T + s.frame0),
                    sizeof(double) * 2 * (size_t)(s.frame1 - s.frame0));
    }
    const size_t kt_b = align256(sizeof(int32_t) * kept_tab.size()), soff_b = align256(sizeof(int32_t) * (ne + 1));
    const size_t nped_b = align256(sizeof(int32_t) * ne), dt_b = align256(sizeof(double) * ne), o64_b = align256(sizeof(int64_t) * off64.size());
    const size_t egor_b = align256(sizeof(double) * 2 * steps);
    // what the kernels write: col_out | cruise | goals | series | onset_dist | onset_step | records
    const size_t ci_b = align256(sizeof(int32_t) * rows), rd_b = align256(sizeof(double) * rows), ser_b = align256(sizeof(double) * steps);
    const size_t frec_b = sizeof(FidEnc) * ne;
    HIP_TRY(h, E.dTab.ensure(kt_b + soff_b + nped_b + dt_b + o64_b + egor_b));
    if (measure) HIP_TRY(h, E.dPacked.ensure(sizeof(double) * 2 * cells));
    if (cruise_on) HIP_TRY(h, E.dSpeeds.ensure(align256(sizeof(double) * cells) * (freewalk ? 2 : 1)));
    HIP_TRY(h, E.dOut.ensure(ci_b + 3 * rd_b + ser_b + rd_b + ci_b + frec_b));
    char *t_kept = (char *)E.dTab.p, *t_soff = t_kept + kt_b, *t_nped = t_soff + soff_b, *t_dt = t_nped + nped_b, *t_o64 = t_dt + dt_b;
    char *t_ego = t_o64 + o64_b;
    HIP_TRY(h, hipMemcpyAsync(t_kept, kept_tab.data(), sizeof(int32_t) * kept_tab.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t_soff, step_off.data(), sizeof(int32_t) * (ne + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t_nped, n_ped.data(), sizeof(int32_t) * ne, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t_dt, dts.data(), sizeof(double) * ne, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t_o64, off64.data(), sizeof(int64_t) * off64.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t_ego, ego_rows.data(), sizeof(double) * 2 * steps, hipMemcpyHostToDevice, st));
    char *o_col = (char *)E.dOut.p, *o_cruise = o_col + ci_b, *o_goals = o_cruise + rd_b, *o_ser = o_goals + 2 * rd_b;
    char *o_dist = o_ser + ser_b, *o_step = o_dist + rd_b, *o_rec = o_step + ci_b;
    EncRowsArgs RA;
    RA.s = S; RA.p = P; RA.n_kept = (int32_t)ne; RA.n_rows = (int64_t)rows; RA.n_cells = (int64_t)cells;
    RA.kept = (const int32_t *)t_kept; RA.step_off = (const int32_t *)t_soff; RA.n_ped = (const int32_t *)t_nped;
    RA.row_off = (const int64_t *)t_o64; RA.ped_base = RA.row_off + ne + 1;
    RA.cols = (const int32_t *)w_cols;
    RA.packed_xy = measure ? E.dPacked.as<double>() : nullptr;
    RA.speeds = cruise_on ? E.dSpeeds.as<double>() : nullptr;
    RA.free_speeds = freewalk ? (double *)((char *)E.dSpeeds.p + align256(sizeof(double) * cells)) : nullptr;
    RA.col_out = (int32_t *)o_col; RA.cruise = (double *)o_cruise; RA.goals = (double *)o_goals;
    LAUNCH_TRY(h, launch_enc_rows(RA, st));
    std::vector<FidEnc> frec(measure ? ne : 0);
    if (measure) {
        FidelityArgs F;
        F.n_enc = (int32_t)ne; F.n_steps = (int64_t)steps; F.n_peds = (int64_t)rows;
        F.step_off = RA.step_off; F.n_ped = RA.n_ped; F.dt = (const double *)t_dt; F.row_off = RA.row_off; F.ped_base = RA.ped_base;
        F.ego = (const double *)t_ego; F.ped_xy = RA.packed_xy; F.ped_vel = nullptr; F.truth = nullptr;
        F.p.accel_threshold = P.accel_threshold; F.p.max_distance = P.max_distance; F.p.interaction_distance = NAN;
        F.series = (double *)o_ser; F.onset_dist = (double *)o_dist; F.ped_sum = nullptr; F.onset_step = (int32_t *)o_step;
        F.ped_keep = nullptr; F.out = (FidEnc *)o_rec;
        LAUNCH_TRY(h, launch_fidelity(F, st));
        HIP_TRY(h, hipMemcpyAsync(frec.data(), o_rec, frec_b, hipMemcpyDeviceToHost, st));
    }
    // everything below is written only now that the call can no longer be refused
    HIP_TRY(h, hipMemcpyAsync(cols, o_col, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, st));
    if (cruise_on) {
        HIP_TRY(h, hipMemcpyAsync(cruise, o_cruise, sizeof(double) * rows, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(goals, o_goals, sizeof(double) * 2 * rows, hipMemcpyDeviceToHost, st));
    }
    if (measure) {
        if (sep_series) HIP_TRY(h, hipMemcpyAsync(sep_series, o_ser, sizeof(double) * steps, hipMemcpyDeviceToHost, st));
        if (onset_dist) HIP_TRY(h, hipMemcpyAsync(onset_dist, o_dist, sizeof(double) * rows, hipMemcpyDeviceToHost, st));
        if (onset_step) HIP_TRY(h, hipMemcpyAsync(onset_step, o_step, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, st));
    }
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    HIP_TRY(h, hipStreamSynchronize(st));             // the second wait (the tables and ego_rows are read until here)
    for (size_t e = 0; e < frec.size(); ++e) rec[(size_t)kept_rec[e]].real = frec[e];
    return deliver((int64_t)rows);
}

}  // extern "C"
