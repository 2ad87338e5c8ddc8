// fot_openloop_emu.cpp -- fot_openloop_eval on the CPU: the table checks, the chunks and the fold of csrc/fot_openloop.hpp, the
// row gather of k_openloop_rows, the resampler's arithmetic (csrc/fot_math.hpp: ResampleAxis, k_resample's constant-velocity
// form) and the scorer's (csrc/fot_predscore.hpp: ps_origin), chunk by chunk as the host enqueues them.  The generator is
// not part of it: a Social-GAN case brings its raw samples.  Stand-alone (its own main), so that it can also be built with
// -fsanitize=address,undefined and run as it is.
//
//   fot_openloop_emu <case.bin> <out.bin>
// case.bin: int32 n_frames, n_cols, n_windows, dtype (0: float32, 1: float64), obs_len, pred_len, method (0: constant
// velocity, 1: raw samples given), S, max_rows (0: the default), 0; float64 dt; int32 win_frame0[n_windows], ped_off[n_windows
// + 1], row_col[rows]; the scene [n_frames][n_cols][2]; method 1: float32 raw[S][pred_len][rows][2].
// out.bin: int32 code (0, or 1 / 2: refused as FOT_ERR_INVALID / FOT_ERR_UNSUPPORTED), int32 n_windows; code 0: the totals
// (fot_openloop_totals, 64 bytes) and n_windows records of 56 bytes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_math.hpp"
#include "../../integrated_path_planning_amd/csrc/fot_openloop.hpp"
#include "../../integrated_path_planning_amd/csrc/fot_predscore.hpp"

namespace {

struct Record {                                   // fot_pred_score (include/fot.h)
    double ade_scene, fde_scene, ade_agent_sum, fde_agent_sum, log_lik_sum;
    int32_t n_peds, n_samples, nll_count, flags;
};
static_assert(sizeof(Record) == 56 && sizeof(fot::OlTotals) == 64, "fot_pred_score / fot_openloop_totals");

bool read_all(std::FILE *f, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

int finish(const char *path, int32_t code, int32_t n, const fot::OlTotals *tot, const std::vector<Record> *rec)
{
    std::FILE *o = std::fopen(path, "wb");
    if (!o) { std::perror(path); return 2; }
    const int32_t hd[2] = { code, n };
    bool ok = std::fwrite(hd, sizeof hd, 1, o) == 1;
    if (ok && code == 0) {
        ok = std::fwrite(tot, sizeof *tot, 1, o) == 1;
        if (ok && n > 0) ok = std::fwrite(rec->data(), sizeof(Record), (size_t)n, o) == (size_t)n;
    }
    std::fclose(o);
    if (!ok) { std::perror("write"); return 2; }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    using namespace fot;
    if (argc != 3) { std::fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    int32_t hd[10];
    double dt = 0.0;
    if (!read_all(in, hd, sizeof hd) || !read_all(in, &dt, sizeof dt)) { std::fprintf(stderr, "truncated header\n"); return 2; }
    const int n_frames = hd[0], n_cols = hd[1], W = hd[2], dtype = hd[3], obs_len = hd[4], pred_len = hd[5], method = hd[6], S = hd[7];
    if (W < 0 || W > (1 << 24) || (dtype != 0 && dtype != 1) || (method != 0 && method != 1) || hd[8] < 0 || !(dt > 0.0)) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int32_t> f0((size_t)W), off((size_t)W + 1);
    if (!read_all(in, f0.data(), 4 * f0.size()) || !read_all(in, off.data(), 4 * off.size())) { std::fprintf(stderr, "truncated tables\n"); return 2; }
    const char *why = "";
    int bad = ol_check_lengths(n_frames, n_cols, W, obs_len, pred_len, S, method == 0, &why);
    if (bad) { std::fprintf(stderr, "refused: %s\n", why); return finish(argv[2], bad, W, nullptr, nullptr); }
    // (row_col's length is ped_off's last entry: read only what a sane table announces)
    bool mono = off[0] == 0;
    for (int w = 0; w < W && mono; ++w) mono = off[(size_t)w + 1] >= off[(size_t)w];
    const int R_all = mono ? off[(size_t)W] : 0;
    std::vector<int32_t> col((size_t)R_all);
    if (!read_all(in, col.data(), 4 * col.size())) { std::fprintf(stderr, "truncated row_col\n"); return 2; }
    int widest = 0;
    bad = ol_check_table(n_frames, n_cols, W, obs_len, pred_len, f0.data(), off.data(), col.data(), &widest, &why);
    const int max_rows = hd[8] > 0 ? hd[8] : OL_DEFAULT_MAX_ROWS;
    if (!bad && widest > max_rows) { bad = OL_BAD_INVALID; why = "max_rows lies below the largest window"; }
    const int n_dense = resample_n_dense(dt, dt, (double)pred_len * dt, pred_len);
    if (!bad && (!ps_horizon_fits(1, pred_len, n_dense, 0) || n_dense > FOT_MAX_NT)) { bad = OL_BAD_INVALID; why = "dt"; }
    if (bad) { std::fprintf(stderr, "refused: %s\n", why); return finish(argv[2], bad, W, nullptr, nullptr); }
    const size_t n_pts = (size_t)n_frames * (size_t)n_cols;
    std::vector<float> s32(dtype == 0 ? 2 * n_pts : 0);
    std::vector<double> s64(dtype == 1 ? 2 * n_pts : 0);
    if (!read_all(in, dtype == 0 ? (void *)s32.data() : (void *)s64.data(), 2 * n_pts * (dtype == 0 ? 4 : 8))) { std::fprintf(stderr, "truncated scene\n"); return 2; }
    std::vector<float> raw(method == 1 ? (size_t)S * pred_len * R_all * 2 : 0);
    if (!read_all(in, raw.data(), 4 * raw.size())) { std::fprintf(stderr, "truncated samples\n"); return 2; }
    std::fclose(in);
    auto scene = [&](int64_t pt, int ax) { return dtype == 0 ? (double)s32[(size_t)(2 * pt + ax)] : s64[(size_t)(2 * pt + ax)]; };

    std::vector<Record> rec((size_t)W);
    OlTotals tot = ol_totals_zero();
    for (int64_t w0 = 0; w0 < W;) {
        const int64_t w1 = ol_chunk_end(off.data(), W, w0, max_rows);
        const int r0 = off[(size_t)w0], R = off[(size_t)w1] - r0;
        // k_openloop_rows: obs [obs_len][R][2] float32, anchor [R][2], truth [R][pred_len][2]
        std::vector<float> obs((size_t)obs_len * R * 2);
        std::vector<double> anchor((size_t)R * 2), truth((size_t)R * pred_len * 2);
        for (int64_t w = w0; w < w1; ++w)
            for (int r = off[(size_t)w] - r0; r < off[(size_t)w + 1] - r0; ++r)
                for (int ax = 0; ax < 2; ++ax) {
                    for (int t = 0; t < obs_len; ++t)
                        obs[((size_t)t * R + r) * 2 + ax] = ol_observe(scene(ol_scene_point(f0[(size_t)w], t, n_cols, col[(size_t)(r0 + r)]), ax));
                    anchor[(size_t)r * 2 + ax] = ol_anchor(scene(ol_scene_point(f0[(size_t)w], obs_len - 1, n_cols, col[(size_t)(r0 + r)]), ax));
                    for (int j = 0; j < pred_len; ++j)
                        truth[((size_t)r * pred_len + j) * 2 + ax] = scene(ol_scene_point(f0[(size_t)w], obs_len + j, n_cols, col[(size_t)(r0 + r)]), ax);
                }
        // k_resample per window block [S][P][n_dense][2], then k_pred_scores' arithmetic
        for (int64_t w = w0; w < w1; ++w) {
            const int p0 = off[(size_t)w] - r0, P = off[(size_t)w + 1] - off[(size_t)w];
            std::vector<double> dyn((size_t)S * P * n_dense * 2);
            for (int s = 0; s < S; ++s)
                for (int q = 0; q < P; ++q)
                    for (int ax = 0; ax < 2; ++ax) {
                        double *dst = &dyn[(((size_t)s * P + q) * n_dense) * 2 + ax];
                        const int r = p0 + q;
                        if (method == 0) {                           // cv = 2: the velocity in float32
                            const double cur = anchor[(size_t)r * 2 + ax];
                            double vel = 0.0;
                            if (obs_len >= 2) vel = (double)(((float)cur - obs[((size_t)(obs_len - 2) * R + r) * 2 + ax]) / (float)dt);
                            for (int i = 0; i < n_dense; ++i) {
                                const double t = (dt + (double)i * dt) + 0.0;
                                dst[2 * i] = cur + vel * t;
                            }
                            continue;
                        }
                        ResampleAxis A;
                        A.sgan_dt = dt; A.staleness = 0.0; A.first_k = 0;
                        int n = 0;
                        A.co[n++] = anchor[(size_t)r * 2 + ax];
                        for (int k = 0; k < pred_len; ++k) A.co[n++] = (double)raw[((((size_t)s * pred_len + k) * R_all) + r0 + r) * 2 + ax];
                        A.n_src = n;
                        const bool constant = A.all_close(A.co[0]) || A.all_close(0.0);
                        const double v_tail = A.tail_velocity();
                        for (int i = 0; i < n_dense; ++i) dst[2 * i] = A.at(dt + (double)i * dt, constant, v_tail);
                    }
            auto at = [&](int s, int q, int k, int ax) { return dyn[(((size_t)s * P + q) * n_dense + k) * 2 + ax]; };
            const PredScoreTerms t = ps_origin(S, P, 1, pred_len, at, truth.data() + (size_t)p0 * pred_len * 2);
            rec[(size_t)w] = Record{ t.ade_scene, t.fde_scene, t.ade_agent_sum, t.fde_agent_sum, t.log_lik_sum,
                                     t.n_peds, t.n_samples, t.nll_count, t.flags };
        }
        w0 = w1;
    }
    for (int w = 0; w < W; ++w) {
        const Record &r = rec[(size_t)w];
        ol_fold(tot, r.ade_scene, r.fde_scene, r.ade_agent_sum, r.fde_agent_sum, r.log_lik_sum, r.n_peds, r.nll_count, r.flags);
    }
    return finish(argv[2], 0, W, &tot, &rec);
}
