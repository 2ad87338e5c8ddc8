// fot_fidelity_emu.cpp -- fot_fidelity_eval on the CPU: the checks, the separation, the onset walk with its window of three
// velocities, the per-pedestrian error and the fold of csrc/fot_fidelity.hpp, in the shape the kernels give them (one
// pedestrian, one step, one encounter at a time; the fold's joins in the order of a 64-lane butterfly).  Stand-alone (its
// own main), so that it can also be built with -fsanitize=address,undefined and run as it is.
//
//   fot_fidelity_emu <case.bin> <out.bin>
// case.bin: float64 accel_threshold, max_distance, interaction_distance; int32 n_enc, have_vel, have_truth, 0; int32
// step_off[n_enc + 1], n_ped[n_enc]; float64 dt[n_enc], ego[steps][2], ped_xy[rows][2], have_vel: ped_vel[rows][2],
// have_truth: truth[rows][2].
// out.bin: int32 code (0, or 1: refused as FOT_ERR_INVALID), n_enc, steps, sum N; code 0: n_enc records of 32 bytes
// (fot_fidelity_enc), float64 series[steps], onset_dist[sum N], away[sum N] (the value that crossed the threshold),
// int32 onset_step[sum N].
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_fidelity.hpp"

namespace {

static_assert(sizeof(fot::FidEnc) == 32 && sizeof(fot::FidParams) == 24, "fot_fidelity_enc / fot_fidelity_params");

bool read_all(std::FILE *f, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }
bool write_all(std::FILE *f, const void *src, size_t bytes) { return bytes == 0 || std::fwrite(src, 1, bytes, f) == bytes; }

int refuse(const char *path, int32_t n_enc, const char *why)
{
    std::fprintf(stderr, "refused: %s\n", why);
    std::FILE *o = std::fopen(path, "wb");
    if (!o) { std::perror(path); return 2; }
    const int32_t hd[4] = { 1, n_enc, 0, 0 };
    const bool ok = write_all(o, hd, sizeof hd);
    std::fclose(o);
    return ok ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv)
{
    using namespace fot;
    if (argc != 3) { std::fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    FidParams P;
    int32_t hd[4];
    if (!read_all(in, &P, sizeof P) || !read_all(in, hd, sizeof hd)) { std::fprintf(stderr, "truncated header\n"); return 2; }
    const int n_enc = hd[0], have_vel = hd[1], have_truth = hd[2];
    if (n_enc < -1 || n_enc > (1 << 24) || (have_vel | have_truth) & ~1) { std::fprintf(stderr, "bad header\n"); return 2; }
    const char *why = "";
    if (fid_check_params(P, &why)) return refuse(argv[2], n_enc, why);
    if (n_enc < 0) return refuse(argv[2], n_enc, "n_enc is negative");
    const size_t ne = (size_t)n_enc;
    std::vector<int32_t> step_off(ne + 1), n_ped(ne + 1);        // (one spare entry: never a NULL table, also with n_enc == 0)
    std::vector<double> dt(ne + 1);
    if (!read_all(in, step_off.data(), 4 * (ne + 1)) || !read_all(in, n_ped.data(), 4 * ne) || !read_all(in, dt.data(), 8 * ne)) {
        std::fprintf(stderr, "truncated tables\n");
        return 2;
    }
    // (the arrays' lengths follow from the tables: read only what sane tables announce)
    if (fid_check_tables(n_enc, step_off.data(), n_ped.data(), dt.data(), &why)) return refuse(argv[2], n_enc, why);
    std::vector<int64_t> row_off(ne + 1, 0), ped_base(ne + 1, 0);
    for (size_t e = 0; e < ne; ++e) {
        row_off[e + 1] = row_off[e] + (int64_t)(step_off[e + 1] - step_off[e]) * n_ped[e];
        ped_base[e + 1] = ped_base[e] + n_ped[e];
    }
    const size_t steps = (size_t)step_off[ne], rows = (size_t)row_off[ne], peds = (size_t)ped_base[ne];
    std::vector<double> ego(2 * steps), xy(2 * rows), vel(have_vel ? 2 * rows : 0), truth(have_truth ? 2 * rows : 0);
    if (!read_all(in, ego.data(), 8 * ego.size()) || !read_all(in, xy.data(), 8 * xy.size()) ||
        !read_all(in, vel.data(), 8 * vel.size()) || !read_all(in, truth.data(), 8 * truth.size())) {
        std::fprintf(stderr, "truncated arrays\n");
        return 2;
    }
    std::fclose(in);

    std::vector<double> series(steps), onset_dist(peds), away(peds), ped_sum(peds);
    std::vector<int32_t> onset_step(peds), ped_keep(peds);
    std::vector<FidEnc> rec(ne);
    for (size_t e = 0; e < ne; ++e) {
        const int s0 = step_off[e], T = step_off[e + 1] - s0, N = n_ped[e];
        const double *eg = ego.data() + 2 * (size_t)s0;
        auto egof = [&](int t, int c) { return eg[2 * t + c]; };
        // k_fidelity_peds: one pedestrian at a time
        for (int j = 0; j < N; ++j) {
            const size_t g = (size_t)ped_base[e] + (size_t)j, first = 2 * ((size_t)row_off[e] + (size_t)j), stride = 2 * (size_t)N;
            const double *p = xy.data() + first;
            auto pos = [&](int t, int c) { return p[(size_t)t * stride + (size_t)c]; };
            if (have_vel) {
                const double *v = vel.data() + first;
                auto velf = [&](int t, int c) { return v[(size_t)t * stride + (size_t)c]; };
                fid_onset(pos, velf, egof, T, dt[e], P, &onset_step[g], &onset_dist[g], &away[g]);
            } else {
                auto velf = [&](int t, int c) { return fid_gradient([&](int s) { return p[(size_t)s * stride + (size_t)c]; }, t, T, dt[e]); };
                fid_onset(pos, velf, egof, T, dt[e], P, &onset_step[g], &onset_dist[g], &away[g]);
            }
            if (have_truth) {
                const double *q = truth.data() + first;
                auto tr = [&](int t, int c) { return q[(size_t)t * stride + (size_t)c]; };
                fid_ped_error(pos, tr, egof, T, P.interaction_distance, &ped_sum[g], &ped_keep[g]);
            }
        }
        // k_fidelity_series: one step at a time
        for (int t = 0; t < T; ++t) {
            const double *r = xy.data() + 2 * ((size_t)row_off[e] + (size_t)t * (size_t)N);
            series[(size_t)(s0 + t)] = fid_separation([&](int j, int c) { return r[2 * j + c]; }, N, eg[2 * t], eg[2 * t + 1]);
        }
        // k_fidelity_fold: 64 lanes stride over the steps, then the butterfly
        FidMin lane[64];
        for (int l = 0; l < 64; ++l) {
            lane[l] = fid_min_zero();
            for (int t = l; t < T; t += 64) lane[l] = fid_min_take(lane[l], series[(size_t)(s0 + t)], t);
        }
        for (int off = 32; off >= 1; off >>= 1) {
            FidMin next[64];
            for (int l = 0; l < 64; ++l) next[l] = fid_min_join(lane[l], lane[l ^ off]);
            std::memcpy(lane, next, sizeof next);
        }
        const size_t b = (size_t)ped_base[e];
        rec[e] = fid_record(lane[0], T, N, have_truth != 0, [&](int j) { return ped_sum[b + (size_t)j]; },
                            [&](int j) { return ped_keep[b + (size_t)j] != 0; }, [&](int j) { return onset_step[b + (size_t)j]; });
    }
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    const int32_t oh[4] = { 0, n_enc, (int32_t)steps, (int32_t)peds };
    const bool ok = write_all(o, oh, sizeof oh) && write_all(o, rec.data(), sizeof(FidEnc) * ne) && write_all(o, series.data(), 8 * steps) &&
                    write_all(o, onset_dist.data(), 8 * peds) && write_all(o, away.data(), 8 * peds) &&
                    write_all(o, onset_step.data(), 4 * peds);
    std::fclose(o);
    if (!ok) { std::perror("write"); return 2; }
    return 0;
}
