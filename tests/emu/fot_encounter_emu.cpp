// fot_encounter_emu.cpp -- fot_encounters_extract on the CPU: the checks and the candidate spans as the library's host code
// runs them, and csrc/fot_encounter.hpp's column walk, compaction, rank selection, cruise speeds and goals in the shape the
// kernels give them (a column's steps in ENC_STEP_WAVES shares; the present columns over 64 lanes and a butterfly; one
// kept pedestrian at a time), then fot_fidelity.hpp on the gathered encounters.  Stand-alone (its own main), so that it
// can also be built with -fsanitize=address,undefined and run as it is.
//
//   fot_encounter_emu <case.bin> <out.bin>
// case.bin: fot_encounter_params (72 bytes); int32 T, A, K, have_vel; float64 ped_xy[T][A][2], have_vel: ped_vel[T][A][2],
// ego_xy[K][T][2], ego_psi[K][T], ego_vel[K][T].
// out.bin: int32 code (0, or 1: refused as FOT_ERR_INVALID), n_spans; int64 n_rows, n_steps; code 0: n_spans records of 80
// bytes (fot_encounter_span), int32 cols[n_rows], float64 cruise[n_rows], goals[n_rows][2], onset_dist[n_rows], int32
// onset_step[n_rows], float64 series[n_steps] (what a mode or flag leaves out: NaN / -1).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_encounter.hpp"

namespace {

static_assert(sizeof(fot::EncParams) == 72 && sizeof(fot::EncSpan) == 80, "fot_encounter_params / fot_encounter_span");

bool read_all(std::FILE *f, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }
bool write_all(std::FILE *f, const void *src, size_t bytes) { return bytes == 0 || std::fwrite(src, 1, bytes, f) == bytes; }

int refuse(const char *path, const char *why)
{
    std::fprintf(stderr, "refused: %s\n", why);
    std::FILE *o = std::fopen(path, "wb");
    if (!o) { std::perror(path); return 2; }
    const int32_t hd[2] = { 1, 0 };
    const int64_t hq[2] = { 0, 0 };
    const bool ok = write_all(o, hd, sizeof hd) && write_all(o, hq, sizeof hq);
    std::fclose(o);
    return ok ? 0 : 2;
}

// the order statistics pick.lo and pick.hi of the non-NaN entries of v[0 .. L), as enc_select finds them
void select(const double *v, int32_t L, const fot::EncPick &pick, double *lo, double *hi)
{
    *lo = *hi = NAN;
    for (int32_t i = 0; i < L; ++i) {
        if (v[i] != v[i]) continue;
        const int32_t r = fot::enc_rank([&](int32_t j) { return v[j]; }, i, L);
        if (r == pick.lo) *lo = v[i];
        if (r == pick.hi) *hi = v[i];
    }
}

}  // namespace

int main(int argc, char **argv)
{
    using namespace fot;
    if (argc != 3) { std::fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    EncParams P;
    int32_t hd[4];
    if (!read_all(in, &P, sizeof P) || !read_all(in, hd, sizeof hd)) { std::fprintf(stderr, "truncated header\n"); return 2; }
    const int32_t T = hd[0], A = hd[1], K = hd[2], have_vel = hd[3];
    if (T > (1 << 20) || A > (1 << 16) || K > (1 << 10) || (have_vel & ~1)) { std::fprintf(stderr, "bad header\n"); return 2; }
    const char *why = "";
    if (enc_check_params(P, &why)) return refuse(argv[2], why);
    if (T < 0 || A < 0 || K < 0) return refuse(argv[2], "a negative size");
    const size_t cells = (size_t)T * (size_t)A, rows_kt = (size_t)K * (size_t)T;
    std::vector<double> xy(2 * cells), vel(have_vel ? 2 * cells : 0), ego(2 * rows_kt), psi(rows_kt), speed(rows_kt);
    if (!read_all(in, xy.data(), 8 * xy.size()) || !read_all(in, vel.data(), 8 * vel.size()) || !read_all(in, ego.data(), 8 * ego.size()) ||
        !read_all(in, psi.data(), 8 * psi.size()) || !read_all(in, speed.data(), 8 * speed.size())) {
        std::fprintf(stderr, "truncated arrays\n");
        return 2;
    }
    std::fclose(in);
    const bool cruise_on = P.cruise_mode != ENC_CRUISE_NONE, measure = (P.flags & ENC_MEASURE_REAL) != 0;

    auto pos_at = [&](int64_t f, int a, int c) { return xy[2 * ((size_t)f * (size_t)A + (size_t)a) + (size_t)c]; };
    auto vel_at = [&](int64_t f, int a, int c) {
        if (have_vel) return vel[2 * ((size_t)f * (size_t)A + (size_t)a) + (size_t)c];
        return enc_fallback_vel([&](int32_t t, int cc) { return pos_at(t, a, cc); }, (int32_t)f, T, c, P.dt);
    };

    // the candidate spans (host), then every long enough span's columns and minimum
    std::vector<EncSpan> rec;
    if (T > 0 && A > 0)
        for (int32_t k = 0; k < K; ++k)
            enc_find_spans(T, ego.data() + 2 * (size_t)k * (size_t)T, psi.data() + (size_t)k * (size_t)T, speed.data() + (size_t)k * (size_t)T,
                           [&](int32_t f0, int32_t f1) {
                EncSpan s;
                std::memset(&s, 0, sizeof s);
                s.min_separation = NAN; s.real.closest = NAN; s.real.closest_step = -1; s.row_base = -1;
                s.status = ENC_SHORT; s.vehicle = k; s.frame0 = f0; s.frame1 = f1; s.min_step = -1; s.min_col = -1;
                rec.push_back(s);
            });
    std::vector<std::vector<int32_t>> span_cols(rec.size());
    int64_t n_rows = 0, n_steps = 0;
    for (size_t i = 0; i < rec.size(); ++i) {
        EncSpan &s = rec[i];
        const int32_t f0 = s.frame0, L = s.frame1 - s.frame0;
        if (L < P.min_len) continue;
        const double *eg = ego.data() + 2 * ((size_t)s.vehicle * (size_t)T + (size_t)f0);
        // k_enc_columns: a column's steps in shares, joined; k_enc_compact: 64 lanes take the present columns in turns
        EncMin lane[64];
        for (int l = 0; l < 64; ++l) lane[l] = enc_min_zero();
        for (int a = 0; a < A; ++a) {
            EncCol c; c.m = fid_min_zero(); c.absent = 0;
            for (int w = ENC_STEP_WAVES - 1; w >= 0; --w)          // (any order: the join is exact)
                c = enc_column_join(c, enc_column([&](int32_t t, int cc) { return pos_at((int64_t)f0 + t, a, cc); },
                                                  [&](int32_t t, int cc) { return vel_at((int64_t)f0 + t, a, cc); },
                                                  [&](int32_t t, int cc) { return eg[2 * t + cc]; }, w, ENC_STEP_WAVES, L));
            if (c.absent) continue;
            const int32_t idx = (int32_t)span_cols[i].size();
            span_cols[i].push_back(a);
            lane[a % 64] = enc_min_join(lane[a % 64], enc_min_of_column(c.m, idx));
        }
        for (int off = 32; off >= 1; off >>= 1) {
            EncMin next[64];
            for (int l = 0; l < 64; ++l) next[l] = enc_min_join(lane[l], lane[l ^ off]);
            std::memcpy(lane, next, sizeof next);
        }
        const EncMin &m = lane[0];
        s.n_ped = (int32_t)span_cols[i].size();
        s.min_separation = s.n_ped == 0 ? (double)INFINITY : m.nan ? (double)NAN : m.v;
        if (s.n_ped > 0 && !m.nan) { s.min_step = m.step; s.min_col = m.col; }
        s.status = enc_status(s.n_ped, s.min_separation, P.min_sep_threshold);
        if (s.status != ENC_KEPT) continue;
        s.row_base = n_rows;
        n_rows += s.n_ped;
        n_steps += L;
    }

    std::vector<int32_t> cols((size_t)n_rows, -1), onset_step((size_t)n_rows, -1);
    std::vector<double> cruise((size_t)n_rows, NAN), goals(2 * (size_t)n_rows, NAN), onset_dist((size_t)n_rows, NAN);
    std::vector<double> series(measure ? (size_t)n_steps : 0);
    size_t step_base = 0;
    for (size_t i = 0; i < rec.size(); ++i) {
        EncSpan &s = rec[i];
        if (s.status != ENC_KEPT) continue;
        const int32_t f0 = s.frame0, L = s.frame1 - s.frame0, N = s.n_ped;
        const double *eg = ego.data() + 2 * ((size_t)s.vehicle * (size_t)T + (size_t)f0);
        auto egof = [&](int t, int c) { return eg[2 * t + c]; };
        // k_enc_gather: the packed encounter and, per pedestrian over its steps, the speeds
        std::vector<double> packed(2 * (size_t)L * (size_t)N), sp((size_t)L * (size_t)N), fs((size_t)L * (size_t)N);
        for (int32_t t = 0; t < L; ++t)
            for (int32_t n = 0; n < N; ++n) {
                const int a = span_cols[i][(size_t)n];
                const double px = pos_at((int64_t)f0 + t, a, 0), py = pos_at((int64_t)f0 + t, a, 1);
                packed[2 * ((size_t)t * (size_t)N + (size_t)n)] = px; packed[2 * ((size_t)t * (size_t)N + (size_t)n) + 1] = py;
                const double v = fid_dist(vel_at((int64_t)f0 + t, a, 0), vel_at((int64_t)f0 + t, a, 1));
                const bool is_free = fid_dist(px - eg[2 * t], py - eg[2 * t + 1]) > P.free_distance && v - v == 0.0;
                sp[(size_t)n * (size_t)L + (size_t)t] = v;
                fs[(size_t)n * (size_t)L + (size_t)t] = is_free ? v : (double)NAN;
            }
        // k_enc_rows: one kept pedestrian at a time
        for (int32_t n = 0; n < N; ++n) {
            const size_t g = (size_t)s.row_base + (size_t)n;
            const int a = span_cols[i][(size_t)n];
            cols[g] = a;
            if (!cruise_on) continue;
            const double *v = sp.data() + (size_t)n * (size_t)L, *f = fs.data() + (size_t)n * (size_t)L;
            double lo, hi, value = 0.0;
            bool median = P.cruise_mode == ENC_CRUISE_MEDIAN;
            if (P.cruise_mode == ENC_CRUISE_FREEWALK) {
                int32_t n_free = 0;
                for (int32_t t = 0; t < L; ++t) n_free += f[t] == f[t] ? 1 : 0;
                if (n_free > 0) {
                    const EncPick pick = enc_pick_quantile(n_free, P.cruise_q);
                    select(f, L, pick, &lo, &hi);
                    value = enc_quantile_value(lo, hi, pick.g);
                } else median = true;
            } else if (!median) {
                const EncPick pick = enc_pick_quantile(L, P.cruise_q);
                select(v, L, pick, &lo, &hi);
                value = enc_quantile_value(lo, hi, pick.g);
            }
            if (median) {
                select(v, L, enc_pick_median(L), &lo, &hi);
                value = enc_median_value(L, lo, hi);
            }
            cruise[g] = enc_floor(value);
            const int64_t f1 = (int64_t)f0 + L - 1;
            enc_goal(pos_at(f0, a, 0), pos_at(f0, a, 1), pos_at(f1, a, 0), pos_at(f1, a, 1), vel_at(f0, a, 0), vel_at(f0, a, 1),
                     P.goal_distance, &goals[2 * g], &goals[2 * g + 1]);
        }
        if (!measure) continue;
        // launch_fidelity on the packed encounter: positions only
        FidParams FP;
        FP.accel_threshold = P.accel_threshold; FP.max_distance = P.max_distance; FP.interaction_distance = NAN;
        const size_t stride = 2 * (size_t)N;
        for (int32_t n = 0; n < N; ++n) {
            const double *p = packed.data() + 2 * (size_t)n;
            auto pos = [&](int t, int c) { return p[(size_t)t * stride + (size_t)c]; };
            auto velf = [&](int t, int c) { return fid_gradient([&](int u) { return p[(size_t)u * stride + (size_t)c]; }, t, L, P.dt); };
            double away;
            fid_onset(pos, velf, egof, L, P.dt, FP, &onset_step[(size_t)s.row_base + (size_t)n], &onset_dist[(size_t)s.row_base + (size_t)n], &away);
        }
        FidMin m = fid_min_zero();
        for (int32_t t = 0; t < L; ++t) {
            const double *r = packed.data() + (size_t)t * stride;
            series[step_base + (size_t)t] = fid_separation([&](int j, int c) { return r[2 * j + c]; }, N, eg[2 * t], eg[2 * t + 1]);
            m = fid_min_take(m, series[step_base + (size_t)t], t);
        }
        const size_t b = (size_t)s.row_base;
        s.real = fid_record(m, L, N, false, [&](int) { return 0.0; }, [&](int) { return false; }, [&](int j) { return onset_step[b + (size_t)j]; });
        step_base += (size_t)L;
    }

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    const int32_t oh[2] = { 0, (int32_t)rec.size() };
    const int64_t oq[2] = { n_rows, measure ? n_steps : 0 };
    const bool ok = write_all(o, oh, sizeof oh) && write_all(o, oq, sizeof oq) && write_all(o, rec.data(), sizeof(EncSpan) * rec.size()) &&
                    write_all(o, cols.data(), 4 * cols.size()) && write_all(o, cruise.data(), 8 * cruise.size()) &&
                    write_all(o, goals.data(), 8 * goals.size()) && write_all(o, onset_dist.data(), 8 * onset_dist.size()) &&
                    write_all(o, onset_step.data(), 4 * onset_step.size()) && write_all(o, series.data(), 8 * series.size());
    std::fclose(o);
    if (!ok) { std::perror("write"); return 2; }
    return 0;
}
