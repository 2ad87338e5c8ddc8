// fot_stepform_emu.cpp -- TEST-ONLY: the evaluation walk's time step in its earlier form against the one the library runs.
//
// The walk (csrc/fot_math.hpp evaluate_segment / check_sample_geo) keeps the four plain limits (speed, acceleration, lateral
// acceleration, road) as running maxima that check_fold() turns into flags behind the walk, and carries the heading
// RELATIVE to the reference frame, composing the two headings of the low-speed rule's yaw step in that branch from the
// rows k and k - 1 (FrameHeadings).  The form before that set the four flags by a compare in every step and carried the
// heading itself.  `old_form` below restates that earlier walk; this program runs the host emulation of the pipeline
// (fot_emu.cpp, included as it is) and walks every candidate the emulation evaluates against the entry lists in both
// forms -- in one piece and cut into 2 and 3 time segments, segment by segment -- and compares, bit for bit: the flag word,
// the largest step, the first NaN index, the last kept sample, v_last, d_last, the hit and the sample mask; and in every
// low-speed step the sin / cos of the yaw step that the earlier form makes from its carried headings against the ones
// FrameHeadings composes.  The tallies say what the candidates exercised.
//
// A program of its own (main below), so that it can be built with -fsanitize=address,undefined and run as it is:
//     fot_stepform_emu <cases.bin>        one line per case, exit status 1 on any difference
//     fot_stepform_emu --limits           directed paths over check_sample alone (limits_unit below)
// cases.bin: a sequence of length-prefixed blobs, the layout of tests/emu/fot_lean_emu.cpp.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_math.hpp"
#include "../../integrated_path_planning_amd/csrc/fot_setup.hpp"

namespace form_check {
using namespace fot;

struct Tally {
    long walked = 0, segments = 0, differences = 0;
    long low_speed = 0;          // low-speed steps compared (sin / cos of the yaw step)
    long low_hold_prev = 0;      // ... whose previous sample is a held one (row k - 1 is the brake ladder's hold row)
    long low_cut_prev = 0;       // ... that are the first step of a segment with k0 > 0 (the predecessor is rebuilt)
    long yaw_far = 0;            // ... that go on to the arc tangent
    long limit_flag = 0;         // candidates that end with one of the four limit flags
    long limit_hit = 0;          // ... whose walk in one piece also recorded a hit
    long seen_nan = 0;
    char first[160] = "";
};
Tally tally;

inline bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

inline void differs(const char *what, int n_seg, int sg, int k)
{
    if (!tally.differences)
        std::snprintf(tally.first, sizeof(tally.first), "candidate %ld, %d segment(s), segment %d, k %d: %s differs",
                      tally.walked, n_seg, sg, k, what);
    ++tally.differences;
}

namespace old_form {
// the earlier check_sample: flags by a compare per step; p and c.prev carry the heading.  rel / prev_rel: the same two
// samples with the relative heading, as the library's walk carries them -- only for the comparison in the low-speed branch.
template <class Tab>
void check_sample(const LoopConst &C, CheckAcc &c, int k, const PathSample &p, const PathSample &rel, const PathSample &prev_rel,
                  const Tab &tab, const LonSample &ls, int n_eval, bool cut, int n_seg, int sg)
{
    check_flag(c, !(isfinite(p.v) && isfinite(p.a) && isfinite(p.kappa)), CK_NONFINITE);
    if (k > 0) {
        const double sx = p.x - c.prev.x, sy = p.y - c.prev.y;
        const double step2 = sum_sq_unfused(sx, sy);
        check_flag(c, isnan(step2), CK_NANSTEP);
        if (step2 > c.max_step2) c.max_step2 = step2;
        check_flag(c, p.v > C.lim_speed, CK_SPEED);
        check_flag(c, fabs(p.a) > C.lim_accel, CK_ACCEL);
        if (p.v > 0.5) {
            check_flag(c, fabs(p.kappa) > C.lim_curv, CK_CURV);
        } else {
            const double dd = fabs(p.d - c.prev.d);
            const double d_s = fabs(tab.s_at(k) - tab.s_at(k - 1));
            check_flag(c, dd > fmax(1.5 * d_s, 0.02), CK_CURV);
            const double sn = p.sin_t * c.prev.cos_t - p.cos_t * c.prev.sin_t;
            const double cs = p.cos_t * c.prev.cos_t + p.sin_t * c.prev.sin_t;
            const bool far = !(cs > 0.0 && fabs(sn) <= 0.09 * cs);
            if (far) check_flag(c, yaw_step_over_cap(sn, cs, C.lim_curv, step2), CK_CURV);
            // what the library's walk hands to the same test
            double ct, st, pct, pst, sn2, cs2;
            FrameHeadings<Tab, false>{ tab, k, ls.cos_r, ls.sin_r }.headings(rel, prev_rel, ct, st, pct, pst);
            yaw_step_sin_cos(ct, st, pct, pst, sn2, cs2);
            ++tally.low_speed;
            tally.low_hold_prev += k - 1 >= n_eval;
            tally.low_cut_prev += cut;
            tally.yaw_far += far;
            if (!same(ct, p.cos_t) || !same(st, p.sin_t)) differs("heading of the sample", n_seg, sg, k);
            if (!same(pct, c.prev.cos_t) || !same(pst, c.prev.sin_t)) differs("heading of the previous sample", n_seg, sg, k);
            if (!same(sn, sn2) || !same(cs, cs2)) differs("sin / cos of the yaw step", n_seg, sg, k);
        }
        check_flag(c, p.v * p.v * fabs(p.kappa) > C.lim_lat, CK_LAT);
        check_flag(c, fabs(p.d) > C.road_lim, CK_ROAD);
    }
    c.prev = p;
}

inline void to_samples(const CartSample &c, double d, PathSample &ps, PathSample &rel)
{
    ps.x = c.x; ps.y = c.y; ps.cos_t = c.cos_t; ps.sin_t = c.sin_t; ps.kappa = c.kappa; ps.v = c.v; ps.a = c.a; ps.d = d;
    rel = ps;
    rel.cos_t = c.cos_d; rel.sin_t = c.sin_d;
}

// the earlier evaluate_segment (the form without scalar registers), over the general sink
template <class Tab>
void evaluate_segment(const DevParams &P, const LoopConst &C, const LonInfo &L, const Tab &lon_tab, const double *q, int k0,
                      int k1, EntryCollider &sink, SegState &g, int n_seg, int sg)
{
    const int n_t = L.n_t;
    CheckAcc &acc = g.acc;
    PathSample prev_rel = acc.prev;
    if (k0 > 0 && k0 - 1 < n_t) {
        LonSample ls;
        lon_tab.load(k0 - 1, ls);
        double d, d_d, d_dd, d_ddd;
        lat_sample(q, k0 - 1, L.n_eval, C.dt, d, d_d, d_dd, d_ddd);
        CartSample c;
        frenet_to_cart(ls, d, d_d, d_dd, c);
        to_samples(c, d, acc.prev, prev_rel);
    }
    for (int k = k0; k < k1; ++k) {
        LonSample ls;
        lon_tab.load(k, ls);
        if (!(k < n_t)) continue;
        double d, d_d, d_dd, d_ddd;
        lat_sample(q, k, L.n_eval, C.dt, d, d_d, d_dd, d_ddd);
        g.d_last = d;
        CartSample c;
        frenet_to_cart(ls, d, d_d, d_dd, c);
        check_flag(acc, isfinite(c.omkd) && c.omkd <= 0.05, CK_SINGULAR);
        if (!(acc.fl & CK_SEEN_NAN) && isnan(c.x)) { acc.fl |= CK_SEEN_NAN; g.first_nan = k; }
        if (!(acc.fl & CK_SEEN_NAN)) {
            PathSample ps, rel;
            to_samples(c, d, ps, rel);
            check_sample(C, acc, k, ps, rel, prev_rel, lon_tab, ls, L.n_eval, k == k0 && k0 > 0, n_seg, sg);
            prev_rel = rel;
            const bool alive = (acc.fl & CK_FAILED) == 0;
            if (C.n_circ_fp > 0) {
                for (int ci = 0; ci < C.n_circ_fp; ++ci)
                    sink.put(k, ci, c.x + P.circ_off[ci] * c.cos_t, c.y + P.circ_off[ci] * c.sin_t, alive);
            } else {
                sink.put(k, 0, c.x, c.y, alive);
            }
            g.v_last = c.v; g.k_last = k;
        }
    }
}
}  // namespace old_form

inline const char *differ(const SegState &a, const SegState &b, const EntryCollider &sa, const EntryCollider &sb)
{
    if (a.acc.fl != b.acc.fl) return "flags";
    if (a.first_nan != b.first_nan) return "first NaN";
    if (a.k_last != b.k_last) return "last kept sample";
    if (!same(a.v_last, b.v_last)) return "v_last";
    if (!same(a.d_last, b.d_last)) return "d_last";
    if (!same(a.acc.max_step2, b.acc.max_step2)) return "largest step";
    if (sa.hit != sb.hit) return "hit";
    if (sa.hit_mask != sb.hit_mask || sa.viol != sb.viol) return "sample mask";
    return nullptr;
}

template <class Tab, class Sink>
void evaluate_candidate(const DevParams &P, const InstDesc &D, const LoopConst &C, const LonInfo &L, const Tab &lon_tab,
                        const double *q, int n_loop, Sink &sink, CandResult &out)
{
    if constexpr (!std::is_same<Sink, EntryCollider>::value) {
        fot::evaluate_candidate(P, D, C, L, lon_tab, q, n_loop, sink, out);
    } else {
        const Sink fresh = sink;                                 // (initialised by the caller, nothing handed over yet)
        fot::evaluate_candidate(P, D, C, L, lon_tab, q, n_loop, sink, out);
        for (int n_seg = 1; n_seg <= 3; ++n_seg) {
            const int seg_len = (n_loop + n_seg - 1) / n_seg;
            for (int sg = 0; sg < n_seg; ++sg) {
                if (sg > 0 && sg * seg_len >= L.n_t) break;
                const int k0 = sg * seg_len, k1 = n_loop < k0 + seg_len ? n_loop : k0 + seg_len;
                Sink s_new = fresh, s_old = fresh;
                SegState g_new, g_old;
                seg_init(g_new); seg_init(g_old);
                fot::evaluate_segment<false, false>(P, C, L, lon_tab, q, k0, k1, s_new, g_new);
                old_form::evaluate_segment(P, C, L, lon_tab, q, k0, k1, s_old, g_old, n_seg, sg);
                ++tally.segments;
                if (const char *what = differ(g_old, g_new, s_old, s_new)) differs(what, n_seg, sg, -1);
                // the form that spends scalar registers carries the same maxima
                Sink s_sreg = fresh;
                SegState g_sreg;
                seg_init(g_sreg);
                fot::evaluate_segment<false, true>(P, C, L, lon_tab, q, k0, k1, s_sreg, g_sreg, L.n_eval);
                if (const char *what = differ(g_old, g_sreg, s_old, s_sreg)) differs(what, n_seg, sg, -2);
                if (n_seg == 1) {
                    const uint32_t lim = CK_SPEED | CK_ACCEL | CK_LAT | CK_ROAD;
                    tally.limit_flag += (g_old.acc.fl & lim) != 0;
                    tally.limit_hit += (g_old.acc.fl & lim) != 0 && s_old.hit;
                    tally.seen_nan += (g_old.acc.fl & CK_SEEN_NAN) != 0;
                }
            }
        }
        ++tally.walked;
    }
}
}  // namespace form_check

#define evaluate_candidate form_check::evaluate_candidate
#include "fot_emu.cpp"
#undef evaluate_candidate

// `--limits`: paths of six fast samples of which exactly ONE exceeds one of the four limits -- the first checked sample
// (k = 1), the last one, or sample 0, which must not count -- by a finite amount, as +inf, and as a NaN (no limit flag:
// the compare is false, the maximum keeps its other operand).  Both forms of check_sample over each; the flag words are
// equal and hold the limit's flag exactly where expected.  One line per path, exit status 1 on any miss.
static int limits_unit()
{
    using namespace fot;
    static double zeros[10 * FOT_MAX_NT];
    const GlobalTab tab{ zeros };
    LoopConst C;
    C.dt = 0.1; C.lim_speed = 10.0; C.lim_accel = 4.0; C.lim_curv = 1e300; C.lim_lat = 50.0; C.road_lim = 3.0; C.n_circ_fp = 0;
    const char *names[4] = { "speed", "accel", "lat_accel", "road" };
    const uint32_t bits[4] = { CK_SPEED, CK_ACCEL, CK_LAT, CK_ROAD };
    const char *where_names[3] = { "k1", "last", "k0" };
    const int n = 6, where_k[3] = { 1, n - 1, 0 };
    const double big[3] = { 1.0, INFINITY, NAN };              // finite excess, +inf, NaN
    int bad = 0;
    for (int rule = 0; rule < 4; ++rule) for (int w = 0; w < 3; ++w) for (int kind = 0; kind < 3; ++kind)
        for (int sign = 0; sign < 2; ++sign) {
            if (sign && (rule == 0 || rule == 2)) continue;    // (v and v^2 |kappa| have no negative side; a and d do)
            CheckAcc a_old, a_new;
            check_init(a_old); check_init(a_new);
            PathSample prev_rel = a_old.prev;
            for (int k = 0; k < n; ++k) {
                PathSample p;
                p.x = 0.3 * k; p.y = 0.0; p.cos_t = 1.0; p.sin_t = 0.0; p.kappa = 0.01; p.v = 5.0; p.a = 1.0; p.d = 0.5;
                if (k == where_k[w]) {
                    const double f = kind == 0 ? 1.25 : big[kind], sg = sign ? -1.0 : 1.0;
                    if (rule == 0) p.v = kind == 0 ? C.lim_speed * f : f;
                    if (rule == 1) p.a = sg * (kind == 0 ? C.lim_accel * f : f);
                    if (rule == 2) p.kappa = kind == 0 ? C.lim_lat * f / (p.v * p.v) : f;
                    if (rule == 3) p.d = sg * (kind == 0 ? C.road_lim * f : f);
                }
                LonSample ls;
                tab.load(k, ls);
                form_check::old_form::check_sample(C, a_old, k, p, p, prev_rel, tab, ls, n, false, 1, 0);
                prev_rel = p;
                check_sample(C, a_new, k, p, true, true, [] { return 1.0; });
            }
            check_fold(C, a_new);
            const uint32_t lim = CK_SPEED | CK_ACCEL | CK_LAT | CK_ROAD;
            uint32_t want = (w != 2 && kind != 2) ? bits[rule] : 0u;
            if (want && rule == 0 && kind == 1) want |= CK_LAT;     // (v = +inf: v^2 |kappa| is +inf too)
            const bool ok = a_old.fl == a_new.fl && (a_new.fl & lim) == want && form_check::same(a_old.max_step2, a_new.max_step2);
            std::printf("limits %s %s %s%s old %#x new %#x want %#x %s\n", names[rule], where_names[w],
                        kind == 0 ? "finite" : kind == 1 ? "inf" : "nan", sign ? " negative" : "", a_old.fl, a_new.fl, want,
                        ok ? "ok" : "MISS");
            bad |= !ok;
        }
    return bad;
}

namespace {
struct Blob { std::vector<char> b; };
bool read_blob(FILE *f, Blob &o)
{
    int64_t n = 0;
    if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > (int64_t)1 << 31) return false;
    o.b.assign((size_t)n + 8, 0);                              // (+8: an empty blob still has an address)
    return n == 0 || std::fread(o.b.data(), 1, (size_t)n, f) == (size_t)n;
}
}  // namespace

// per case: name | fot_params | wx | wy | fot_ego | target_speed | fot_overrides | max_stop | static_off[2] | static_xy |
// dyn_off[1] | dyn_dims[4] | dyn_xy     (one instance, float64 obstacles)
int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <cases.bin> | --limits\n", argv[0]); return 2; }
    if (!std::strcmp(argv[1], "--limits")) return limits_unit();
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int bad = 0, n_cases = 0;
    for (;;) {
        Blob name;
        if (!read_blob(f, name)) break;
        Blob b[12];
        for (Blob &x : b) if (!read_blob(f, x)) { std::fprintf(stderr, "%s: truncated case\n", name.b.data()); return 2; }
        if (b[0].b.size() != sizeof(fot_params) + 8 || b[3].b.size() != sizeof(fot_ego) + 8 ||
            b[5].b.size() != sizeof(fot_overrides) + 8) {
            std::fprintf(stderr, "%s: structure sizes differ from include/fot.h\n", name.b.data());
            return 2;
        }
        fot_params params;
        std::memcpy(&params, b[0].b.data(), sizeof(params));
        const int n_knots = (int)((b[1].b.size() - 8) / sizeof(double));
        fot_batch bt;
        std::memset(&bt, 0, sizeof(bt));
        bt.n_inst = 1; bt.obstacle_dtype = FOT_F64;
        bt.ego = (const fot_ego *)b[3].b.data();
        bt.target_speed = (const double *)b[4].b.data();
        bt.overrides = (const fot_overrides *)b[5].b.data();
        bt.max_stop_distance = (const double *)b[6].b.data();
        if (b[8].b.size() > 8) { bt.static_xy = b[8].b.data(); bt.static_off = (const int32_t *)b[7].b.data(); }
        if (b[11].b.size() > 8) {
            bt.dyn_xy = b[11].b.data(); bt.dyn_off = (const int64_t *)b[9].b.data(); bt.dyn_dims = (const int32_t *)b[10].b.data();
        }
        form_check::tally = form_check::Tally();
        std::vector<fot_result> out(1);
        char err[256] = "";
        const int rc = emu_plan_batch(&params, n_knots, (const double *)b[1].b.data(), (const double *)b[2].b.data(), &bt,
                                      out.data(), 0, nullptr, nullptr, nullptr, err);
        const form_check::Tally &t = form_check::tally;
        std::printf("%s rc %d walked %ld segments %ld differences %ld low_speed %ld low_hold_prev %ld low_cut_prev %ld yaw_far %ld "
                    "limit_flag %ld limit_hit %ld seen_nan %ld %s\n", name.b.data(), rc, t.walked, t.segments, t.differences,
                    t.low_speed, t.low_hold_prev, t.low_cut_prev, t.yaw_far, t.limit_flag, t.limit_hit, t.seen_nan, t.first);
        if (rc != 0 || t.differences) bad = 1;
        ++n_cases;
    }
    std::fclose(f);
    if (!n_cases) { std::fprintf(stderr, "no case in %s\n", argv[1]); return 2; }
    return bad;
}
