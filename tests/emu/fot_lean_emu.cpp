// fot_lean_emu.cpp -- TEST-ONLY: the lean form of the evaluation walk against the general form, on the host.
//
// The walk k_evaluate* run is host/device-shared code (csrc/fot_math.hpp: evaluate_segment, EntryColliderT); its lean
// form -- the one the library launches for plan calls without a chance budget, the single centre circle and at most 64
// samples per candidate -- is `evaluate_segment<true>` over `EntryColliderT<true>`.  This program runs the whole host
// emulation of the pipeline (fot_emu.cpp, included below as it is) and, for every candidate the emulation evaluates
// with an EntryCollider of an eligible instance, evaluates it a second time in the lean form and compares everything a
// candidate carries out of the walk bit for bit: the check flags, the first NaN index, the last kept sample, v_last,
// d_last, the largest step, and after finish_candidate status, keep, cost and travel; and whether it was hit.
//
// A program of its own (main below), so that it can be built with -fsanitize=address,undefined and run as it is:
//     fot_lean_emu <cases.bin>        one line per case, exit status 1 on any difference
// cases.bin is written by tests/test_lean_walk_cpu.py from the golden vectors (a sequence of length-prefixed blobs).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_math.hpp"
#include "../../integrated_path_planning_amd/csrc/fot_setup.hpp"

namespace lean_check {
struct Tally {
    long general = 0;        // candidates evaluated with an EntryCollider
    long compared = 0;       // ... of an eligible instance: walked again in the lean form
    long differences = 0;
    long hit = 0, seen_nan = 0, singular = 0, failed = 0;     // what the compared candidates exercised (general form)
    char first[160] = "";
};
Tally tally;

inline bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

template <class Tab, class Sink>
void evaluate_candidate(const fot::DevParams &P, const fot::InstDesc &D, const fot::LoopConst &C, const fot::LonInfo &L,
                        const Tab &lon_tab, const double *q, int n_loop, Sink &sink, fot::CandResult &out)
{
    using namespace fot;
    if constexpr (!std::is_same<Sink, EntryCollider>::value) {
        fot::evaluate_candidate(P, D, C, L, lon_tab, q, n_loop, sink, out);
    } else {
        SegState g;
        seg_init(g);
        evaluate_segment(P, C, L, lon_tab, q, 0, n_loop, sink, g);
        finish_candidate(P, D, L, lon_tab, q, g, sink.collided(), out);
        ++tally.general;
        // the library's rule (enqueue_lane): at most 64 samples, the single centre circle, no chance budget
        if (P.n_total > WAVE || C.n_circ_fp != 0 || D.max_viol != 0) return;
        EntryColliderT<true> ls;
        ls.init(P, D);
        ls.rng = sink.rng; ls.thr_k = sink.thr_k; ls.thr_sure_k = sink.thr_sure_k;
        ls.e32 = sink.e32; ls.e64 = sink.e64; ls.sid = sink.sid;
        SegState gl;
        seg_init(gl);
        evaluate_segment<true>(P, C, L, lon_tab, q, 0, n_loop, ls, gl);
        CandResult rl;
        finish_candidate(P, D, L, lon_tab, q, gl, ls.collided(), rl);
        ++tally.compared;
        tally.hit += sink.hit; tally.seen_nan += (g.acc.fl & CK_SEEN_NAN) != 0;
        tally.singular += (g.acc.fl & CK_SINGULAR) != 0; tally.failed += (g.acc.fl & CK_FAILED) != 0;
        const char *what = nullptr;
        if (g.acc.fl != gl.acc.fl) what = "flags";
        else if (g.first_nan != gl.first_nan) what = "first NaN";
        else if (g.k_last != gl.k_last) what = "last kept sample";
        else if (!same(g.v_last, gl.v_last) || !same(out.v_last, rl.v_last)) what = "v_last";
        else if (!same(g.d_last, gl.d_last)) what = "d_last";
        else if (!same(g.acc.max_step2, gl.acc.max_step2)) what = "largest step";
        else if (sink.hit != ls.hit) what = "hit";
        else if (out.status != rl.status) what = "status";
        else if (out.keep != rl.keep) what = "kept length";
        else if (!same(out.cost, rl.cost)) what = "cost";
        else if (!same(out.travel, rl.travel)) what = "travel";
        if (what) {
            if (!tally.differences)
                std::snprintf(tally.first, sizeof(tally.first), "candidate %ld of the case: %s differs", tally.compared - 1, what);
            ++tally.differences;
        }
    }
}
}  // namespace lean_check

#define evaluate_candidate lean_check::evaluate_candidate
#include "fot_emu.cpp"
#undef evaluate_candidate

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
    if (argc < 2) { std::fprintf(stderr, "usage: %s <cases.bin>\n", argv[0]); return 2; }
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
        lean_check::tally = lean_check::Tally();
        std::vector<fot_result> out(1);
        char err[256] = "";
        const int rc = emu_plan_batch(&params, n_knots, (const double *)b[1].b.data(), (const double *)b[2].b.data(), &bt,
                                      out.data(), 0, nullptr, nullptr, nullptr, err);
        const lean_check::Tally &t = lean_check::tally;
        std::printf("%s rc %d general %ld compared %ld differences %ld hit %ld seen_nan %ld singular %ld failed %ld %s\n",
                    name.b.data(), rc, t.general, t.compared, t.differences, t.hit, t.seen_nan, t.singular, t.failed, t.first);
        if (rc != 0 || t.differences) bad = 1;
        ++n_cases;
    }
    std::fclose(f);
    if (!n_cases) { std::fprintf(stderr, "no case in %s\n", argv[1]); return 2; }
    return bad;
}
