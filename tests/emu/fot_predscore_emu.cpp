// fot_predscore_emu.cpp -- csrc/fot_predscore.hpp on the CPU: every origin of a case file evaluated sequentially by
// ps_origin, the records written in fot_pred_score's layout.  Stand-alone (its own main), so that it can also be built
// with -fsanitize=address,undefined and run as it is.
//
//   fot_predscore_emu <cases.bin> <records.bin>
// cases.bin: int32 n, then per origin int32 S, P, T, stride, E, t_major, skip, dtype (0: float32, 1: float64), the tensor
// (S P T 2 elements, [S][P][T][2] or [T][S][P][2]) and the truth (P E 2 float64).  records.bin: n records of 56 bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_predscore.hpp"

namespace {

struct Record {                                   // fot_pred_score (include/fot.h)
    double ade_scene, fde_scene, ade_agent_sum, fde_agent_sum, log_lik_sum;
    int32_t n_peds, n_samples, nll_count, flags;
};
static_assert(sizeof(Record) == 56, "fot_pred_score");

bool read_all(std::FILE *f, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin records.bin\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    int32_t n = 0;
    if (!read_all(in, &n, sizeof n) || n < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<Record> out((size_t)n);
    for (int32_t c = 0; c < n; ++c) {
        int32_t hd[8];
        if (!read_all(in, hd, sizeof hd)) { std::fprintf(stderr, "case %d: truncated header\n", c); return 2; }
        const int S = hd[0], P = hd[1], T = hd[2], stride = hd[3], E = hd[4], tmajor = hd[5], skip = hd[6], dtype = hd[7];
        if (S < 1 || P < 0 || T < 1 || stride < 1 || E < 1 || (skip != 0 && skip != 1) || (dtype != 0 && dtype != 1) ||
            !fot::ps_horizon_fits(stride, E, T, skip)) {
            std::fprintf(stderr, "case %d: bad shape\n", c);
            return 2;
        }
        const size_t n_el = (size_t)S * P * T * 2;
        std::vector<float> t32(dtype == 0 ? n_el : 0);
        std::vector<double> t64(dtype == 1 ? n_el : 0), truth((size_t)P * E * 2);
        if (!read_all(in, dtype == 0 ? (void *)t32.data() : (void *)t64.data(), n_el * (dtype == 0 ? 4 : 8)) ||
            !read_all(in, truth.data(), truth.size() * 8)) {
            std::fprintf(stderr, "case %d: truncated data\n", c);
            return 2;
        }
        auto at = [&](int s, int p, int k, int ax) {
            const int kk = k + skip;
            const size_t i = (tmajor ? ((size_t)kk * S + s) * P + p : ((size_t)s * P + p) * T + kk) * 2 + ax;
            return dtype == 0 ? (double)t32[i] : t64[i];
        };
        const fot::PredScoreTerms t = fot::ps_origin(S, P, stride, E, at, truth.data());
        out[(size_t)c] = Record{ t.ade_scene, t.fde_scene, t.ade_agent_sum, t.fde_agent_sum, t.log_lik_sum,
                                 t.n_peds, t.n_samples, t.nll_count, t.flags };
    }
    std::fclose(in);
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    if (n > 0 && std::fwrite(out.data(), sizeof(Record), (size_t)n, o) != (size_t)n) { std::perror("write"); return 2; }
    std::fclose(o);
    return 0;
}
