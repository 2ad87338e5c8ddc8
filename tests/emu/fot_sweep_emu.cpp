// fot_sweep_emu.cpp -- test-only program: the layout arithmetic of a sweep loop (csrc/fot_sweep.hpp, shared by the sweep
// forms of the selection and block kernels and the host) on the CPU.  Built with g++ by tests/test_loop_sweep_cpu.py, once
// plainly and once with -fsanitize=address,undefined, and run as it is; no HIP.
//
// Reads cases from standard input, one per line, and answers each with one line:
//   layout  n_run dist_end T select_all  P[n_run]  slot[n_run]  n_slots mode[n_slots]
//           -> size  rep_off[0] select[0] ... rep_off[n_run - 1] select[n_run - 1]
//   columns n_run P[n_run] slot[n_run] n_slots slot_P[n_slots] col0[n_slots] n_rec_cols
//           -> fit  col[0] ... col[rows - 1]        (fit: sweep_columns_fit over ALL slots; the columns are formed only if it holds)
//   capacity S n_cols T -> points
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_sweep.hpp"

using namespace fot;

namespace {

template <class T>
std::vector<T> read_n(std::istream &in, int64_t n)
{
    std::vector<T> v((size_t)n);
    for (auto &x : v) { int64_t t = 0; in >> t; x = (T)t; }
    return v;
}

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "layout") {
            int64_t n_run = 0, dist_end = 0, T = 0, select_all = 0, n_slots = 0;
            in >> n_run >> dist_end >> T >> select_all;
            const std::vector<int32_t> P = read_n<int32_t>(in, n_run), slot = read_n<int32_t>(in, n_run);
            in >> n_slots;
            const std::vector<int32_t> mode = read_n<int32_t>(in, n_slots);
            if (!in) { std::puts("error"); return 2; }
            std::vector<int32_t> ped0((size_t)n_run + 1, 0);
            for (int64_t i = 0; i < n_run; ++i) ped0[(size_t)i + 1] = ped0[(size_t)i] + P[(size_t)i];
            std::vector<SweepEp> tab((size_t)n_run);
            const int64_t size = sweep_layout((int32_t)n_run, ped0.data(), slot.data(), mode.data(), dist_end, (int32_t)T,
                                              select_all != 0, tab.data());
            std::printf("%lld", (long long)size);
            for (const SweepEp &e : tab) {
                if (sweep_plans_on_block(e) != (e.rep_off >= 0) || e._pad != 0) { std::puts(" error"); return 2; }
                std::printf(" %lld %d", (long long)e.rep_off, (int)e.select);
            }
            std::printf("\n");
        } else if (what == "columns") {
            int64_t n_run = 0, n_slots = 0, n_rec_cols = 0;
            in >> n_run;
            const std::vector<int32_t> P = read_n<int32_t>(in, n_run), slot = read_n<int32_t>(in, n_run);
            in >> n_slots;
            const std::vector<int32_t> slot_P = read_n<int32_t>(in, n_slots), col0 = read_n<int32_t>(in, n_slots);
            in >> n_rec_cols;
            if (!in) { std::puts("error"); return 2; }
            std::vector<int32_t> ped0((size_t)n_run + 1, 0), slot_ped0((size_t)n_slots + 1, 0);
            for (int64_t i = 0; i < n_run; ++i) ped0[(size_t)i + 1] = ped0[(size_t)i] + P[(size_t)i];
            for (int64_t e = 0; e < n_slots; ++e) slot_ped0[(size_t)e + 1] = slot_ped0[(size_t)e] + slot_P[(size_t)e];
            const bool fit = sweep_columns_fit((int32_t)n_slots, slot_ped0.data(), col0.data(), (int32_t)n_rec_cols);
            std::printf("%d", fit ? 1 : 0);
            if (fit) {
                std::vector<int32_t> col((size_t)ped0[(size_t)n_run]);      // (exactly the frame's rows: a write past them is caught)
                sweep_fill_columns((int32_t)n_run, ped0.data(), slot.data(), col0.data(), col.data());
                for (int32_t c : col) std::printf(" %d", (int)c);
            }
            std::printf("\n");
        } else if (what == "capacity") {
            int64_t S = 0, n_cols = 0, T = 0;
            in >> S >> n_cols >> T;
            std::printf("%lld\n", (long long)sweep_capacity_points((int32_t)S, n_cols, (int32_t)T));
        } else {
            std::puts("error");
            return 2;
        }
    }
    return 0;
}
