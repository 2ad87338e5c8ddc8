// fot_slot_samples_emu.cpp -- test-only program: the ragged layout of a sweep loop whose slots keep sample counts of their
// own (fot_loop_set_slot_samples; csrc/fot_sweep.hpp, shared by the kernels and the host) on the CPU.  Built with g++ by
// tests/test_slot_samples_cpu.py, once plainly and once with -fsanitize=address,undefined, and run as it is; no HIP.
//
// Reads cases from standard input, one per line, and answers each with one line:
//   frame    n_run T select_all  P[n_run]  slot[n_run]  n_slots slot_S[n_slots] mode[n_slots]
//            -> S_max  S[0] .. S[n_run - 1]  blk[0] .. blk[n_run]  size  rep_off[0] select[0] ... rep_off[n_run - 1] select[n_run - 1]
//               (the counts, the packed distribution blocks, then sweep_layout behind them)
//   capacity n_slots T  slot_P[n_slots]  slot_S[n_slots]  -> points
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
        if (what == "frame") {
            int64_t n_run = 0, T = 0, select_all = 0, n_slots = 0;
            in >> n_run >> T >> select_all;
            const std::vector<int32_t> P = read_n<int32_t>(in, n_run), slot = read_n<int32_t>(in, n_run);
            in >> n_slots;
            const std::vector<int32_t> slot_S = read_n<int32_t>(in, n_slots), mode = read_n<int32_t>(in, n_slots);
            if (!in) { std::puts("error"); return 2; }
            std::vector<int32_t> ped0((size_t)n_run + 1, 0);
            for (int64_t i = 0; i < n_run; ++i) ped0[(size_t)i + 1] = ped0[(size_t)i] + P[(size_t)i];
            std::vector<int32_t> ep_S((size_t)n_run);                   // (exactly the frame's episodes: a write past them is caught)
            std::vector<int64_t> blk((size_t)n_run + 1);
            std::vector<SweepEp> tab((size_t)n_run);
            const int32_t most = sweep_slot_counts((int32_t)n_run, slot.data(), slot_S.data(), ep_S.data());
            const int64_t dist_end = sweep_slot_blocks((int32_t)n_run, ped0.data(), ep_S.data(), (int32_t)T, blk.data());
            const int64_t size = sweep_layout((int32_t)n_run, ped0.data(), slot.data(), mode.data(), dist_end, (int32_t)T,
                                              select_all != 0, tab.data());
            std::printf("%d", (int)most);
            for (int32_t s : ep_S) std::printf(" %d", (int)s);
            for (int64_t b : blk) std::printf(" %lld", (long long)b);
            std::printf(" %lld", (long long)size);
            for (size_t i = 0; i < tab.size(); ++i) {
                if (blk[i + 1] - blk[i] != sweep_slot_block_points(ep_S[i], P[i], (int32_t)T)) { std::puts(" error"); return 2; }
                std::printf(" %lld %d", (long long)tab[i].rep_off, (int)tab[i].select);
            }
            std::printf("\n");
        } else if (what == "capacity") {
            int64_t n_slots = 0, T = 0;
            in >> n_slots >> T;
            const std::vector<int32_t> slot_P = read_n<int32_t>(in, n_slots), slot_S = read_n<int32_t>(in, n_slots);
            if (!in) { std::puts("error"); return 2; }
            std::vector<int32_t> slot_ped0((size_t)n_slots + 1, 0);
            for (int64_t e = 0; e < n_slots; ++e) slot_ped0[(size_t)e + 1] = slot_ped0[(size_t)e] + slot_P[(size_t)e];
            std::printf("%lld\n", (long long)sweep_slot_capacity_points((int32_t)n_slots, slot_ped0.data(), slot_S.data(), (int32_t)T));
        } else {
            std::puts("error");
            return 2;
        }
    }
    return 0;
}
