// fot_crowd_emu.cpp -- test-only program: the crowd tables and the consistency check of a sampler loop whose slots share
// their crowds' samples (fot_loop_set_sampler_shared; csrc/fot_sweep.hpp, the code the host runs) on the CPU.  Built with g++
// by tests/test_loop_crowd_sampler_cpu.py, once plainly and once with -fsanitize=address,undefined, and run as it is; no HIP.
//
// Reads cases from standard input, one per line, and answers each with one line:
//   tables     n_run P[n_run] slot[n_run] n_slots crowd[n_slots]
//              -> n_scenes crowd_rows identity  scene_off[n_scenes + 1]  scene_slot[n_scenes]  scene_crowd[n_scenes]
//                 row_scene[crowd_rows]  col[rows]
//   consistent n_slots P[n_slots] frames[n_slots] crowd[n_slots] n_frames_max pos[n_frames_max * sum P * 2] (C99 hex floats)
//              -> code slot_a slot_b                  (slot_a = slot_b = -1 where code is 0)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

template <class V>
void print_all(const V &v) { for (auto x : v) std::printf(" %d", (int)x); }

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "tables") {
            int64_t n_run = 0, n_slots = 0;
            in >> n_run;
            const std::vector<int32_t> P = read_n<int32_t>(in, n_run), slot = read_n<int32_t>(in, n_run);
            in >> n_slots;
            const std::vector<int32_t> crowd = read_n<int32_t>(in, n_slots);
            if (!in) { std::puts("error"); return 2; }
            std::vector<int32_t> ped0((size_t)n_run + 1, 0);
            for (int64_t i = 0; i < n_run; ++i) ped0[(size_t)i + 1] = ped0[(size_t)i] + P[(size_t)i];
            const size_t rows = (size_t)ped0[(size_t)n_run];
            // (exactly the sizes the header names: a write past them is caught)
            std::vector<int32_t> scene_off((size_t)n_run + 1, -7), row_scene(rows, -7), scene_slot((size_t)n_run, -7),
                scene_crowd((size_t)n_run, -7), col(rows, -7);
            const CrowdShape sh = sweep_crowd_tables((int32_t)n_run, ped0.data(), slot.data(), crowd.data(), scene_off.data(),
                                                     row_scene.data(), scene_slot.data(), scene_crowd.data(), col.data());
            if (sh.n_scenes < 0 || sh.n_scenes > n_run || sh.crowd_rows < 0 || (size_t)sh.crowd_rows > rows) { std::puts("error"); return 2; }
            scene_off.resize((size_t)sh.n_scenes + 1); scene_slot.resize((size_t)sh.n_scenes); scene_crowd.resize((size_t)sh.n_scenes);
            row_scene.resize((size_t)sh.crowd_rows);
            std::printf("%d %d %d", (int)sh.n_scenes, (int)sh.crowd_rows, sh.identity ? 1 : 0);
            print_all(scene_off); print_all(scene_slot); print_all(scene_crowd); print_all(row_scene); print_all(col);
            std::printf("\n");
        } else if (what == "consistent") {
            int64_t n_slots = 0, n_frames_max = 0;
            in >> n_slots;
            const std::vector<int32_t> P = read_n<int32_t>(in, n_slots), frames = read_n<int32_t>(in, n_slots),
                                       crowd = read_n<int32_t>(in, n_slots);
            in >> n_frames_max;
            if (!in) { std::puts("error"); return 2; }
            std::vector<int32_t> ped0((size_t)n_slots + 1, 0);
            for (int64_t e = 0; e < n_slots; ++e) ped0[(size_t)e + 1] = ped0[(size_t)e] + P[(size_t)e];
            const int32_t n_cols = ped0[(size_t)n_slots];
            std::vector<double> pos((size_t)n_frames_max * (size_t)n_cols * 2);
            for (double &v : pos) {
                std::string tok;
                if (!(in >> tok)) { std::puts("error"); return 2; }
                v = std::strtod(tok.c_str(), nullptr);
            }
            int32_t a = -1, b = -1;
            const int code = sweep_crowds_consistent((int32_t)n_slots, ped0.data(), frames.data(), crowd.data(), pos.data(), n_cols, &a, &b);
            if (code == 0) a = b = -1;
            std::printf("%d %d %d\n", code, (int)a, (int)b);
        } else {
            std::puts("error");
            return 2;
        }
    }
    return 0;
}
