// fot_model_emu.cpp -- test-only program: the tables of a sampler loop whose slots name their Social-GAN model
// (fot_loop_set_sampler_models; csrc/fot_sweep.hpp's sweep_model_tables and sweep_model_rows, the code the host runs) on the
// CPU.  Built with g++ by tests/test_loop_models_cpu.py, once plainly and once with -fsanitize=address,undefined, and run as
// it is; no HIP.
//
// Reads cases from standard input, one per line, and answers each with one line:
//   models n_run P[n_run] slot[n_run] n_slots crowd[n_slots] model[n_slots] n_models
//          -> for every model: n_scenes rows  scene_off[n_scenes + 1]  scene_slot[n_scenes]  scene_crowd[n_scenes]  row_scene[rows]
//             then row_model[frame rows]  col[frame rows]  and, per frame row, the gather entry: base width col
//             (model m's tensor at element 1000 m) and its source element for sample 2, predictor step 1 of pred_len 3
//   crowds n_run P[n_run] slot[n_run] n_slots crowd[n_slots]          (sweep_crowd_tables, for the one-model comparison)
//          -> n_scenes rows  scene_off  scene_slot  scene_crowd  row_scene  col[frame rows]
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

void print_n(const int32_t *v, int64_t n) { for (int64_t i = 0; i < n; ++i) std::printf(" %d", (int)v[i]); }

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what != "models" && what != "crowds") { std::puts("error"); return 2; }
        int64_t n_run = 0, n_slots = 0, n_models = 1;
        in >> n_run;
        const std::vector<int32_t> P = read_n<int32_t>(in, n_run), slot = read_n<int32_t>(in, n_run);
        in >> n_slots;
        const std::vector<int32_t> crowd = read_n<int32_t>(in, n_slots);
        std::vector<int32_t> model;
        if (what == "models") { model = read_n<int32_t>(in, n_slots); in >> n_models; }
        if (!in || n_models < 1) { std::puts("error"); return 2; }
        std::vector<int32_t> ped0((size_t)n_run + 1, 0);
        for (int64_t i = 0; i < n_run; ++i) ped0[(size_t)i + 1] = ped0[(size_t)i] + P[(size_t)i];
        const size_t rows = (size_t)ped0[(size_t)n_run], nr = (size_t)n_run, nm = (size_t)n_models;
        if (what == "crowds") {
            std::vector<int32_t> scene_off(nr + 1, -7), row_scene(rows, -7), scene_slot(nr, -7), scene_crowd(nr, -7), col(rows, -7);
            const CrowdShape sh = sweep_crowd_tables((int32_t)n_run, ped0.data(), slot.data(), crowd.data(), scene_off.data(),
                                                     row_scene.data(), scene_slot.data(), scene_crowd.data(), col.data());
            std::printf("%d %d", (int)sh.n_scenes, (int)sh.crowd_rows);
            print_n(scene_off.data(), sh.n_scenes + 1); print_n(scene_slot.data(), sh.n_scenes);
            print_n(scene_crowd.data(), sh.n_scenes); print_n(row_scene.data(), sh.crowd_rows); print_n(col.data(), (int64_t)rows);
            std::printf("\n");
            continue;
        }
        // (exactly the sizes the header names, strides n_run and the frame's rows: a write past them is caught)
        std::vector<ModelShape> shape(nm);
        std::vector<int32_t> scene_off(nm * (nr + 1), -7), row_scene(nm * rows, -7), scene_slot(nm * nr, -7), scene_crowd(nm * nr, -7),
            row_model(rows, -7), col(rows, -7);
        sweep_model_tables((int32_t)n_run, ped0.data(), slot.data(), crowd.data(), model.data(), (int32_t)n_models, (int32_t)n_run,
                           (int32_t)rows, shape.data(), scene_off.data(), row_scene.data(), scene_slot.data(), scene_crowd.data(),
                           row_model.data(), col.data());
        bool first = true;
        for (size_t m = 0; m < nm; ++m) {
            const ModelShape &sh = shape[m];
            if (sh.n_scenes < 0 || sh.n_scenes > n_run || sh.rows < 0 || (size_t)sh.rows > rows) { std::puts("error"); return 2; }
            std::printf(first ? "%d %d" : " %d %d", (int)sh.n_scenes, (int)sh.rows);
            first = false;
            print_n(scene_off.data() + m * (nr + 1), sh.n_scenes + 1); print_n(scene_slot.data() + m * nr, sh.n_scenes);
            print_n(scene_crowd.data() + m * nr, sh.n_scenes); print_n(row_scene.data() + m * rows, sh.rows);
        }
        print_n(row_model.data(), (int64_t)rows); print_n(col.data(), (int64_t)rows);
        std::vector<int64_t> base(nm);
        for (size_t m = 0; m < nm; ++m) base[m] = 1000 * (int64_t)m;
        std::vector<ModelRow> tab(rows);
        sweep_model_rows((int32_t)rows, row_model.data(), col.data(), shape.data(), base.data(), tab.data());
        for (const ModelRow &r : tab)
            std::printf(" %lld %d %d %lld", (long long)r.base, (int)r.width, (int)r.col, (long long)sweep_model_src_elem(r, 3, 2, 1));
        std::printf("\n");
    }
    return 0;
}
