// fot_select_emu.cpp -- TEST-ONLY: the candidate selection's merge (csrc/fot_math.hpp select_entry / scan_merge) applied
// on the CPU in the shapes the kernels apply it in, and the tile tables of the shared host builder (csrc/fot_setup.hpp).
//
//   emu_tile_tables       cand0[] / n[] of build_tile_shapes_wave / build_tile_shapes_grouped for a lattice and an n_tv:
//                         which tile, lane and group a candidate index sits in under either cut
//   emu_select_entries    select_entry on arrays: what each candidate enters the selection with
//   emu_merge_butterfly   wave_argmin (csrc/fot_kernels.hip): the xor butterfly, offsets 32 .. 1 over 64 slots, every slot
//                         merging its partner's value of the step before as the shuffle hands it over
//   emu_merge_strided     select_instance_wave: slot l folds the parts l, l + 64, ... in ascending order, then the
//                         butterfly; the winning part's `keep` carried as the kernel carries it (a transcription: the
//                         carry itself lives in the kernel, only the merge is shared code)
//   emu_merge_serial      a serial fold of the parts in a given order (the order tiles might arrive in)
//
// Built by tests/test_selection_ties_cpu.py as a shared object (ctypes) and, with -DFOT_SELECT_EMU_MAIN, as a program
// of its own that checks the three shapes against a strict `<` loop on seeded sets -- the form the sanitizer build runs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_math.hpp"
#include "../../integrated_path_planning_amd/csrc/fot_setup.hpp"

using namespace fot;

namespace {
void butterfly(ScanBest *b)                        // b[WAVE]: every slot ends with the wave's result
{
    for (int off = 32; off >= 1; off >>= 1) {
        ScanBest o[WAVE];
        for (int l = 0; l < WAVE; ++l) o[l] = b[l ^ off];
        for (int l = 0; l < WAVE; ++l) scan_merge(b[l], o[l]);
    }
}
}  // namespace

extern "C" int emu_tile_tables(const fot_params *params, int n_tv, int grouped, int cap, int32_t *cand0, int32_t *n)
{
    std::string err;
    DevParams P;
    if (build_dev_params(*params, P, err) != FOT_OK || n_tv < 1 || n_tv > FOT_MAX_TV) return -1;
    TileShapes T;
    if (grouped) build_tile_shapes_grouped(P, T); else build_tile_shapes_wave(P, T);
    const int nt = T.tiles_of(n_tv);
    if (nt > cap) return -2;
    for (int t = 0; t < nt; ++t) {
        cand0[t] = T.cand0[(size_t)T.off[n_tv] + t];
        n[t] = T.n[(size_t)T.off[n_tv] + t];
    }
    return nt;
}

extern "C" int emu_group_tiles(void) { return GROUP_TILES; }

extern "C" void emu_select_entries(int n, const int32_t *status, const double *cost, const int32_t *index,
                                   double *e_cost, int32_t *e_idx)
{
    for (int i = 0; i < n; ++i) {
        const ScanBest e = select_entry(status[i], cost[i], index[i]);
        e_cost[i] = e.dist; e_idx[i] = e.idx;
    }
}

// cost / idx [WAVE] -> out_cost / out_idx [WAVE]: the result every slot holds; returns 0 if all slots agree, else 1
extern "C" int emu_merge_butterfly(const double *cost, const int32_t *idx, double *out_cost, int32_t *out_idx)
{
    ScanBest b[WAVE];
    for (int l = 0; l < WAVE; ++l) { b[l].dist = cost[l]; b[l].idx = idx[l]; }
    butterfly(b);
    int differ = 0;
    for (int l = 0; l < WAVE; ++l) {
        out_cost[l] = b[l].dist; out_idx[l] = b[l].idx;
        differ |= b[l].idx != b[0].idx;
    }
    return differ;
}

// n parts (cost, idx, keep) -> the selected (cost, idx, keep); returns 0, or 1 if the slots disagree
extern "C" int emu_merge_strided(int n, const double *cost, const int32_t *idx, const int32_t *keep,
                                 double *out_cost, int32_t *out_idx, int32_t *out_keep)
{
    ScanBest b[WAVE];
    int keep_l[WAVE], mine[WAVE];
    for (int l = 0; l < WAVE; ++l) {
        b[l].dist = INFINITY; b[l].idx = -1; keep_l[l] = 0;
        for (int t = l; t < n; t += WAVE) {
            const ScanBest o = { cost[t], idx[t] };
            const int before = b[l].idx;
            scan_merge(b[l], o);
            if (b[l].idx != before) keep_l[l] = keep[t];
        }
        mine[l] = b[l].idx;
    }
    butterfly(b);
    int differ = 0, who = -1;
    for (int l = 0; l < WAVE; ++l) {
        differ |= b[l].idx != b[0].idx;
        if (who < 0 && mine[l] == b[0].idx && b[0].idx >= 0) who = l;      // (the first set bit of the ballot)
    }
    *out_cost = b[0].dist; *out_idx = b[0].idx; *out_keep = who >= 0 ? keep_l[who] : 0;
    return differ;
}

// the parts folded one after the other in the order perm[0], perm[1], ...
extern "C" void emu_merge_serial(int n, const double *cost, const int32_t *idx, const int32_t *perm,
                                 double *out_cost, int32_t *out_idx)
{
    ScanBest b = { INFINITY, -1 };
    for (int i = 0; i < n; ++i) {
        const ScanBest o = { cost[perm[i]], idx[perm[i]] };
        scan_merge(b, o);
    }
    *out_cost = b.dist; *out_idx = b.idx;
}

#ifdef FOT_SELECT_EMU_MAIN
// Seeded sets of candidates (status, cost from a handful of values so that ties dominate, +inf and NaN among them),
// cut into parts of up to 64 as tiles are; every shape must select what the strict `<` loop over the indices selects.
// Prints "sets N differences D"; exit status 1 on a difference.
namespace {
uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t m)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33) % m;
}
}  // namespace

int main(int argc, char **argv)
{
    const int n_sets = argc > 1 ? std::atoi(argv[1]) : 200;
    int differences = 0;
    for (int set = 0; set < n_sets; ++set) {
        const int n_parts = 1 + (int)rnd(320);
        const double values[7] = { 0.0, 1.5, 1.5000000000000002, -2.0, 7.25, INFINITY, NAN };
        const int n_values = 3 + (int)rnd(3), with_nonfinite = set % 3 == 0;
        std::vector<double> p_cost((size_t)n_parts, INFINITY);
        std::vector<int32_t> p_idx((size_t)n_parts, -1), p_keep((size_t)n_parts, 0), perm((size_t)n_parts);
        double want_cost = INFINITY;
        int want_idx = -1, want_keep = 0, index = 0;
        for (int t = 0; t < n_parts; ++t) {
            const int n = (int)rnd(WAVE + 1);                  // candidates of the part (0: an empty tile)
            std::vector<double> c((size_t)WAVE, INFINITY), ec((size_t)WAVE, INFINITY), oc((size_t)WAVE);
            std::vector<int32_t> st((size_t)WAVE, FOT_ST_DROPPED), ix((size_t)WAVE, -1), ei((size_t)WAVE, -1), oi((size_t)WAVE);
            std::vector<int32_t> kp((size_t)WAVE, 0);
            for (int l = 0; l < n; ++l, ++index) {
                int v = (int)rnd((uint32_t)n_values);
                if (with_nonfinite && rnd(4) == 0) v = 5 + (int)rnd(2);
                c[(size_t)l] = values[v]; ix[(size_t)l] = index; kp[(size_t)l] = 1 + (int)rnd(250);
                st[(size_t)l] = rnd(3) ? FOT_ST_OK : (int)rnd(6);
                if (st[(size_t)l] == FOT_ST_OK && c[(size_t)l] < want_cost) {        // the reference's loop
                    want_cost = c[(size_t)l]; want_idx = index; want_keep = kp[(size_t)l];
                }
            }
            emu_select_entries(WAVE, st.data(), c.data(), ix.data(), ec.data(), ei.data());
            differences += emu_merge_butterfly(ec.data(), ei.data(), oc.data(), oi.data());
            p_cost[(size_t)t] = oc[0]; p_idx[(size_t)t] = oi[0];
            p_keep[(size_t)t] = oi[0] >= 0 ? kp[(size_t)(oi[0] - ix[0])] : 0;
        }
        double got_cost; int32_t got_idx, got_keep;
        differences += emu_merge_strided(n_parts, p_cost.data(), p_idx.data(), p_keep.data(), &got_cost, &got_idx, &got_keep);
        differences += got_idx != want_idx || got_keep != want_keep || (want_idx >= 0 && got_cost != want_cost);
        for (int rep = 0; rep < 3; ++rep) {
            for (int t = 0; t < n_parts; ++t) perm[(size_t)t] = t;
            for (int t = n_parts - 1; t > 0; --t) std::swap(perm[(size_t)t], perm[(size_t)rnd((uint32_t)t + 1)]);
            emu_merge_serial(n_parts, p_cost.data(), p_idx.data(), perm.data(), &got_cost, &got_idx);
            differences += got_idx != want_idx || (want_idx >= 0 && got_cost != want_cost);
        }
    }
    std::printf("sets %d differences %d\n", n_sets, differences);
    return differences ? 1 : 0;
}
#endif
