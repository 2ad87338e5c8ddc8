// fot_head_templates_emu.cpp -- TEST-ONLY: a group header composed from the handle's header templates (csrc/fot_types.h
// HeadTemplate, csrc/fot_setup.hpp build_head_templates, csrc/fot_math.hpp group_head_compose) against build_group_head,
// the derivation k_frenet_state ran per instance before the templates existed, on the host.
//
// The harness does what the library does per handle: the tile tables of all its scenarios under the grouped cut, their
// concatenation, the templates of every group of every lattice shape in both variants.  Then, for every
// scenario and grid size, an instance in five states of the ego -- moving, just over the brake gate, AT the gate
// (0.1 m/s: no ladder), standing, no Frenet state -- gets its header at every position of the handle's longest shape
// twice: from build_group_head, and from the sixteen lanes of group_head_compose on the template that
// head_template_index picks.  The two must agree in every named field of a full header, the profile summaries (LonInfo)
// bit for bit; an EMPTY header in `present` and `grp_tile0`, an ABSENT one in `present`, and in both what is not written
// must still be what the table held before.
//
// A program of its own (main below), so that it can be built with -fsanitize=address,undefined and run as it is:
//     fot_head_templates_emu <cases.bin>      one line per handle, exit status 1 on any difference
// cases.bin: per handle an int32 count of scenarios, then that many fot_params structs (tests/test_head_templates_cpu.py).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_math.hpp"
#include "../../integrated_path_planning_amd/csrc/fot_setup.hpp"

using namespace fot;

namespace {

struct Field { const char *name; size_t off, size; };
#define F(m) { #m, offsetof(GroupHead, m), sizeof(((GroupHead *)0)->m) }
const Field FIELDS[] = {
    F(present), F(grp_tile0), F(slot_lo), F(n_stage), F(total_rows), F(n_total), F(n_circ_fp), F(cand_off), F(tile0),
    F(ent_cap), F(max_viol), F(n_grid), F(n_tv), F(n_di), F(n_side), F(n_ti), F(row0), F(t_cand0), F(t_n), F(t_n_loop),
    F(t_own_lo), F(t_own_hi), F(ent_off), F(d_road_w), F(dt), F(road_lim), F(lim_speed), F(lim_accel), F(lim_curv),
    F(lim_lat), F(ego_x), F(ego_y), F(frenet0), F(info),
};
#undef F

struct Tally {
    long heads = 0, full = 0, empty = 0, absent = 0, clipped = 0, profiles = 0, differences = 0;
    char first[200] = "";
};

void differ(Tally &T, int scen, int n_tv, int state_id, int pos, const char *what)
{
    if (!T.differences++)
        std::snprintf(T.first, sizeof T.first, "scen=%d n_tv=%d state=%d pos=%d: %s", scen, n_tv, state_id, pos, what);
}

// one header both ways
void check_head(const DevParams &P, const InstDesc &D, const InstState &S, const int32_t *tc, const int32_t *tn,
                const std::vector<HeadTemplate> &tmpl, int n_entries, int pos, int state_id, Tally &T)
{
    GroupHead want, got;
    std::memset((void *)&want, 0xa5, sizeof want);              // (a reused table: whatever an earlier call left)
    std::memset((void *)&got, 0xa5, sizeof got);
    build_group_head(P, D, S.frenet0, S.c2f_ok, S.n_cand, tc, tn, pos, want);
    const int variant = S.n_brake > 0 ? HEAD_VARIANT_BRAKE : HEAD_VARIANT_GRID;
    const size_t at = (size_t)head_template_index(D, variant, n_entries, pos);
    if (at >= tmpl.size()) { differ(T, D.scen, D.n_tv, state_id, pos, "template index beyond the table"); return; }
    for (int p = 0; p < GROUP_MAX_PROFILES; ++p) group_head_compose(P, D, S.frenet0, S.c2f_ok, tmpl[at], p, got);
    ++T.heads;
    if (got.present != want.present) { differ(T, D.scen, D.n_tv, state_id, pos, "present"); return; }
    if (want.present == GROUP_HEAD_FULL) {
        ++T.full;
        for (const Field &f : FIELDS)
            if (std::memcmp((const char *)&got + f.off, (const char *)&want + f.off, f.size) != 0)
                differ(T, D.scen, D.n_tv, state_id, pos, f.name);
        T.profiles += want.n_stage;
        for (int t = 0; t < GROUP_TILES; ++t) T.clipped += want.t_n[t] != tn[D.shape_off + want.grp_tile0 + t];
        // behind the last field nothing is written
        const size_t end = offsetof(GroupHead, info) + sizeof want.info;
        if (std::memcmp((const char *)&got + end, (const char *)&want + end, sizeof want - end) != 0)
            differ(T, D.scen, D.n_tv, state_id, pos, "bytes behind info");
    } else {
        // ABSENT: `present` is the only word that is written; EMPTY: `grp_tile0` too -- so the whole records agree
        ++(want.present == GROUP_HEAD_EMPTY ? T.empty : T.absent);
        if (std::memcmp(&got, &want, sizeof want) != 0)
            differ(T, D.scen, D.n_tv, state_id, pos, want.present == GROUP_HEAD_EMPTY ? "an empty header" : "an absent header");
    }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int handle = 0, bad = 0;
    int32_t n_scen = 0;
    while (std::fread(&n_scen, sizeof n_scen, 1, f) == 1) {
        if (n_scen < 1 || n_scen > FOT_MAX_SCENARIOS) { std::fprintf(stderr, "bad scenario count %d\n", n_scen); return 2; }
        std::vector<fot_params> params((size_t)n_scen);
        if (std::fread(params.data(), sizeof(fot_params), (size_t)n_scen, f) != (size_t)n_scen) { std::fprintf(stderr, "short file\n"); return 2; }
        std::vector<DevParams> P((size_t)n_scen);
        std::string err;
        bool ok = true;
        for (int s = 0; s < n_scen; ++s) ok = ok && build_dev_params(params[(size_t)s], P[(size_t)s], err) == FOT_OK;
        if (!ok) {                                               // beyond a FOT_MAX_* limit: not a handle libfot makes
            std::printf("%d rc -1\n", handle++);
            continue;
        }
        // the handle's tables, as upload_tile_shapes puts them together
        std::vector<const DevParams *> ps((size_t)n_scen);
        for (int s = 0; s < n_scen; ++s) ps[(size_t)s] = &P[(size_t)s];
        std::vector<TileShapes> shapes((size_t)n_scen);
        build_tile_shapes(ps.data(), n_scen, shapes.data(), TILE_CUT_GROUP);
        std::vector<int32_t> cand0, nn;
        std::vector<ScenarioRef> refs((size_t)n_scen);
        for (int s = 0; s < n_scen; ++s) {
            refs[(size_t)s].hp = &params[(size_t)s]; refs[(size_t)s].P = &P[(size_t)s];
            refs[(size_t)s].shapes = &shapes[(size_t)s]; refs[(size_t)s].shape_base = (int32_t)cand0.size();
            cand0.insert(cand0.end(), shapes[(size_t)s].cand0.begin(), shapes[(size_t)s].cand0.end());
            nn.insert(nn.end(), shapes[(size_t)s].n.begin(), shapes[(size_t)s].n.end());
        }
        const int n_entries = head_template_entries(refs.data(), n_scen);
        std::vector<HeadTemplate> tmpl;
        build_head_templates(refs.data(), n_scen, cand0.data(), nn.data(), n_entries, tmpl);
        int n_pos = 0;                                           // positions of the handle's longest shape
        for (int s = 0; s < n_scen; ++s)
            for (int n_tv = 1; n_tv <= FOT_MAX_TV; ++n_tv) n_pos = std::max(n_pos, shapes[(size_t)s].tiles_of(n_tv) / GROUP_TILES);

        Tally T;
        for (int s = 0; s < n_scen; ++s) {
            const DevParams &Ps = P[(size_t)s];
            for (int n_tv = 1; n_tv <= FOT_MAX_TV; ++n_tv) {
                InstDesc D = shape_desc(Ps, n_tv);
                D.scen = s;
                D.shape_off = refs[(size_t)s].shape_base + shapes[(size_t)s].off[n_tv];
                D.n_tiles = shapes[(size_t)s].tiles_of(n_tv);
                D.ego.x = 12.5 + n_tv; D.ego.y = -3.25 - s;
                D.target_speed = 0.75 * Ps.d_t_s * n_tv; D.n_down = n_tv - 1 - (n_tv > 1 ? 1 : 0);
                D.lim_speed = 13.0 + s; D.lim_accel = 2.5; D.lim_curv = 0.9; D.lim_lat = 3.5;
                D.cand_off = 64 * n_tv; D.tile0 = 7 * n_tv + s; D.ent_cap = 16 * (n_tv % 3);
                D.ent_off = ((int64_t)1 << 33) + 1024 * n_tv;
                D.max_viol = n_tv % 2;
                for (int state_id = 0; state_id < 5; ++state_id) {
                    InstState S = InstState();
                    const double sd = state_id == 0 ? 6.5 : state_id == 1 ? 0.11 : state_id == 2 ? 0.1 : 0.0;
                    const double fr[6] = { 17.25, sd, state_id == 0 ? 0.4 : 0.0, 0.35, state_id == 0 ? -0.2 : 0.0, 0.05 };
                    S.c2f_ok = state_id == 4 ? 0 : 1;
                    for (int i = 0; i < 6; ++i) S.frenet0[i] = S.c2f_ok ? fr[i] : NAN;
                    S.n_brake = (S.c2f_ok && fr[1] > 0.1) ? Ps.n_brake : 0;                  // (k_frenet_state's gate)
                    S.n_cand = S.c2f_ok ? D.n_grid + S.n_brake : 0;
                    for (int pos = 0; pos < n_pos; ++pos)
                        check_head(Ps, D, S, cand0.data(), nn.data(), tmpl, n_entries, pos, state_id, T);
                }
            }
        }
        // (positions: of the handle's longest shape; tiles1: tiles with candidates of scenario 0's one-speed shape)
        int tiles1 = 0;
        for (int t = shapes[0].off[1]; t < shapes[0].off[2]; ++t) tiles1 += shapes[0].n[(size_t)t] > 0;
        std::printf("%d rc 0 heads %ld full %ld empty %ld absent %ld clipped %ld profiles %ld positions %d tiles1 %d differences %ld %s\n",
                    handle++, T.heads, T.full, T.empty, T.absent, T.clipped, T.profiles, n_pos, tiles1, T.differences, T.first);
        bad += T.differences != 0;
    }
    std::fclose(f);
    return bad ? 1 : 0;
}
