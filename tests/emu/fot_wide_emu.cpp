// fot_wide_emu.cpp -- TEST-ONLY: the sample-mask forms of csrc/fot_math.hpp on the host.
//
// A prediction distribution of up to 64 samples counts its DISTINCT hitting samples in one 64-bit word, one of up to
// FOT_MAX_PLAN_SAMPLES = 254 samples in a SampleMask4 (the wide launches of a handle with a raised sample capacity).
// This program runs, for ONE instance and every candidate of its lattice, each portable form of that count:
//   definition   collide_candidate (words = 1) / collide_candidate_wide (words = 4) on the candidate's recorded points
//   collider     EntryColliderT<false, words> fed by evaluate_candidate, in one piece
//   segments     the same in 2, 3 and 4 time segments, the segments' masks OR-ed and counted (k_evaluate_split*)
//   lean         EntryColliderT<true, words>, where the instance is eligible (no budget, no footprint, <= 64 steps):
//                for words = 4 the re-check that never looks at a sample id
// and returns each form's status table (final_status applied), for tests/test_wide_samples_cpu.py to hold against the
// oracle.  The entry lists are the whole obstacle set of each step's time row (no broad phase: the colliders' float32
// filter and exact re-check see every entry).  Helpers (nearest point, sinks) are fot_emu.cpp's.
#include "fot_emu.cpp"

namespace {

template <int W> struct Definition;
template <> struct Definition<1> {
    template <class Src> static bool collide(const DevParams &P, const InstDesc &D, const ObstacleView &o, int keep, const Src &s)
    { return collide_candidate(P, D, o, keep, s); }
};
template <> struct Definition<WIDE_MASK_WORDS> {
    template <class Src> static bool collide(const DevParams &P, const InstDesc &D, const ObstacleView &o, int keep, const Src &s)
    { return collide_candidate_wide(P, D, o, keep, s); }
};

template <int W>
int wide_tables(const fot_params *params, int n_knots, const double *wx, const double *wy, const fot_batch *b, int cap,
                int32_t *st_def, int32_t *st_col, int32_t *st_seg /* [3][cap] */, int32_t *st_lean, int32_t *n_cand_out,
                int32_t *lean_eligible, std::string &err)
{
    DevParams P;
    int rc = build_dev_params(*params, P, err);
    HostSpline hs;
    if (rc == FOT_OK) rc = build_spline(n_knots, wx, wy, hs, err);
    BatchLayout L;
    TileShapes shapes;
    if (rc == FOT_OK) build_tile_shapes(P, shapes);
    if (rc == FOT_OK) rc = build_batch_layout(*params, P, shapes, *b, L, err, W == 1 ? FOT_MAX_SAMPLES : FOT_MAX_PLAN_SAMPLES);
    if (rc != FOT_OK) return rc;
    if (L.n_inst != 1) { err = "one instance"; return FOT_ERR_INVALID; }
    const SplineView sp = spline_view(hs);
    const InstDesc &D = L.desc[0];
    if (b->obstacle_dtype != FOT_F64) { err = "float64 obstacles"; return FOT_ERR_INVALID; }
    InstState S;
    if (!emu_frenet_state(P, D, sp, D.ego.prev_s, S)) { err = "no Frenet state"; return FOT_ERR_INVALID; }
    *n_cand_out = S.n_cand;
    if (S.n_cand > cap) { err = "table too small"; return FOT_ERR_INVALID; }

    ObstacleView obs;
    obs.dtype = FOT_F64;
    obs.stat = b->static_xy ? (const char *)b->static_xy + 16 * (size_t)D.static_off : nullptr;
    obs.dyn = b->dyn_xy ? (const char *)b->dyn_xy + 16 * (size_t)D.dyn_off : nullptr;
    const int n_dyn = D.dyn_mode != FOT_DYN_NONE ? D.S * D.P : 0;
    std::vector<uint8_t> nan_track((size_t)n_dyn + 1, 0);
    for (int j = 0; j < n_dyn; ++j)
        for (int t = 0; t < D.T; ++t) {
            const d2 o = obs.dyn_at(j / D.P, j % D.P, t, D.P, D.T);
            if (o.x != o.x || o.y != o.y) nan_track[(size_t)j] = 1;
        }
    obs.nan_track = nan_track.data();
    // entry lists: every obstacle of the step's time row, FAR32 / SID_STATIC padding up to ent_cap
    const size_t ecap = (size_t)D.ent_cap;
    f2 farq; farq.x = FAR32; farq.y = FAR32;
    d2 infq; infq.x = INFINITY; infq.y = INFINITY;
    std::vector<f2> e32(ecap * P.n_total + 16, farq);
    std::vector<d2> e64(ecap * P.n_total + 16, infq);
    std::vector<uint8_t> sid(ecap * P.n_total + 16, SID_STATIC);
    std::vector<uint32_t> rng((size_t)P.n_total, 0u);
    for (int k = 0; k < P.n_total && D.ent_cap > 0; ++k) {
        const int row = k < D.T - 1 ? k : D.T - 1;
        size_t n = 0;
        for (int i = 0; i < D.n_static + n_dyn; ++i) {
            d2 o; int s = SID_STATIC;
            if (i < D.n_static) o = obs.static_at(i);
            else {
                const int j = i - D.n_static;
                if (nan_track[(size_t)j]) continue;
                o = obs.dyn_at(j / D.P, j % D.P, row, D.P, D.T); s = j / D.P;
            }
            ent32_store(e32.data(), (int64_t)ecap * k + (int64_t)n, (float)(o.x - D.ego.x), (float)(o.y - D.ego.y));
            e64[ecap * k + n] = o; sid[ecap * k + n] = (uint8_t)s;
            ++n;
        }
        if (n > ecap) { err = "entry list overflow"; return FOT_ERR_INVALID; }
        rng[(size_t)k] = (uint32_t)((n + ENT_CHUNK - 1) / ENT_CHUNK);          // chunks [0, ceil(n / 8))
    }
    *lean_eligible = (P.n_total <= WAVE && !P.has_footprint && D.max_viol == 0) ? 1 : 0;

    const int n_grid_lon = P.n_ti * D.n_tv;
    std::vector<double> tab((size_t)LON_FIELDS * FOT_MAX_NT, 0.0);
    std::vector<d2> pts((size_t)P.n_circ * P.n_total);
    const LoopConst lc = loop_const(P, D);
    typedef EntryColliderT<false, W> Collider;
    for (int idx = 0; idx < S.n_cand; ++idx) {
        const CandDecode cd = decode_candidate(P, D, S.frenet0, idx);
        LonInfo Li;
        if (cd.lon_slot < n_grid_lon) {
            const int ti = cd.lon_slot / D.n_tv, itv = cd.lon_slot - ti * D.n_tv;
            lon_coeffs(S.frenet0, tv_value(P, D, itv), P.ti[ti], Li);
            Li.n_t = P.ti[ti].n_t; Li.n_eval = Li.n_t;
        } else {
            const TimeInfo &tb = P.brake[cd.lon_slot - n_grid_lon];
            lon_coeffs(S.frenet0, 0.0, tb, Li);
            Li.n_t = P.n_total; Li.n_eval = tb.n_t;
        }
        double js = 0.0, sd_last = 0.0;
        for (int k = 0; k < Li.n_t; ++k) {
            LonSample ls; double sddd;
            make_lon_sample(sp, Li, k, P.dt, ls, sddd);
            tab[0 * FOT_MAX_NT + k] = ls.s; tab[1 * FOT_MAX_NT + k] = ls.sd; tab[2 * FOT_MAX_NT + k] = ls.sdd;
            tab[3 * FOT_MAX_NT + k] = ls.rx; tab[4 * FOT_MAX_NT + k] = ls.ry;
            tab[5 * FOT_MAX_NT + k] = ls.cos_r; tab[6 * FOT_MAX_NT + k] = ls.sin_r;
            tab[7 * FOT_MAX_NT + k] = ls.kr; tab[8 * FOT_MAX_NT + k] = ls.dkr; tab[9 * FOT_MAX_NT + k] = ls.inv_sd;
            js += sddd * sddd; sd_last = ls.sd;
        }
        Li.Js = js; Li.sd_last = sd_last;
        double q[6];
        lat_coeffs(S.frenet0, cd.di, cd.brake ? P.brake[cd.ti] : P.ti[cd.ti], q);
        const GlobalTab gt = { tab.data() };
        const auto fin = [&](const CandResult &r) { return final_status(r.status, r.v_last, r.travel, D.max_stop); };
        const auto arm = [&](auto &c) {
            c.init(P, D);
            c.rng = D.ent_cap > 0 ? rng.data() : nullptr;
            c.e32 = e32.data(); c.e64 = e64.data(); c.sid = sid.data();
        };
        {   // the definition on the recorded points
            VecSink vs = { &pts, P.n_total };
            CandResult rk;
            evaluate_candidate(P, D, lc, Li, gt, q, P.n_total, vs, rk);
            if (rk.status == ST_PENDING && D.ent_cap > 0) {
                VecSource src = { pts.data(), P.n_total };
                if (Definition<W>::collide(P, D, obs, rk.keep, src)) rk.status = FOT_ST_COLLISION;
            }
            st_def[idx] = fin(rk);
        }
        {   // the collider in one piece
            Collider ec;
            arm(ec);
            CandResult r;
            evaluate_candidate(P, D, lc, Li, gt, q, P.n_total, ec, r);
            st_col[idx] = fin(r);
        }
        for (int n_seg = 2; n_seg <= 4; ++n_seg) {                        // time segments, masks merged by OR, then counted
            const int n_loop = P.n_total, seg_len = (n_loop + n_seg - 1) / n_seg;
            SegState g;
            typename Collider::Mask hit_mask = typename Collider::Mask();
            bool hit = false;
            for (int sg = 0; sg < n_seg; ++sg) {
                if (sg > 0 && sg * seg_len >= Li.n_t) break;
                Collider es;
                arm(es);
                SegState part;
                seg_init(part);
                evaluate_segment(P, lc, Li, gt, q, sg * seg_len, std::min(n_loop, (sg + 1) * seg_len), es, part);
                bool counts = true;
                if (sg == 0) g = part; else counts = seg_merge(g, part);
                if (counts) { mask_or(hit_mask, es.hit_mask); hit |= es.hit; }
            }
            hit |= mask_count(hit_mask) > D.max_viol;
            CandResult rs;
            finish_candidate(P, D, Li, gt, q, g, hit, rs);
            st_seg[(size_t)(n_seg - 2) * cap + idx] = fin(rs);
        }
        st_lean[idx] = -1;
        if (*lean_eligible) {
            EntryColliderT<true, W> el;
            arm(el);
            CandResult r;
            evaluate_candidate<true>(P, D, lc, Li, gt, q, P.n_total, el, r);
            st_lean[idx] = fin(r);
        }
    }
    return FOT_OK;
}

}  // namespace

// words: 1 (the forms every launch of up to 64 samples runs) or 4 (the wide forms).  Tables of `cap` entries each
// (st_seg: three, for 2, 3 and 4 segments); st_lean is -1 throughout where the instance is not lean-eligible.
extern "C" int emu_wide_tables(int words, const fot_params *params, int n_knots, const double *wx, const double *wy,
                               const fot_batch *b, int cap, int32_t *st_def, int32_t *st_col, int32_t *st_seg,
                               int32_t *st_lean, int32_t *n_cand, int32_t *lean_eligible, char *errbuf)
{
    std::string err;
    int rc = FOT_ERR_INVALID;
    if (words == 1)
        rc = wide_tables<1>(params, n_knots, wx, wy, b, cap, st_def, st_col, st_seg, st_lean, n_cand, lean_eligible, err);
    else if (words == WIDE_MASK_WORDS)
        rc = wide_tables<WIDE_MASK_WORDS>(params, n_knots, wx, wy, b, cap, st_def, st_col, st_seg, st_lean, n_cand,
                                          lean_eligible, err);
    else err = "words: 1 or 4";
    if (rc != FOT_OK && errbuf) std::strncpy(errbuf, err.c_str(), 255);
    return rc;
}
