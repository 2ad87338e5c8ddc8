// fot_host.cpp -- the handle and plan unit of the C ABI of libfot.so (include/fot.h): handle lifetime, paths and
// scenarios, the enqueue machinery of a plan call, the plan entry points and their debug and wire entries.
// No torch, no oracle, no CPU fallback: every entry point drives the gfx950 kernels or fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "fot_host.hpp"
#include "fot_kernels.h"

namespace {

thread_local std::string g_create_error;

// Every handle fot_create returned and fot_destroy has not taken back: fot_destroy of anything else (a second destroy,
// a stale pointer) is a no-op instead of a double free, and a binding can ask how many it still owns (fot_live_handles).
std::mutex g_live_mu;
std::unordered_set<fot_handle *> &live_handles()
{
    static std::unordered_set<fot_handle *> *s = new std::unordered_set<fot_handle *>();   // (never destroyed: no static
    return *s;                                                                            //  destructor order to lose)
}

// Teardown never blocks for good.  Work the handle enqueued may sit on a CALLER's stream (fot_plan_batch_device on a
// PyTorch stream) whose owner is free to have destroyed it, and a destroy may run while the process is exiting: the
// handle's streams and its ordering event are POLLED (hipStreamQuery / hipEventQuery) for a bounded time; if they do
// not drain, or the runtime answers with an error, the device and pinned memory is left to the process teardown
// instead of being freed under work that may still touch it.
double destroy_timeout_s()
{
    if (const char *ev = std::getenv("FOT_DESTROY_TIMEOUT_MS")) { const double v = std::atof(ev); if (v >= 0.0) return v * 1e-3; }
    return 5.0;
}

template <class Query>
bool drained(const Query &query, double seconds)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = query();
        if (e == hipSuccess) return true;
        if (e != hipErrorNotReady) { (void)hipGetLastError(); return false; }   // stream / context gone: nothing to wait for, nothing to free
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

void destroy_handle(fot_handle *h)
{
    const double budget = destroy_timeout_s();
    bool quiet = hipSetDevice(h->device) == hipSuccess;
    // the handle's own stream, the lanes' streams, and the event behind its last enqueue (which may be on a caller's
    // stream): polled, never waited on
    if (quiet && h->stream) quiet = drained([&] { return hipStreamQuery(h->stream); }, budget);
    if (quiet && h->order_valid) quiet = drained([&] { return hipEventQuery(h->order_done); }, budget);
    for (Workspace &w : h->ws) if (quiet && w.stream) quiet = drained([&] { return hipStreamQuery(w.stream); }, budget);
    if (!quiet) {
        // something is still running (or the runtime is already gone): the host-side struct goes, everything the device
        // may still touch stays until the process ends
        (void)hipGetLastError();
        delete h;
        return;
    }
    for (Scenario &S : h->sc) S.dSpline.release();
    DevBuf *bufs[] = { &h->dP, &h->dSplineTab, &h->dShapes, &h->dHeadTmpl, &h->dUserStatic, &h->dUserDyn, &h->dOut, &h->dTmpA, &h->dTmpB, &h->dTmpC, &h->dTmpD
                     };
    for (DevBuf *b : bufs) b->release();
    for (Workspace &w : h->ws) w.release();
    h->hSmallIn.release(); h->hSmallOut.release(); h->hRecOut.release(); h->hDone.release();
    h->hScoreIn.release(); h->hScoreOut.release(); h->dScoreT.release();
    for (fot_handle::Sgan &g : h->sgan) g.release();
    h->ol.release();
    h->fp.release();
    h->fid.release();
    h->enc.release();
    h->loop.release();
    for (hipEvent_t e : h->prof_pool) (void)hipEventDestroy(e);
    if (h->fork) (void)hipEventDestroy(h->fork);
    if (h->order_done) (void)hipEventDestroy(h->order_done);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// the SplineView of every scenario, in HBM (a scenario without a path yet: an empty view no batch can reach)
int upload_spline_table(fot_handle *h)
{
    std::vector<SplineView> tab(h->sc.size());
    for (size_t s = 0; s < h->sc.size(); ++s) tab[s] = spline_view(h, (int)s);
    HIP_TRY(h, h->dSplineTab.ensure(sizeof(SplineView) * tab.size()));
    HIP_TRY(h, hipMemcpy(h->dSplineTab.p, tab.data(), sizeof(SplineView) * tab.size(), hipMemcpyHostToDevice));
    return FOT_OK;
}

// scenario `scen`'s spline into HBM (its coefficient arrays and its entry of the SplineView table)
int upload_spline(fot_handle *h, int scen = 0)
{
    Scenario &S = h->sc[(size_t)scen];
    const int n = S.spline.n;
    std::vector<double> flat((size_t)9 * n, 0.0);
    const std::vector<double> *src[9] = { &S.spline.s, &S.spline.ax, &S.spline.bx, &S.spline.cx, &S.spline.dx,
                                          &S.spline.ay, &S.spline.by, &S.spline.cy, &S.spline.dy };
    for (int f = 0; f < 9; ++f)
        std::memcpy(flat.data() + (size_t)f * n, src[f]->data(), sizeof(double) * std::min((size_t)n, src[f]->size()));
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // nothing may still be reading the old spline
    HIP_TRY(h, S.dSpline.ensure(flat.size() * sizeof(double)));
    HIP_TRY(h, hipMemcpy(S.dSpline.p, flat.data(), flat.size() * sizeof(double), hipMemcpyHostToDevice));
    { int r = upload_spline_table(h); if (r != FOT_OK) return r; }
    S.has_path = true;
    S.flat_path = spline_is_flat(S.spline);                      // (every fot_set_path_* route ends here)
    h->last_valid = false;
    return FOT_OK;
}

// the DevParams of every scenario, element s = scenario s, into HBM
int upload_params(fot_handle *h)
{
    std::vector<DevParams> tab(h->sc.size());
    for (size_t s = 0; s < h->sc.size(); ++s) tab[s] = h->sc[s].P;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // nothing may still be reading the old table
    HIP_TRY(h, h->dP.ensure(sizeof(DevParams) * tab.size()));
    HIP_TRY(h, hipMemcpy(h->dP.p, tab.data(), sizeof(DevParams) * tab.size(), hipMemcpyHostToDevice));
    h->last_valid = false;
    return FOT_OK;
}

// (re)builds the tile tables of all scenarios for the given cut (one cut per handle) and puts their concatenation into
// HBM: cand0[] | n[] | span[]; with them the group-header templates of a grouped cut, which are a function of the table
int upload_tile_shapes(fot_handle *h, int cut)
{
    const size_t n_sc = h->sc.size();
    std::vector<const DevParams *> ps(n_sc);
    std::vector<TileShapes> shapes(n_sc);
    for (size_t s = 0; s < n_sc; ++s) ps[s] = &h->sc[s].P;
    build_tile_shapes(ps.data(), (int)n_sc, shapes.data(), cut);
    std::vector<int32_t> cand0, nn, span;
    for (size_t s = 0; s < n_sc; ++s) {
        h->sc[s].shape_base = (int32_t)cand0.size();
        cand0.insert(cand0.end(), shapes[s].cand0.begin(), shapes[s].cand0.end());
        nn.insert(nn.end(), shapes[s].n.begin(), shapes[s].n.end());
        span.insert(span.end(), shapes[s].span.begin(), shapes[s].span.end());
        h->sc[s].shapes = std::move(shapes[s]);
    }
    h->refs.assign(n_sc, ScenarioRef());
    for (size_t s = 0; s < n_sc; ++s) {
        h->refs[s].hp = &h->sc[s].params; h->refs[s].P = &h->sc[s].P;
        h->refs[s].shapes = &h->sc[s].shapes; h->refs[s].shape_base = h->sc[s].shape_base;
    }
    h->tile_cut = cut;
    std::vector<HeadTemplate> tmpl;
    h->head_tmpl_entries = head_template_entries(h->refs.data(), (int)n_sc);
    if (h->head_tmpl_entries > 0)
        build_head_templates(h->refs.data(), (int)n_sc, cand0.data(), nn.data(), h->head_tmpl_entries, tmpl);
    const size_t nt = cand0.size();
    h->n_shape_entries = (int32_t)nt;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // nothing may still be reading the old table
    HIP_TRY(h, h->dShapes.ensure(sizeof(int32_t) * 3 * std::max<size_t>(nt, 1)));
    if (nt) {
        HIP_TRY(h, hipMemcpy(h->dShapes.p, cand0.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->dShapes.as<int32_t>() + nt, nn.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->dShapes.as<int32_t>() + 2 * nt, span.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
    }
    if (!tmpl.empty()) {
        HIP_TRY(h, h->dHeadTmpl.ensure(sizeof(HeadTemplate) * tmpl.size()));
        HIP_TRY(h, hipMemcpy(h->dHeadTmpl.p, tmpl.data(), sizeof(HeadTemplate) * tmpl.size(), hipMemcpyHostToDevice));
    }
    h->last_valid = false;
    return FOT_OK;
}

// the paths of a batch laid out by L: its one scenario's in the kernel arguments, or the table of a mixed batch
PathSet path_set(const fot_handle *h, const BatchLayout &L, const DevParams **P_launch)
{
    const DevParams *dP = h->dP.as<DevParams>();
    if (L.scens.size() <= 1) {
        const int s = L.scens.empty() ? 0 : L.scens[0];
        *P_launch = dP + s;
        return PathSet::single(spline_view(h, s));
    }
    PathSet ps;
    ps.table = h->dSplineTab.as<SplineView>();
    ps.mixed = 1;
    for (int s : L.scens) ps.knots[ps.n_knots++] = h->sc[(size_t)s].spline.n;
    *P_launch = dP;
    return ps;
}

const char *const kKernelNames[FOT_PROFILE_KERNELS] = { "k_frenet_state", "k_cull", "k_evaluate" };

// accumulate finished event pairs into the per-kernel totals (waits for them)
int prof_drain(fot_handle *h)
{
    for (size_t i = 0; i < h->prof_kernel.size(); ++i) {
        hipEvent_t a = h->prof_pool[2 * i], b = h->prof_pool[2 * i + 1];
        HIP_TRY(h, hipEventSynchronize(b));
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, a, b));
        h->prof_launches[h->prof_kernel[i]] += 1;
        h->prof_ms[h->prof_kernel[i]] += (double)ms;
    }
    h->prof_kernel.clear();
    h->prof_used = 0;
    return FOT_OK;
}

// Stage descriptors, size the lane's workspace and enqueue the whole pipeline for the sub-batch `b` on `st`.
// d_static / d_dyn are device pointers to the caller's obstacle coordinates (offsets in b are absolute),
// d_out the device fot_result slot of the sub-batch's first instance.
// sync_caller: see enqueue_plan.
// d_dyn_stage: HBM block the NaN-scan blocks copy the dynamic tensors into as they read them (a small call's tensors
// lie in pinned host memory: the later kernels then read the copy instead of crossing PCIe again), or nullptr.
int enqueue_lane(fot_handle *h, Workspace &w, const fot_batch &b, const int32_t *scen, const void *d_static,
                 const void *d_dyn, fot_result *d_out, hipStream_t st, bool sync_caller = false, void *d_dyn_stage = nullptr)
{
    BatchLayout &L = w.last;
    std::string err;
    int rc = build_batch_layout(h->refs.data(), (int)h->refs.size(), scen, b, L, err, h->sample_cap);
    if (rc != FOT_OK) return fail(h, rc, err);
    if (L.n_inst == 0) return FOT_OK;

    // --- staging: the descriptors in a pinned block (k_frenet_state pulls them into HBM)
    const size_t desc_bytes = align256(sizeof(InstDesc) * (size_t)L.n_inst);
    const size_t meta_bytes = desc_bytes;
    const int slot = (w.staging_slot ^= 1);
    if (w.staging_pending[slot]) { HIP_TRY(h, hipEventSynchronize(w.staging_done[slot])); w.staging_pending[slot] = false; }
    HIP_TRY(h, w.staging[slot].ensure(desc_bytes));
    char *stg = (char *)w.staging[slot].p;
    std::memcpy(stg, L.desc.data(), sizeof(InstDesc) * (size_t)L.n_inst);

    // --- workspace (grow-only; a growing hipFree/hipMalloc synchronises, steady state does not)
    const DevParams &P = h->sc[0].P;                             // (n_total: the same in every scenario)
    HIP_TRY(h, w.dMeta.ensure(meta_bytes));
    HIP_TRY(h, w.dState.ensure(sizeof(InstState) * (size_t)L.n_inst));
    const size_t slots = (size_t)std::max<int64_t>(L.n_slots, 1);
    HIP_TRY(h, w.dCost.ensure(sizeof(double) * slots));
    HIP_TRY(h, w.dParts.ensure(sizeof(TilePart) * (size_t)std::max(L.n_tiles, 1)));
    HIP_TRY(h, w.dStatus.ensure(slots));
    HIP_TRY(h, w.dKeep.ensure(sizeof(uint16_t) * slots));
    const size_t n_ent = (size_t)L.n_entries + 64;              // slack: the scalar prefetch reads one chunk ahead
    HIP_TRY(h, w.dEntCnt.ensure(sizeof(int32_t) * (size_t)P.n_total * (size_t)L.n_inst));
    HIP_TRY(h, w.dEnt32.ensure(sizeof(f2) * n_ent));
    HIP_TRY(h, w.dEnt64.ensure(sizeof(d2) * n_ent));
    HIP_TRY(h, w.dEntSid.ensure(n_ent));
    HIP_TRY(h, w.dWaveRng.ensure(sizeof(TileStep) * (size_t)P.n_total * (size_t)std::max(L.n_tiles, 1)));
    HIP_TRY(h, w.dNanFlag.ensure((size_t)std::max<int64_t>(L.n_tracks, 16)));
    HIP_TRY(h, w.dDone.ensure(sizeof(int32_t) * (size_t)L.n_inst));

    // no H2D copy in front of the kernels: k_frenet_state pulls the staging block into HBM (one dependent hop less)
    w.staging_pending[slot] = true;

    const InstDesc *d_desc = (const InstDesc *)w.dMeta.p;
    TileTable tt;
    tt.cand0 = h->dShapes.as<int32_t>();
    tt.n = h->dShapes.as<int32_t>() + h->n_shape_entries;
    tt.span = h->dShapes.as<int32_t>() + 2 * (size_t)h->n_shape_entries;
    tt.n_tiles = L.n_tiles; tt.max_tiles = L.max_tiles; tt.row_budget = L.row_budget;
    tt.eval_segments = h->eval_segments;
    tt.grouped = L.grouped;
    // The lean evaluation kernels (FusedSink<true>): at most 64 samples per candidate and the single centre circle in
    // every scenario of the handle, no chance budget on any instance of this launch.  Anything else: the general form.
    tt.lean = h->eval_form == 0 ? 1 : 0;
    for (const Scenario &S : h->sc) if (S.P.n_total > WAVE || S.P.has_footprint) tt.lean = 0;
    for (int i = 0; i < L.n_inst && tt.lean; ++i) if (L.desc[(size_t)i].max_viol != 0) tt.lean = 0;
    // A wide launch: an instance of more than FOT_MAX_SAMPLES samples (only on a handle whose capacity was raised).  The
    // same rule picks its form; it has kernels of its own (FusedSink<., WIDE_MASK_WORDS>) and no flat form.  Every other
    // launch, raised capacity or not, goes where it went before.
    tt.wide = L.max_S > FOT_MAX_SAMPLES ? 1 : 0;
    h->last_eval_forms |= tt.wide ? (tt.lean ? 8 : 4) : tt.lean ? 2 : 1;
    // Their flat forms: every path the launch's instances use is exactly straight.  Decided from the paths' coefficients
    // (Scenario::flat_path) -- the lateral states need no test: frenet_to_cart<., true> keeps the one multiply-add
    // that poisons a sample whose d is not finite, as the general form's 1 - kr d does.
    tt.flat = tt.lean && !tt.wide && h->flat_mode != 0 ? 1 : 0;
    if (L.scens.empty()) { if (!h->sc[0].flat_path) tt.flat = 0; }
    for (int s : L.scens) if (!h->sc[(size_t)s].flat_path) tt.flat = 0;
    h->last_flat |= evaluate_flat(tt) ? 1 : 0;
    GroupHeadOut gh;                                             // the grouped kernels' headers: k_frenet_state builds them
    if (evaluate_in_groups(tt)) {
        gh.n_pos = L.max_tiles / GROUP_TILES;
        HIP_TRY(h, w.dHeads.ensure(sizeof(GroupHead) * (size_t)L.n_inst * (size_t)gh.n_pos));
        gh.heads = tt.heads = w.dHeads.as<GroupHead>();
        gh.tmpl = h->dHeadTmpl.as<HeadTemplate>(); gh.tmpl_entries = h->head_tmpl_entries;
        if (gh.tmpl_entries < 1) return fail(h, FOT_ERR_INVALID, "plan: no header templates for this handle's tile table");
    }
    const DevParams *dP = nullptr;
    const PathSet sv = path_set(h, L, &dP);
    CandArrays ca;
    ca.cost = w.dCost.as<double>(); ca.parts = w.dParts.as<TilePart>();
    ca.status = w.dStatus.as<uint8_t>(); ca.keep = w.dKeep.as<uint16_t>();
    if (sync_caller && h->done_seq_armed) { ca.done_flag = (int32_t *)h->hDone.p; ca.done_seq = h->done_seq; }

    EntryArrays ea;
    ea.cnt = w.dEntCnt.as<int32_t>(); ea.e32 = w.dEnt32.as<f2>(); ea.e64 = w.dEnt64.as<d2>();
    ea.sid = w.dEntSid.as<uint8_t>(); ea.rng = w.dWaveRng.as<TileStep>();
    ea.nan_flag = w.dNanFlag.as<uint8_t>();
    MetaImport imp;
    imp.h_desc = (const InstDesc *)stg;
    imp.d_desc = (InstDesc *)w.dMeta.p;
    // one scan block per 256 KB of an instance's tensor (few, fat blocks: each first reads its descriptor out of the
    // pinned staging block, a PCIe round trip), at most 64 per instance
    // Only time-major tensors are scanned (k_cull finds the NaN tracks of the caller's [S][P][T] layout itself, among the
    // few its boxes touch); a small call's tensors in pinned memory take the same blocks for their one pass over PCIe.
    // (FOT_NAN_SCAN=eager: the scan blocks for every layout, as before round 4 -- the scan then doubles as a prefetch of
    // the tensor into the memory-side cache: 4 us less on the serial step of config 4, the same step with three calls in
    // flight, the tensor read twice.  A small call's staging pass leaves the flags behind anyway: k_cull uses them.)
    static const bool eager_env = getenv("FOT_NAN_SCAN") && !std::strcmp(getenv("FOT_NAN_SCAN"), "eager");
    const bool eager_nan = eager_env || d_dyn_stage != nullptr;
    ea.eager_nan = eager_nan ? 1 : 0;
    NanScan scan;
    scan.eager = ea.eager_nan;
    if (L.n_tracks > 0 && (L.any_tmajor || eager_nan)) {
        scan.dyn_xy = d_dyn; scan.dtype = b.obstacle_dtype; scan.flag = w.dNanFlag.as<uint8_t>();
        scan.blocks_per_inst = (int)std::min<int64_t>(64, std::max<int64_t>(1, (L.max_dyn_bytes + 262143) / 262144));
        if (d_dyn_stage) {                                       // (cull and the rest read the copy)
            scan.stage = d_dyn_stage; d_dyn = d_dyn_stage;
            // across PCIe a block moves 64 KB per round trip: one block per 64 KB, so that the copy is done well inside
            // the nearest-point chain it runs beside
            scan.blocks_per_inst = (int)std::min<int64_t>(64, std::max<int64_t>(1, (L.max_dyn_bytes + 65535) / 65536));
        }
    }
    {
        ProfScope ps(h, 0, st);
        LAUNCH_TRY(h, launch_frenet_state(dP, sv, d_desc, w.dState.as<InstState>(), L.n_inst, imp, scan, w.dDone.as<int32_t>(), st, gh));
    }
    if (L.any_obstacles) {
        ProfScope ps(h, 1, st);
        LAUNCH_TRY(h, launch_cull(dP, d_desc, w.dState.as<InstState>(), L.n_inst, P.n_total, L.n_ext, sv,
                                  d_static, d_dyn, b.obstacle_dtype, ea, tt, st));
    }
    {
        ProfScope ps(h, 2, st);
        LAUNCH_TRY(h, launch_evaluate(dP, sv, d_desc, w.dState.as<InstState>(), P.n_total, L.n_inst, tt, ea, ca, d_out,
                                      w.dDone.as<int32_t>(), st));
    }
    HIP_TRY(h, hipEventRecord(w.staging_done[slot], st));        // (behind the call: see Workspace::staging_done)
    return FOT_OK;
}

// sub-batch [i0, i0+n) of b: per-instance arrays shifted, obstacle offsets stay absolute
fot_batch sub_batch(const fot_batch &b, int i0, int n)
{
    fot_batch s = b;
    s.n_inst = n;
    s.ego = b.ego + i0;
    s.target_speed = b.target_speed + i0;
    s.overrides = b.overrides ? b.overrides + i0 : nullptr;
    s.max_stop_distance = b.max_stop_distance ? b.max_stop_distance + i0 : nullptr;
    s.static_off = b.static_off ? b.static_off + i0 : nullptr;
    s.dyn_off = b.dyn_off ? b.dyn_off + i0 : nullptr;
    s.dyn_dims = b.dyn_dims ? b.dyn_dims + 4 * (size_t)i0 : nullptr;
    return s;
}

// lane and local index of global instance `inst` of the most recent plan call
Workspace *lane_of(fot_handle *h, int inst, int *local)
{
    for (int l = h->lanes_used - 1; l >= 0; --l)
        if (inst >= h->ws[l].first_inst && inst < h->ws[l].first_inst + h->ws[l].last.n_inst) {
            *local = inst - h->ws[l].first_inst;
            return &h->ws[l];
        }
    return nullptr;
}

// shared body of fot_check_collision_paths (mode 0) and fot_check_paths (mode 1)
int check_ext(fot_handle *h, int mode, int32_t n_paths, const int32_t *len, const int32_t *rule_len,
              const double *const arr[9], const fot_overrides *ov, double max_stop,
              int32_t n_static, const double *static_xy, int32_t dmode, int32_t S, int32_t Pn, int32_t T,
              const double *dyn, int32_t *status_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_paths <= 0) return FOT_OK;
    if (!len || !status_out) return fail(h, FOT_ERR_INVALID, "NULL path array");
    const DevParams &P = h->sc[0].P;
    // one single-instance batch carries limits + obstacle set
    fot_ego ego = {};
    double target = 0.0;
    int32_t soff[2] = { 0, n_static > 0 ? n_static : 0 };
    int64_t doff[1] = { 0 };
    int32_t dims[4] = { dmode, S, Pn, T };
    fot_batch b = {};
    b.n_inst = 1; b.obstacle_dtype = FOT_F64; b.ego = &ego; b.target_speed = &target;
    b.overrides = ov; b.max_stop_distance = &max_stop;
    b.static_xy = static_xy; b.static_off = soff; b.dyn_xy = dyn; b.dyn_off = doff; b.dyn_dims = dims;
    BatchLayout L;
    std::string err;
    int rc = build_batch_layout(h->sc[0].params, P, h->sc[0].shapes, b, L, err, h->sample_cap);
    if (rc != FOT_OK) return fail(h, rc, err);
    h->last_valid = false;

    const size_t np = (size_t)n_paths, plane = np * FOT_MAX_NT;
    std::vector<double> flat(9 * plane, 0.0);
    for (int i = 0; i < n_paths; ++i)
        if (len[i] < 0 || len[i] > FOT_MAX_NT) return fail(h, FOT_ERR_INVALID, "path length out of range");
    for (int f = 0; f < 9; ++f)
        if (arr[f]) std::memcpy(flat.data() + f * plane, arr[f], sizeof(double) * plane);
    // meta: len[np], then rule_len[np][FOT_CHECK_RULE_LENS] (NULL: every array holds len[i] samples)
    std::vector<int32_t> meta((1 + FOT_CHECK_RULE_LENS) * np);
    std::memcpy(meta.data(), len, sizeof(int32_t) * np);
    for (size_t j = 0; j < FOT_CHECK_RULE_LENS * np; ++j) {
        const int32_t v = rule_len ? rule_len[j] : len[j / FOT_CHECK_RULE_LENS];
        if (v < 0 || v > FOT_MAX_NT) return fail(h, FOT_ERR_INVALID, "rule length out of range");
        meta[np + j] = v;
    }

    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const size_t st_bytes = sizeof(double) * 2 * (size_t)L.n_static, dy_bytes = sizeof(double) * 2 * (size_t)L.dyn_src_points;
    HIP_TRY(h, h->dUserStatic.ensure(std::max<size_t>(st_bytes, 16)));
    HIP_TRY(h, h->dUserDyn.ensure(std::max<size_t>(dy_bytes, 16)));
    HIP_TRY(h, h->dTmpA.ensure(sizeof(InstDesc)));
    HIP_TRY(h, h->dTmpB.ensure(sizeof(double) * flat.size()));
    HIP_TRY(h, h->dTmpC.ensure(sizeof(int32_t) * meta.size()));
    HIP_TRY(h, h->dTmpD.ensure(sizeof(int32_t) * np));
    if (st_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserStatic.p, static_xy, st_bytes, hipMemcpyHostToDevice, st));
    // a pedestrian whose track holds a NaN coordinate anywhere is no obstacle at any step (the reference's pre-filter
    // takes np.min / np.max over the whole track, frenet_planner.py:1211-1219): k_check_ext tests step by step, where an
    // all-NaN track says the same
    std::vector<double> dyn_clean;
    if (dy_bytes && L.desc[0].dyn_mode != FOT_DYN_NONE) {
        const InstDesc &D0 = L.desc[0];
        const size_t row = 2 * (size_t)D0.T;
        for (size_t j = 0; j < (size_t)D0.S * D0.P; ++j) {
            bool bad = false;
            for (size_t e = 0; e < row; ++e) bad |= std::isnan(dyn[j * row + e]);
            if (!bad) continue;
            if (dyn_clean.empty()) dyn_clean.assign(dyn, dyn + 2 * (size_t)L.dyn_src_points);
            for (size_t e = 0; e < row; ++e) dyn_clean[j * row + e] = NAN;
        }
    }
    if (dy_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserDyn.p, dyn_clean.empty() ? dyn : dyn_clean.data(), dy_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpA.p, L.desc.data(), sizeof(InstDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpB.p, flat.data(), sizeof(double) * flat.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpC.p, meta.data(), sizeof(int32_t) * meta.size(), hipMemcpyHostToDevice, st));
    LAUNCH_TRY(h, launch_check_ext(h->dP.as<DevParams>(), h->dTmpA.as<InstDesc>(), n_paths, mode, h->dTmpC.as<int32_t>(),
                                   h->dTmpC.as<int32_t>() + np, h->dTmpB.as<double>(), h->dUserStatic.as<double>(),
                                   h->dUserDyn.as<double>(), h->dTmpD.as<int32_t>(), st, L.max_S > FOT_MAX_SAMPLES ? 1 : 0));
    HIP_TRY(h, hipMemcpyAsync(status_out, h->dTmpD.p, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

}  // namespace

// ---- the helpers fot_host.hpp declares for the other host units

int fot::host::fail(fot_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

int fot::host::hip_fail(fot_handle *h, hipError_t e, const char *what)
{
    return fail(h, FOT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// see fot_handle::order_done
int fot::host::order_begin(fot_handle *h, hipStream_t st)
{
    if (h->order_valid && st != h->order_stream) HIP_TRY(h, hipStreamWaitEvent(st, h->order_done, 0));
    return FOT_OK;
}

int fot::host::order_end(fot_handle *h, hipStream_t st)
{
    HIP_TRY(h, hipEventRecord(h->order_done, st));
    h->order_stream = st;
    h->order_valid = true;
    return FOT_OK;
}

SplineView fot::host::spline_view(const fot_handle *h, int scen)
{
    SplineView v;
    const double *b = h->sc[(size_t)scen].dSpline.as<double>();
    const int n = h->sc[(size_t)scen].spline.n;
    v.s = b; v.ax = b + n; v.bx = b + 2 * n; v.cx = b + 3 * n; v.dx = b + 4 * n;
    v.ay = b + 5 * n; v.by = b + 6 * n; v.cy = b + 7 * n; v.dy = b + 8 * n;
    v.n = n; v._pad = 0;
    return v;
}

// The scenarios a batch's instances name: known ids with a path, chains on one scenario (scen NULL: scenario 0)
int fot::host::check_scenarios(fot_handle *h, const fot_batch &b, const int32_t *scen)
{
    const int n_inst = b.n_inst;
    if (!scen) return h->sc[0].has_path ? FOT_OK : fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    for (int i = 0; i < n_inst; ++i) {
        if (scen[i] < 0 || scen[i] >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
        if (!h->sc[(size_t)scen[i]].has_path)
            return fail(h, FOT_ERR_NO_PATH_SET, "an instance's scenario has no path (fot_set_scenario_path_*)");
    }
    // (build_batch_layout refuses this too, lane by lane; checked here so that a refused call enqueues nothing)
    for (int i = 1; i < n_inst && b.ego; ++i)
        if (b.ego[i].has_prev_s == FOT_PREV_S_CHAINED && scen[i] != scen[i - 1])
            return fail(h, FOT_ERR_INVALID, "a chained instance must be on its predecessor's scenario (a chain is one planner)");
    return FOT_OK;
    return FOT_OK;
}

// Enqueue one plan call behind everything already on `user`; small batches run on `user` itself, large ones
// fork into the lanes' streams and join `user` again.
// sync_caller: the caller waits for the records right behind this call (the synchronous entry points): the selecting
// waves then raise a flag per record in pinned memory (wait_records).
int fot::host::enqueue_plan(fot_handle *h, const fot_batch &b, const int32_t *scen, const void *d_static, const void *d_dyn,
                            fot_result *d_out, hipStream_t user, bool sync_caller, void *d_dyn_stage)
{
    if (b.n_inst < 0) return fail(h, FOT_ERR_INVALID, "n_inst < 0");
    { int r = check_scenarios(h, b, scen); if (r != FOT_OK) return r; }
    h->last_valid = false;
    h->last_eval_forms = 0;
    h->last_flat = 0;
    if (b.n_inst == 0) { h->lanes_used = 0; h->last_valid = true; return FOT_OK; }
    if (!d_out) return fail(h, FOT_ERR_INVALID, "out is NULL");
    if (!b.ego || !b.target_speed) return fail(h, FOT_ERR_INVALID, "ego / target_speed missing");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->prof_on && h->prof_kernel.size() > 16384) { int r = prof_drain(h); if (r != FOT_OK) return r; }
    { int r = order_begin(h, user); if (r != FOT_OK) return r; }

    if (b.n_inst < FOT_SPLIT_MIN_INSTANCES * h->lanes_cfg / 2 || h->lanes_cfg <= 1) {
        h->ws[0].first_inst = 0;
        int rc = enqueue_lane(h, h->ws[0], b, scen, d_static, d_dyn, d_out, user, sync_caller, d_dyn_stage);
        if (rc != FOT_OK) return rc;
        h->lanes_used = 1;
        h->last_valid = true;
        return order_end(h, user);
    }
    HIP_TRY(h, hipEventRecord(h->fork, user));
    int i0 = 0;
    const int lanes = h->lanes_cfg;
    for (int l = 0; l < lanes; ++l) {
        Workspace &w = h->ws[l];
        int n = b.n_inst / lanes + (l < b.n_inst % lanes ? 1 : 0);
        if (l == lanes - 1) n = b.n_inst - i0;
        while (i0 + n < b.n_inst && b.ego[i0 + n].has_prev_s == FOT_PREV_S_CHAINED) ++n;   // never cut a chain
        if (n > b.n_inst - i0) n = b.n_inst - i0;
        if (n <= 0) { w.last = BatchLayout(); w.first_inst = i0; continue; }
        HIP_TRY(h, hipStreamWaitEvent(w.stream, h->fork, 0));
        w.first_inst = i0;
        int rc = enqueue_lane(h, w, sub_batch(b, i0, n), scen ? scen + i0 : nullptr, d_static, d_dyn, d_out + i0, w.stream);
        if (rc != FOT_OK) return rc;
        HIP_TRY(h, hipEventRecord(w.done, w.stream));
        HIP_TRY(h, hipStreamWaitEvent(user, w.done, 0));
        i0 += n;
    }
    h->lanes_used = lanes;
    h->last_valid = true;
    return order_end(h, user);
}

// Arms the record flags for the next synchronous call of n records (false: this call waits on the stream instead).
bool fot::host::arm_records(fot_handle *h, int n)
{
    h->done_seq_armed = false;
    static const bool off = std::getenv("FOT_NO_RECORD_FLAGS") != nullptr;       // diagnostics scripts
    if (off || h->prof_on || n <= 0 || n > 64) return false;
    // only the single-lane path hands the flags to its kernels (the predicate of enqueue_plan): a call the lanes split
    // would raise none, and wait_records would spin out its 20 ms before falling back to the stream
    if (h->lanes_cfg > 1 && n >= FOT_SPLIT_MIN_INSTANCES * h->lanes_cfg / 2) return false;
    if (h->hDone.ensure(sizeof(int32_t) * 64) != hipSuccess) return false;
    if (++h->done_seq == 0) {                                    // (wrapped: no stale flag may equal the new number)
        std::memset(h->hDone.p, 0, sizeof(int32_t) * 64);
        h->done_seq = 1;
    }
    h->done_seq_armed = true;
    return true;
}

// Waits until the n records of the call armed above are in pinned memory; after 20 ms without them (a kernel that
// faulted, a path that raises no flags) the stream is synchronised instead -- never a hang here that the stream
// synchronisation would not have been.
int fot::host::wait_records(fot_handle *h, int n, hipStream_t st)
{
    const bool armed = h->done_seq_armed;
    h->done_seq_armed = false;
    if (armed && spin_words((const int32_t *)h->hDone.p, n, h->done_seq)) return FOT_OK;
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

extern "C" {

const char *fot_version(void) { return "libfot 0.2 (gfx950, float64 lattice)"; }

int32_t fot_abi_info(int32_t cap, int32_t *out)
{
    const int32_t v[FOT_ABI_INFO_WORDS] = {
        FOT_ABI_VERSION,
        (int32_t)sizeof(fot_params), (int32_t)sizeof(fot_ego), (int32_t)sizeof(fot_overrides), (int32_t)sizeof(fot_result),
        (int32_t)sizeof(fot_batch), (int32_t)sizeof(fot_resample_params), (int32_t)sizeof(fot_safety),
        (int32_t)sizeof(fot_loop_frame), (int32_t)sizeof(fot_loop_request), (int32_t)sizeof(fot_wire_header),
        FOT_MAX_NT, FOT_MAX_CIRCLES, FOT_MAX_TI, FOT_MAX_TV, FOT_MAX_BRAKE, FOT_MAX_SAMPLES, FOT_MAX_PRED_LEN,
        FOT_PROFILE_KERNELS, FOT_MARGIN_GROUPS,
        (int32_t)sizeof(fot_loop_config), (int32_t)sizeof(fot_loop_step_out),
        (int32_t)sizeof(fot_loop_replay), (int32_t)sizeof(fot_loop_run_out), (int32_t)sizeof(fot_loop_summary),
        (int32_t)sizeof(fot_pred_origin), (int32_t)sizeof(fot_pred_score),
        (int32_t)sizeof(fot_sgan_desc), FOT_SGAN_MAX_EMBEDDING, FOT_SGAN_MAX_HIDDEN, FOT_SGAN_MAX_MLP, FOT_SGAN_MAX_BOTTLENECK,
        FOT_SGAN_MAX_OBS_LEN, FOT_SGAN_MAX_PEDS, FOT_SGAN_POOL_HIDDEN,
    };
    for (int i = 0; i < FOT_ABI_INFO_WORDS && i < cap && out; ++i) out[i] = v[i];
    return FOT_ABI_INFO_WORDS;
}

const char *fot_last_error(const fot_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int fot_create(const fot_params *params, int device, fot_handle **out)
{
    if (!params || !out) return fail(nullptr, FOT_ERR_INVALID, "params/out is NULL");
    *out = nullptr;
    DevParams P;
    std::string err;
    int rc = build_dev_params(*params, P, err);
    if (rc != FOT_OK) return fail(nullptr, rc, err);
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, FOT_ERR_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0) { e = hipGetDevice(&device); if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDevice"); }
    if (device >= n_dev) return fail(nullptr, FOT_ERR_INVALID, "device index out of range");
    fot_handle *h = new (std::nothrow) fot_handle();
    if (!h) return fail(nullptr, FOT_ERR_HIP, "out of host memory");
    h->device = device;
    if (const char *ev = std::getenv("FOT_LANES")) {             // tuning knob: 1 disables the split
        const int v = std::atoi(ev);
        if (v >= 1 && v <= FOT_LANES) h->lanes_cfg = v;
    }
    h->sc.reserve(FOT_MAX_SCENARIOS);
    h->sc.emplace_back();
    h->sc[0].params = *params;
    h->sc[0].P = P;
    auto bail = [&](hipError_t ee, const char *what) {
        int r = hip_fail(nullptr, ee, what);
        destroy_handle(h);
        return r;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    if ((e = hipEventCreateWithFlags(&h->fork, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&h->order_done, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    for (int l = 0; l < FOT_LANES; ++l) {
        Workspace &w = h->ws[l];
        // lane streams only when the handle splits batches; lane 0 of a single-lane handle runs on the caller's stream
        if (h->lanes_cfg > 1 && l < h->lanes_cfg &&
            (e = hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
        if (l >= h->lanes_cfg) continue;
        for (int i = 0; i < 2; ++i)
            if ((e = hipEventCreateWithFlags(&w.staging_done[i], hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&w.done, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    }
    if ((e = h->dP.ensure(sizeof(DevParams))) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemcpy(h->dP.p, &h->sc[0].P, sizeof(DevParams), hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy");
    if (upload_spline_table(h) != FOT_OK) { std::string m = h->err; destroy_handle(h); return fail(nullptr, FOT_ERR_HIP, m); }
    {
        int cut = TILE_CUT_AUTO;                                 // FOT_TILE_CUT=wave|group: diagnostics scripts
        if (const char *ev = std::getenv("FOT_TILE_CUT")) cut = ev[0] == 'g' ? TILE_CUT_GROUP : ev[0] == 'w' ? TILE_CUT_WAVE : TILE_CUT_AUTO;
        if (upload_tile_shapes(h, cut) != FOT_OK) { std::string m = h->err; destroy_handle(h); return fail(nullptr, FOT_ERR_HIP, m); }
    }
    { std::lock_guard<std::mutex> lk(g_live_mu); live_handles().insert(h); }
    *out = h;
    return FOT_OK;
}

int32_t fot_live_handles(void)
{
    std::lock_guard<std::mutex> lk(g_live_mu);
    return (int32_t)live_handles().size();
}

void fot_destroy(fot_handle *h)
{
    if (!h) return;
    {   // idempotent: only a handle fot_create handed out and nobody has destroyed yet (the pointer is not even read else)
        std::lock_guard<std::mutex> lk(g_live_mu);
        auto &live = live_handles();
        auto it = live.find(h);
        if (it == live.end()) return;
        live.erase(it);
    }
    destroy_handle(h);
}

int fot_set_scenario_path_waypoints(fot_handle *h, int32_t id, int32_t n, const double *wx, const double *wy)
{
    if (!h) return FOT_ERR_INVALID;
    if (id < 0 || id >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
    std::string err;
    HostSpline sp;
    int rc = build_spline(n, wx, wy, sp, err);
    if (rc != FOT_OK) return fail(h, rc, err);
    h->sc[(size_t)id].spline = sp;
    return upload_spline(h, id);
}

int fot_set_path_waypoints(fot_handle *h, int32_t n, const double *wx, const double *wy)
{
    return fot_set_scenario_path_waypoints(h, 0, n, wx, wy);
}

int fot_set_scenario_path_coeffs(fot_handle *h, int32_t id, int32_t n, const double *s,
                                 const double *ax, const double *bx, const double *cx, const double *dx,
                                 const double *ay, const double *by, const double *cy, const double *dy)
{
    if (!h) return FOT_ERR_INVALID;
    if (id < 0 || id >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
    if (n < 2 || !s || !ax || !bx || !cx || !dx || !ay || !by || !cy || !dy)
        return fail(h, FOT_ERR_INVALID, "spline needs >= 2 knots and all nine coefficient arrays");
    HostSpline &sp = h->sc[(size_t)id].spline;
    sp.n = n;
    sp.s.assign(s, s + n);
    sp.ax.assign(ax, ax + n); sp.bx.assign(bx, bx + n - 1); sp.cx.assign(cx, cx + n); sp.dx.assign(dx, dx + n - 1);
    sp.ay.assign(ay, ay + n); sp.by.assign(by, by + n - 1); sp.cy.assign(cy, cy + n); sp.dy.assign(dy, dy + n - 1);
    sp.bx.resize(n, 0.0); sp.dx.resize(n, 0.0); sp.by.resize(n, 0.0); sp.dy.resize(n, 0.0);
    return upload_spline(h, id);
}

int fot_set_path_coeffs(fot_handle *h, int32_t n, const double *s,
                        const double *ax, const double *bx, const double *cx, const double *dx,
                        const double *ay, const double *by, const double *cy, const double *dy)
{
    return fot_set_scenario_path_coeffs(h, 0, n, s, ax, bx, cx, dx, ay, by, cy, dy);
}

int fot_add_scenario(fot_handle *h, const fot_params *params, int32_t *id_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (!params || !id_out) return fail(h, FOT_ERR_INVALID, "params / id_out is NULL");
    const fot_params &p0 = h->sc[0].params;
    if (!(params->dt == p0.dt) || !(params->max_t == p0.max_t))
        return fail(h, FOT_ERR_INVALID, "a scenario has the handle's dt and max_t (one time grid per handle)");
    DevParams P;
    std::string err;
    int rc = build_dev_params(*params, P, err);
    if (rc != FOT_OK) return fail(h, rc, err);
    if ((int)h->sc.size() >= FOT_MAX_SCENARIOS) return fail(h, FOT_ERR_UNSUPPORTED, "more than FOT_MAX_SCENARIOS scenarios");
    h->sc.emplace_back();
    Scenario &S = h->sc.back();
    S.params = *params;
    S.P = P;
    rc = upload_params(h);
    if (rc == FOT_OK) rc = upload_spline_table(h);
    if (rc == FOT_OK) rc = upload_tile_shapes(h, h->tile_cut);
    if (rc != FOT_OK) {                                          // (a HIP failure: back to the scenarios before the call)
        h->sc.pop_back();
        (void)upload_params(h); (void)upload_spline_table(h); (void)upload_tile_shapes(h, h->tile_cut);
        return rc;
    }
    *id_out = (int32_t)h->sc.size() - 1;
    return FOT_OK;
}

int fot_get_path_coeffs(const fot_handle *h, int32_t *n_out, double *s,
                        double *ax, double *bx, double *cx, double *dx,
                        double *ay, double *by, double *cy, double *dy)
{
    return fot_get_scenario_path_coeffs(h, 0, n_out, s, ax, bx, cx, dx, ay, by, cy, dy);
}

int fot_get_scenario_path_coeffs(const fot_handle *h, int32_t id, int32_t *n_out, double *s,
                                 double *ax, double *bx, double *cx, double *dx,
                                 double *ay, double *by, double *cy, double *dy)
{
    if (!h) return FOT_ERR_NO_PATH_SET;
    if (id < 0 || id >= (int)h->sc.size()) return FOT_ERR_INVALID;
    if (!h->sc[(size_t)id].has_path) return FOT_ERR_NO_PATH_SET;
    const HostSpline &sp = h->sc[(size_t)id].spline;
    const int n = sp.n;
    if (n_out) *n_out = n;
    auto cp = [](double *dst, const std::vector<double> &src, int cnt) {
        if (dst) std::memcpy(dst, src.data(), sizeof(double) * (size_t)cnt);
    };
    cp(s, sp.s, n);
    cp(ax, sp.ax, n); cp(bx, sp.bx, n - 1); cp(cx, sp.cx, n); cp(dx, sp.dx, n - 1);
    cp(ay, sp.ay, n); cp(by, sp.by, n - 1); cp(cy, sp.cy, n); cp(dy, sp.dy, n - 1);
    return FOT_OK;
}

int fot_spline_eval(fot_handle *h, int32_t n, const double *s, double *x, double *y,
                    double *yaw, double *kappa, double *dkappa)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    if (n <= 0) return FOT_OK;
    if (!s) return fail(h, FOT_ERR_INVALID, "s is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    { int r = order_begin(h, h->stream); if (r != FOT_OK) return r; }
    HIP_TRY(h, h->dTmpA.ensure(sizeof(double) * (size_t)n));
    HIP_TRY(h, h->dTmpB.ensure(sizeof(double) * 5 * (size_t)n));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpA.p, s, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    LAUNCH_TRY(h, launch_spline_eval(spline_view(h, 0), n, h->dTmpA.as<double>(), h->dTmpB.as<double>(), h->stream));
    std::vector<double> outv((size_t)5 * n);
    HIP_TRY(h, hipMemcpyAsync(outv.data(), h->dTmpB.p, sizeof(double) * 5 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double *dst[5] = { x, y, yaw, kappa, dkappa };
    for (int f = 0; f < 5; ++f)
        if (dst[f]) std::memcpy(dst[f], outv.data() + (size_t)f * n, sizeof(double) * (size_t)n);
    return FOT_OK;
}

int fot_profile_enable(fot_handle *h, int on)
{
    if (!h) return FOT_ERR_INVALID;
    if (!on && h->prof_on) { int r = prof_drain(h); if (r != FOT_OK) return r; }
    h->prof_on = on != 0;
    return FOT_OK;
}

int fot_profile_read(fot_handle *h, int reset, int32_t cap, int32_t *launches, double *total_ms)
{
    if (!h) return FOT_ERR_INVALID;
    if (cap < 0) return fail(h, FOT_ERR_INVALID, "fot_profile_read: cap < 0");
    HIP_TRY(h, hipSetDevice(h->device));
    int r = prof_drain(h);
    if (r != FOT_OK) return r;
    for (int k = 0; k < FOT_PROFILE_KERNELS; ++k) {
        if (k < cap) {                                           // (never past the caller's arrays, whatever header it was built with)
            if (launches) launches[k] = h->prof_launches[k];
            if (total_ms) total_ms[k] = h->prof_ms[k];
        }
        if (reset) { h->prof_launches[k] = 0; h->prof_ms[k] = 0.0; }
    }
    return FOT_PROFILE_KERNELS;
}

const char *fot_profile_kernel_name(int index)
{
    return index >= 0 && index < FOT_PROFILE_KERNELS ? kKernelNames[index] : "";
}

int fot_synchronize(fot_handle *h)
{
    if (!h) return FOT_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FOT_OK;
}

int fot_plan_batch_scenarios_device(fot_handle *h, const fot_batch *batch, const int32_t *scenario, fot_result *out_dev,
                                    void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (!batch) return fail(h, FOT_ERR_INVALID, "batch is NULL");
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return enqueue_plan(h, *batch, scenario, batch->static_xy, batch->dyn_xy, out_dev, st);
}

int fot_plan_batch_device(fot_handle *h, const fot_batch *batch, fot_result *out_dev, void *stream)
{
    return fot_plan_batch_scenarios_device(h, batch, nullptr, out_dev, stream);
}

int fot_plan_batch(fot_handle *h, const fot_batch *batch, fot_result *out)
{
    return fot_plan_batch_scenarios(h, batch, nullptr, out);
}

int fot_plan_batch_scenarios(fot_handle *h, const fot_batch *batch, const int32_t *scenario, fot_result *out)
{
    if (!h) return FOT_ERR_INVALID;
    if (!batch) return fail(h, FOT_ERR_INVALID, "batch is NULL");
    if (batch->n_inst > 0 && !out) return fail(h, FOT_ERR_INVALID, "out is NULL");
    if (batch->n_inst <= 0) return batch->n_inst == 0 ? FOT_OK : fail(h, FOT_ERR_INVALID, "n_inst < 0");
    { int r = check_scenarios(h, *batch, scenario); if (r != FOT_OK) return r; }
    // extents of the caller's obstacle arrays
    BatchLayout probe;
    std::string err;
    int rc = build_batch_layout(h->refs.data(), (int)h->refs.size(), scenario, *batch, probe, err, h->sample_cap);
    if (rc != FOT_OK) return fail(h, rc, err);
    const size_t elem = batch->obstacle_dtype == FOT_F32 ? sizeof(float) : sizeof(double);
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t st_bytes = (size_t)probe.n_static * 2 * elem, dy_bytes = (size_t)probe.dyn_src_points * 2 * elem;
    const size_t out_bytes = sizeof(fot_result) * (size_t)batch->n_inst;
    // A plan step for one or a few egos is latency, not bandwidth: its obstacle points and its records (written once,
    // by the selecting wave) then travel straight between the kernels and pinned host memory -- two copy operations and
    // their synchronisation less per call.  The dynamic tensors cross the bus ONCE: the NaN-scan blocks of the first
    // launch read them out of the pinned block and leave a copy in HBM for k_cull (NanScan::stage); the few static points
    // are read in place.  Up to the 2 MiB below that beats a staging copy plus its wait (scripts/size_sweep.py), beyond
    // it the tensors are staged in HBM with copy operations.
    if (st_bytes + dy_bytes <= 2 * SMALL_CALL_BYTES && out_bytes <= 8 * SMALL_CALL_BYTES) {   // (records stream out as instances finish)
        const size_t dy_off = align256(st_bytes);
        HIP_TRY(h, h->hSmallIn.ensure(dy_off + dy_bytes + 256));
        HIP_TRY(h, h->hRecOut.ensure(out_bytes));
        char *in = (char *)h->hSmallIn.p;
        if (st_bytes) std::memcpy(in, batch->static_xy, st_bytes);
        if (dy_bytes) std::memcpy(in + dy_off, batch->dyn_xy, dy_bytes);
        // the dynamic tensors cross PCIe once: the scan blocks of the first launch leave a copy in HBM for the others
        static const bool no_stage = std::getenv("FOT_NO_SCAN_STAGE") != nullptr;        // diagnostics scripts
        void *stage = nullptr;
        if (dy_bytes && !no_stage) { HIP_TRY(h, h->dUserDyn.ensure(dy_bytes + 256)); stage = h->dUserDyn.p; }
        arm_records(h, batch->n_inst);
        rc = enqueue_plan(h, *batch, scenario, in, in + dy_off, (fot_result *)h->hRecOut.p, h->stream, true, stage);
        if (rc != FOT_OK) { h->done_seq_armed = false; return rc; }
        rc = wait_records(h, batch->n_inst, h->stream);
        if (rc != FOT_OK) return rc;
        // what the device wrote of each record: the header and the first n_total entries of the 15 path arrays (a fifth of
        // the record at 51 samples -- the whole-record copy cost a one-ego call 2 us); the caller's entries past n_total stay
        // as they are
        const size_t head = offsetof(fot_result, t), used = sizeof(double) * (size_t)h->sc[0].P.n_total;
        for (int i = 0; i < batch->n_inst; ++i) {
            const fot_result *src = (const fot_result *)h->hRecOut.p + i;
            std::memcpy(&out[i], src, head);
            for (int f = 0; f < 15; ++f) std::memcpy(out[i].t + (size_t)f * FOT_MAX_NT, src->t + (size_t)f * FOT_MAX_NT, used);
        }
        return FOT_OK;
    }
    HIP_TRY(h, h->dUserStatic.ensure(std::max<size_t>(st_bytes, 16)));
    HIP_TRY(h, h->dUserDyn.ensure(std::max<size_t>(dy_bytes, 16)));
    HIP_TRY(h, h->dOut.ensure_zeroed(sizeof(fot_result) * (size_t)batch->n_inst));
    if (st_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserStatic.p, batch->static_xy, st_bytes, hipMemcpyHostToDevice, h->stream));
    if (dy_bytes) HIP_TRY(h, hipMemcpyAsync(h->dUserDyn.p, batch->dyn_xy, dy_bytes, hipMemcpyHostToDevice, h->stream));
    rc = enqueue_plan(h, *batch, scenario, h->dUserStatic.p, h->dUserDyn.p, h->dOut.as<fot_result>(), h->stream);
    if (rc != FOT_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, h->dOut.p, sizeof(fot_result) * (size_t)batch->n_inst, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FOT_OK;
}

int fot_frenet_state_batch(fot_handle *h, int32_t n, const fot_ego *ego,
                           double *frenet, double *ref, double *new_prev_s, int32_t *ok)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    if (n <= 0) return FOT_OK;
    if (!ego) return fail(h, FOT_ERR_INVALID, "ego is NULL");
    std::vector<InstDesc> desc((size_t)n);
    for (int i = 0; i < n; ++i) { desc[i] = InstDesc(); desc[i].ego = ego[i]; }
    for (int i = n - 1, run = 0; i >= 0; --i) {                 // chain lengths, as build_batch_layout sets them
        desc[i].n_chained = run;
        run = desc[i].ego.has_prev_s == FOT_PREV_S_CHAINED ? run + 1 : 0;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    { int r = order_begin(h, h->stream); if (r != FOT_OK) return r; }
    if (sizeof(InstDesc) * (size_t)n <= SMALL_CALL_BYTES) {      // small call: straight from / into pinned host memory
        HIP_TRY(h, h->hSmallIn.ensure(sizeof(InstDesc) * (size_t)n));
        HIP_TRY(h, h->hSmallOut.ensure(sizeof(InstState) * (size_t)n));
        std::memcpy(h->hSmallIn.p, desc.data(), sizeof(InstDesc) * (size_t)n);
        LAUNCH_TRY(h, launch_frenet_state(h->dP.as<DevParams>(), PathSet::single(spline_view(h, 0)), (const InstDesc *)h->hSmallIn.p,
                                          (InstState *)h->hSmallOut.p, n, MetaImport(), NanScan(), nullptr, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const InstState *stp = (const InstState *)h->hSmallOut.p;
        for (int i = 0; i < n; ++i) {
            if (frenet) std::memcpy(frenet + 6 * (size_t)i, stp[i].frenet0, sizeof(double) * 6);
            if (ref) std::memcpy(ref + 6 * (size_t)i, stp[i].ref0, sizeof(double) * 6);
            if (new_prev_s) new_prev_s[i] = stp[i].new_prev_s;
            if (ok) ok[i] = stp[i].c2f_ok;
        }
        return FOT_OK;
    }
    HIP_TRY(h, h->dTmpA.ensure(sizeof(InstDesc) * (size_t)n));
    HIP_TRY(h, h->dTmpB.ensure(sizeof(InstState) * (size_t)n));
    HIP_TRY(h, hipMemcpyAsync(h->dTmpA.p, desc.data(), sizeof(InstDesc) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    LAUNCH_TRY(h, launch_frenet_state(h->dP.as<DevParams>(), PathSet::single(spline_view(h, 0)), h->dTmpA.as<InstDesc>(),
                                      h->dTmpB.as<InstState>(), n, MetaImport(), NanScan(), nullptr, h->stream));
    std::vector<InstState> st((size_t)n);
    HIP_TRY(h, hipMemcpyAsync(st.data(), h->dTmpB.p, sizeof(InstState) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
        if (frenet) std::memcpy(frenet + 6 * (size_t)i, st[i].frenet0, sizeof(double) * 6);
        if (ref) std::memcpy(ref + 6 * (size_t)i, st[i].ref0, sizeof(double) * 6);
        if (new_prev_s) new_prev_s[i] = st[i].new_prev_s;
        if (ok) ok[i] = st[i].c2f_ok;
    }
    return FOT_OK;
}

int fot_gather_paths(const fot_result *records, int32_t n, const int32_t *index, int32_t kmax, double *out)
{
    if (n < 0 || kmax < 0 || kmax > FOT_MAX_NT) return FOT_ERR_INVALID;
    if (n == 0 || kmax == 0) return FOT_OK;
    if (!records || !index || !out) return FOT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        if (index[i] < 0) return FOT_ERR_INVALID;
        const double *src = records[index[i]].t;                 // the 15 arrays lie back to back (static_assert below)
        for (int f = 0; f < 15; ++f)
            std::memcpy(out + ((size_t)f * n + i) * kmax, src + (size_t)f * FOT_MAX_NT, sizeof(double) * (size_t)kmax);
    }
    return FOT_OK;
}

int fot_debug_candidates(fot_handle *h, int32_t inst, int32_t cap, double *cost,
                         int32_t *status, int32_t *keep, int32_t *n_t)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->last_valid) return fail(h, FOT_ERR_INVALID, "no completed plan call on this handle");
    int local = 0;
    Workspace *w = lane_of(h, inst, &local);
    if (!w) return fail(h, FOT_ERR_INVALID, "instance index out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // diagnostic entry: whatever stream the plan ran on
    const InstDesc &D = w->last.desc[local];
    InstState S;
    HIP_TRY(h, hipMemcpy(&S, w->dState.as<InstState>() + local, sizeof(InstState), hipMemcpyDeviceToHost));
    const int n = S.n_cand;
    const int m = n < cap ? n : cap;
    if (m <= 0) return n;
    std::vector<uint8_t> st8((size_t)m);
    std::vector<uint16_t> kp16((size_t)m);
    if (cost) HIP_TRY(h, hipMemcpy(cost, w->dCost.as<double>() + D.cand_off, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(st8.data(), w->dStatus.as<uint8_t>() + D.cand_off, (size_t)m, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(kp16.data(), w->dKeep.as<uint16_t>() + D.cand_off, sizeof(uint16_t) * (size_t)m, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; ++i) {
        if (status) status[i] = st8[i];
        if (keep) keep[i] = kp16[i];
        if (n_t) {                                               // (on the instance's own scenario)
            const DevParams &P = h->sc[(size_t)D.scen].P;
            if (i < D.n_grid) n_t[i] = P.ti[i / (D.n_tv * P.n_di)].n_t;
            else n_t[i] = P.n_total;
        }
    }
    return n;
}

int fot_debug_candidate_path(fot_handle *h, int32_t inst, int32_t index, double *arrays, int32_t *n_t)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->last_valid) return fail(h, FOT_ERR_INVALID, "no completed plan call on this handle");
    int local = 0;
    Workspace *w = lane_of(h, inst, &local);
    if (!w) return fail(h, FOT_ERR_INVALID, "instance index out of range");
    if (!arrays) return fail(h, FOT_ERR_INVALID, "arrays is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, h->dTmpA.ensure(sizeof(double) * 15 * FOT_MAX_NT));
    HIP_TRY(h, h->dTmpD.ensure(sizeof(int32_t) * 2));
    HIP_TRY(h, hipMemsetAsync(h->dTmpA.p, 0, sizeof(double) * 15 * FOT_MAX_NT, h->stream));
    const int scen = w->last.desc[(size_t)local].scen;          // the instance's own scenario
    LAUNCH_TRY(h, launch_debug_path(h->dP.as<DevParams>() + scen, (const InstDesc *)w->dMeta.p, w->dState.as<InstState>(),
                                    spline_view(h, scen), local, index,
                                    h->dTmpA.as<double>(), h->dTmpD.as<int32_t>(), h->stream));
    int32_t meta[2] = { 0, 0 };
    HIP_TRY(h, hipMemcpyAsync(arrays, h->dTmpA.p, sizeof(double) * 15 * FOT_MAX_NT, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(meta, h->dTmpD.p, sizeof(meta), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!meta[1]) return fail(h, FOT_ERR_INVALID, "candidate index out of range");
    if (n_t) *n_t = meta[0];
    return FOT_OK;
}

int32_t fot_wire_n_total(const fot_handle *h) { return h ? h->sc[0].P.n_total : FOT_ERR_INVALID; }

int32_t fot_wire_record_bytes(int32_t n_total)
{
    if (n_total < 1 || n_total > FOT_MAX_NT) return FOT_ERR_INVALID;
    return (int32_t)align256(sizeof(fot_wire_header) + sizeof(float) * 15 * (size_t)n_total);
}

int fot_pack_records_device(fot_handle *h, int32_t n, const fot_result *records_dev, void *wire_dev, void *stream)
{
    if (!h) return FOT_ERR_INVALID;
    if (n <= 0) return n == 0 ? FOT_OK : fail(h, FOT_ERR_INVALID, "n < 0");
    if (!records_dev || !wire_dev) return fail(h, FOT_ERR_INVALID, "NULL buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // ordered behind the handle's previous enqueue whatever stream that ran on: the records are usually the output of
    // the plan call just made, and NULL (= the handle's own stream) is also torch's default-stream handle
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    LAUNCH_TRY(h, launch_pack_wire(n, h->sc[0].P.n_total, fot_wire_record_bytes(h->sc[0].P.n_total), records_dev,
                                   (unsigned char *)wire_dev, st));
    return order_end(h, st);
}

static_assert(offsetof(fot_result, s) - offsetof(fot_result, t) == sizeof(double) * FOT_MAX_NT &&
              offsetof(fot_result, c) - offsetof(fot_result, t) == sizeof(double) * FOT_MAX_NT * 14,
              "the 15 path arrays of fot_result are contiguous");

int fot_pack_records_host(int32_t n_total, int32_t n, const fot_result *records, void *wire)
{
    const int32_t stride = fot_wire_record_bytes(n_total);
    if (stride < 0 || n < 0 || (n > 0 && (!records || !wire))) return FOT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const fot_result &R = records[i];
        unsigned char *w = (unsigned char *)wire + (size_t)i * stride;
        std::memset(w, 0, (size_t)stride);
        fot_wire_header H;
        std::memset(&H, 0, sizeof(H));
        H.status = R.status; H.best_index = R.best_index; H.n_cand = R.n_cand; H.n_keep = R.n_keep;
        H.cost = R.cost; H.stats_valid = R.stats_valid; H.n_total = n_total;
        H.new_last_kappa = R.new_last_kappa; H.new_prev_s = R.new_prev_s;
        std::memcpy(H.stats, R.stats, sizeof(H.stats));
        std::memcpy(H.frenet0, R.frenet0, sizeof(H.frenet0));
        std::memcpy(H.ref0, R.ref0, sizeof(H.ref0));
        std::memcpy(w, &H, sizeof(H));
        float *path = (float *)(w + sizeof(H));
        const double *arr = R.t;
        for (int f = 0; f < 15; ++f) {                           // (k_pack_wire: offsets for s, x, y; zeros past n_keep)
            const double base = f == 1 ? R.frenet0[0] : f == 9 ? R.ref0[1] : f == 10 ? R.ref0[2] : 0.0;
            for (int k = 0; k < n_total; ++k)
                path[f * n_total + k] = k < R.n_keep ? (float)(arr[f * FOT_MAX_NT + k] - base) : 0.0f;
        }
    }
    return FOT_OK;
}

int fot_unpack_records(int32_t n_total, int32_t n, const void *wire, fot_result *records)
{
    const int32_t stride = fot_wire_record_bytes(n_total);
    if (stride < 0 || n < 0 || (n > 0 && (!records || !wire))) return FOT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const unsigned char *w = (const unsigned char *)wire + (size_t)i * stride;
        fot_wire_header H;
        std::memcpy(&H, w, sizeof(H));
        if (H.n_total != n_total) return FOT_ERR_INVALID;
        if (H.n_keep < 0 || H.n_keep > n_total || H.n_cand < 0 || H.best_index < -1 || H.best_index >= (H.n_cand > 0 ? H.n_cand : 1))
            return FOT_ERR_INVALID;                              // (a corrupt or foreign record)
        fot_result &R = records[i];
        std::memset(&R, 0, sizeof(R));
        R.status = H.status; R.best_index = H.best_index; R.n_cand = H.n_cand; R.n_keep = H.n_keep;
        R.cost = H.cost; R.stats_valid = H.stats_valid;
        R.new_last_kappa = H.new_last_kappa; R.new_prev_s = H.new_prev_s;
        std::memcpy(R.stats, H.stats, sizeof(H.stats));
        std::memcpy(R.frenet0, H.frenet0, sizeof(H.frenet0));
        std::memcpy(R.ref0, H.ref0, sizeof(H.ref0));
        const float *path = (const float *)(w + sizeof(H));
        double *arr = R.t;
        const int keep = H.n_keep < n_total ? H.n_keep : n_total;
        for (int f = 0; f < 15; ++f) {
            const double base = f == 1 ? R.frenet0[0] : f == 9 ? R.ref0[1] : f == 10 ? R.ref0[2] : 0.0;
            for (int k = 0; k < keep; ++k) arr[f * FOT_MAX_NT + k] = base + (double)path[f * n_total + k];
        }
    }
    return FOT_OK;
}

int fot_debug_set_eval_segments(fot_handle *h, int32_t n_seg)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_seg < 0 || n_seg > 4) return fail(h, FOT_ERR_INVALID, "fot_debug_set_eval_segments: 0 (automatic) .. 4");
    h->eval_segments = n_seg;
    return FOT_OK;
}

int fot_debug_set_tile_cut(fot_handle *h, int32_t cut)
{
    if (!h) return FOT_ERR_INVALID;
    if (cut != TILE_CUT_AUTO && cut != TILE_CUT_WAVE && cut != TILE_CUT_GROUP)
        return fail(h, FOT_ERR_INVALID, "fot_debug_set_tile_cut: 0 (automatic), 1 (per-wave rows), 2 (groups)");
    if (cut == h->tile_cut) return FOT_OK;
    return upload_tile_shapes(h, cut);
}

int fot_debug_set_eval_form(fot_handle *h, int32_t form)
{
    if (!h) return FOT_ERR_INVALID;
    if (form < -1 || form > 1)
        return fail(h, FOT_ERR_INVALID, "fot_debug_set_eval_form: 0 (by eligibility), 1 (general form), -1 (query only)");
    if (form >= 0) h->eval_form = form;
    return h->last_eval_forms;
}

int fot_set_sample_capacity(fot_handle *h, int32_t n_samples)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_samples < FOT_MAX_SAMPLES || n_samples > FOT_MAX_PLAN_SAMPLES)
        return fail(h, FOT_ERR_INVALID, "fot_set_sample_capacity: FOT_MAX_SAMPLES (64) .. FOT_MAX_PLAN_SAMPLES (254) samples");
    // a loop that is set up with more samples keeps its capacity: the predictor of a resident loop (sampler or recording),
    // and the distribution of a stepwise loop's current frame, whose later requests still plan against it
    const LoopState &L = h->loop;
    const int loop_S = std::max(L.replay.set ? L.replay.dist_S() : 0, L.have_frame ? L.dist_S : 0);
    if (n_samples < loop_S)
        return fail(h, FOT_ERR_INVALID, "fot_set_sample_capacity: the handle's loop is set up with " + std::to_string(loop_S) +
                                        " samples (a capacity below them: after fot_loop_begin* / fot_loop_set_replay anew)");
    h->sample_cap = n_samples;
    return FOT_OK;
}

int32_t fot_max_plan_samples(void) { return FOT_MAX_PLAN_SAMPLES; }

int fot_get_sample_capacity(const fot_handle *h, int32_t *out)
{
    if (!h || !out) return FOT_ERR_INVALID;
    *out = h->sample_cap;
    return FOT_OK;
}

int fot_debug_set_flat(fot_handle *h, int32_t on)
{
    if (!h) return FOT_ERR_INVALID;
    if (on < -1 || on > 1)
        return fail(h, FOT_ERR_INVALID, "fot_debug_set_flat: 0 (never), 1 (by eligibility), -1 (query only)");
    if (on >= 0) h->flat_mode = on;
    return h->last_flat;
}

int fot_debug_time_info(const fot_handle *h, double time, int32_t *n_t, double *quartic_inv4, double *quintic_inv9)
{
    if (!h || !(time > 0.0)) return FOT_ERR_INVALID;
    TimeInfo ti;
    if (!time_info(time, h->sc[0].params.dt, ti)) return FOT_ERR_UNSUPPORTED;      // more than FOT_MAX_NT samples
    if (n_t) *n_t = ti.n_t;
    if (quartic_inv4) std::memcpy(quartic_inv4, ti.qa, sizeof(ti.qa));
    if (quintic_inv9) std::memcpy(quintic_inv9, ti.qi, sizeof(ti.qi));
    return FOT_OK;
}

int fot_debug_margins(fot_handle *h, int32_t inst, int32_t cap, double *margins)
{
    if (!h) return FOT_ERR_INVALID;
    if (!h->last_valid) return fail(h, FOT_ERR_INVALID, "no completed plan call on this handle");
    int local = 0;
    Workspace *w = lane_of(h, inst, &local);
    if (!w) return fail(h, FOT_ERR_INVALID, "instance index out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());                          // diagnostic entry: whatever stream the plan ran on
    InstState S;
    HIP_TRY(h, hipMemcpy(&S, w->dState.as<InstState>() + local, sizeof(InstState), hipMemcpyDeviceToHost));
    const int n = S.n_cand;
    const int m = n < cap ? n : cap;
    if (m <= 0 || !margins) return n;
    const size_t bytes = sizeof(double) * FOT_MARGIN_GROUPS * (size_t)m;
    HIP_TRY(h, h->dTmpB.ensure(bytes));
    EntryArrays ea;
    ea.cnt = w->dEntCnt.as<int32_t>(); ea.e32 = w->dEnt32.as<f2>(); ea.e64 = w->dEnt64.as<d2>();
    ea.sid = w->dEntSid.as<uint8_t>(); ea.rng = w->dWaveRng.as<TileStep>();
    const int scen = w->last.desc[(size_t)local].scen;          // the instance's own scenario
    LAUNCH_TRY(h, launch_debug_margins(h->dP.as<DevParams>() + scen, (const InstDesc *)w->dMeta.p, w->dState.as<InstState>(),
                                       spline_view(h, scen), local, ea, m, h->dTmpB.as<double>(), h->stream));
    HIP_TRY(h, hipMemcpyAsync(margins, h->dTmpB.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return n;
}

int fot_check_collision_paths(fot_handle *h, int32_t n_paths, const int32_t *len,
                              const double *x, const double *y, const double *yaw, const double *t,
                              int32_t n_static, const double *static_xy,
                              int32_t mode, int32_t S, int32_t Pn, int32_t T, const double *dyn,
                              int32_t *free_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_paths > 0 && (!x || !y || !t)) return fail(h, FOT_ERR_INVALID, "NULL path array");
    if (n_paths > 0 && h->sc[0].P.has_footprint && !yaw)
        return fail(h, FOT_ERR_INVALID, "yaw is required with a multi-circle footprint");
    const double *arr[9] = { x, y, yaw, nullptr, nullptr, nullptr, nullptr, nullptr, t };
    return check_ext(h, 0, n_paths, len, nullptr, arr, nullptr, NAN, n_static, static_xy, mode, S, Pn, T, dyn, free_out);
}

int fot_check_paths(fot_handle *h, int32_t n_paths, const int32_t *len, const int32_t *rule_len,
                    const double *x, const double *y, const double *yaw, const double *v, const double *a,
                    const double *c, const double *d, const double *s, const double *t,
                    const fot_overrides *overrides, double max_stop_distance,
                    int32_t n_static, const double *static_xy,
                    int32_t mode, int32_t S, int32_t Pn, int32_t T, const double *dyn, int32_t *status_out)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_paths > 0 && (!x || !y || !v || !a || !c || !t)) return fail(h, FOT_ERR_INVALID, "NULL path array");
    const double *arr[9] = { x, y, yaw, v, a, c, d, s, t };
    return check_ext(h, 1, n_paths, len, rule_len, arr, overrides, max_stop_distance, n_static, static_xy, mode, S, Pn, T,
                     dyn, status_out);
}

}  // extern "C"
