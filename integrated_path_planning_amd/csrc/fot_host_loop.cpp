// fot_host_loop.cpp -- the closed loop of libfot.so, everything that reads or writes fot_handle::loop: the stepwise loop
// (fot_loop_plan / _observe / _step with the fail-safe state machine) and the resident one (fot_loop_set_replay /
// fot_loop_run with its summaries, scores, sampler, recorded samples and representative sample).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fot_host.hpp"
#include "fot_kernels.h"         // launch_frenet_state: the goal test's nearest point (observe_begin_impl)
#include "fot_loop_kernels.h"
#include "fot_sgan.h"            // launch_sgan_window, launch_sgan_noise: the resident sampler's window and noise

namespace {

// A scenario loop's static points: every scenario's set once in HBM (rebuilt after fot_loop_set_scenario_static), and
// room for the per-request blocks of n_req requests.  Synchronises only when something has to be uploaded or to grow.
int ensure_scen_static(fot_handle *h, int n_req, hipStream_t st)
{
    LoopState &L = h->loop;
    const size_t n_sc = h->sc.size();
    if (L.scen_static_dirty || L.scen_static_off.size() != n_sc + 1) {
        L.scen_static.resize(n_sc);
        std::vector<int32_t> off(n_sc + 1, 0);
        for (size_t s = 0; s < n_sc; ++s) off[s + 1] = off[s] + (int32_t)(L.scen_static[s].size() / 2);
        std::vector<double> all;
        all.reserve(2 * (size_t)off[n_sc]);
        for (size_t s = 0; s < n_sc; ++s) all.insert(all.end(), L.scen_static[s].begin(), L.scen_static[s].end());
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, L.dScenStatic.ensure(sizeof(double) * std::max<size_t>(all.size(), 2)));
        if (!all.empty()) HIP_TRY(h, hipMemcpy(L.dScenStatic.p, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice));
        L.scen_static_off = off;
        L.scen_static_dirty = false;
    }
    int32_t most = 0;
    for (size_t s = 0; s + 1 < L.scen_static_off.size(); ++s) most = std::max(most, L.scen_static_off[s + 1] - L.scen_static_off[s]);
    const size_t need = sizeof(double) * 2 * (size_t)most * (size_t)std::max(n_req, 1);
    if (need > L.dGather.cap || sizeof(StaticGather) * (size_t)std::max(n_req, 1) > L.hGather.cap) {
        HIP_TRY(h, hipStreamSynchronize(st));                    // (a block that grows moves)
        HIP_TRY(h, L.dGather.ensure(std::max<size_t>(need, 16)));
        HIP_TRY(h, L.hGather.ensure(sizeof(StaticGather) * (size_t)std::max(n_req, 1)));
    }
    return FOT_OK;
}

// FOT_LOOP_PLAN_REPRESENTATIVE: room for a frame of n_ep episodes on slots below n_slots with `rows` pedestrians and T time
// entries per track, each of S samples (the rows of the selection's table are best_dev_stride(S) apart).  (A block that
// grows is freed first, which waits for the device: nothing still reads the old one.)
int rep_ensure(fot_handle *h, int n_slots, int n_ep, size_t rows, int T, int S)
{
    LoopRep &Q = h->loop.rep;
    const size_t ns = (size_t)std::max(n_slots, 1), ne = (size_t)std::max(n_ep, 1);
    HIP_TRY(h, Q.dBlk.ensure(sizeof(double) * 2 * std::max<size_t>(rows, 1) * (size_t)T));
    HIP_TRY(h, Q.dBest.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, Q.dDev.ensure(sizeof(double) * ns * (size_t)best_dev_stride(S)));
    HIP_TRY(h, Q.dPre.ensure(sizeof(int32_t) * ne));
    HIP_TRY(h, Q.hBest.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, Q.hPre.ensure(sizeof(int32_t) * ne));
    return FOT_OK;
}

// A resident sweep loop (fot_loop_begin_sweep) that predicts S samples: the selection's tables, the steps' SweepEp rows and
// a tensor with room for every slot's planning block behind the distribution blocks, so that nothing grows inside a run.
int sweep_ensure(fot_handle *h, int S)
{
    LoopState &L = h->loop;
    const LoopReplay &R = L.replay;
    const int n = R.cfg.n_slots, T = R.n_dense + 1;
    { int r = rep_ensure(h, n, n, 0, T, S); if (r != FOT_OK) return r; }
    HIP_TRY(h, L.hSweep.ensure(sizeof(SweepEp) * (size_t)std::max(n, 1)));
    HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * (size_t)sweep_capacity_points(S, std::max(R.n_cols, 1), T)));
    return FOT_OK;
}

// The planning blocks of the frame's n episodes behind their distribution blocks in dDyn (f: pos, ped0, blk): the
// selection into the given tables (the mode's own, or the scores' where a resident loop scores too), then
// k_loop_rep_block.  Enqueue only.
int rep_enqueue(fot_handle *h, const int32_t *slot_of, const FrameDev &f, int n, int S, int n_dense, double *dev_tab,
                int32_t *best_tab, int32_t *best_host, hipStream_t st)
{
    LoopState &L = h->loop;
    LoopRep &Q = L.rep;
    LAUNCH_TRY(h, launch_loop_best_sample(slot_of, f, L.dDyn.as<double>(), n, S, n_dense, dev_tab, best_tab, best_host, st));
    LAUNCH_TRY(h, launch_loop_rep_block(slot_of, f, L.dDyn.as<double>(), best_tab, n, S, n_dense, Q.dBlk.as<double>(),
                                        Q.dPre.as<int32_t>(), (int32_t *)Q.hPre.p, st));
    return FOT_OK;
}

// The requests of a loop step as one plan call against the step's tensor (LoopState: pedestrian counts, block offsets and
// lengths of the frame's episodes), records to rec_out: enqueued on st, not waited for.
int loop_enqueue_requests(fot_handle *h, int32_t n_req, const fot_loop_request *req, fot_result *rec_out, hipStream_t st,
                          bool sync_caller)
{
    LoopState &L = h->loop;
    const int n_ep = (int)L.ped_off.size() - 1;
    const bool by_scen = !L.frame_scen.empty();                  // a scenario loop: request j is on its episode's scenario
    const int n_static = by_scen ? 0 : (int)(L.static_xy.size() / 2);
    std::vector<int32_t> scen;
    if (by_scen) {
        scen.resize((size_t)n_req);
        for (int j = 0; j < n_req; ++j) {
            const int e = req[j].episode;
            if (e < 0 || e >= n_ep || e >= (int)L.frame_scen.size()) return fail(h, FOT_ERR_INVALID, "request: episode out of range");
            scen[(size_t)j] = L.frame_scen[(size_t)e];
        }
        int r = ensure_scen_static(h, n_req, st); if (r != FOT_OK) return r;
    }
    if (n_static > 0 && L.static_tiles < n_req) {              // (grows a few times in the life of a loop)
        const int tiles = std::max(n_req, 2 * L.static_tiles);
        std::vector<double> rep((size_t)tiles * L.static_xy.size());
        for (int t = 0; t < tiles; ++t)
            std::memcpy(rep.data() + (size_t)t * L.static_xy.size(), L.static_xy.data(), sizeof(double) * L.static_xy.size());
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, L.dStatic.ensure(sizeof(double) * rep.size()));
        HIP_TRY(h, hipMemcpy(L.dStatic.p, rep.data(), sizeof(double) * rep.size(), hipMemcpyHostToDevice));
        L.static_tiles = tiles;
    }
    std::vector<fot_ego> ego((size_t)n_req);
    std::vector<fot_overrides> ov((size_t)n_req);
    std::vector<double> tgt((size_t)n_req), stop((size_t)n_req);
    std::vector<int32_t> s_off((size_t)n_req + 1), dims(4 * (size_t)n_req);
    std::vector<int64_t> d_off((size_t)n_req);
    bool any_dyn = false;
    for (int j = 0; j < n_req; ++j) {
        const int e = req[j].episode;
        if (e < 0 || e >= n_ep) return fail(h, FOT_ERR_INVALID, "request: episode out of range");
        ego[j] = req[j].ego; ov[j] = req[j].overrides; tgt[j] = req[j].target_speed; stop[j] = req[j].max_stop_distance;
        if (!by_scen) s_off[j] = j * n_static;
        if (by_scen) {
            // its scenario's points: gathered on the device into [s_off[j], s_off[j + 1]) of dGather, the layout k_cull reads
            const int32_t sc = scen[(size_t)j], src = L.scen_static_off[(size_t)sc], cnt = L.scen_static_off[(size_t)sc + 1] - src;
            StaticGather &g = ((StaticGather *)L.hGather.p)[j];
            g.src = src; g.dst = s_off[j]; g.n = cnt; g._pad = 0;
            s_off[j + 1] = s_off[j] + cnt;
        }
        const int P_e = L.ped_off[e + 1] - L.ped_off[e];
        if (L.rep.frame) {
            // its episode's representative sample: one [P_e][T][2] block per episode, in the frame's pedestrian order
            d_off[j] = (int64_t)L.ped_off[e] * L.rep.T;
            dims[4 * j] = P_e > 0 ? FOT_DYN_SINGLE : FOT_DYN_NONE;
            dims[4 * j + 1] = 1; dims[4 * j + 2] = P_e; dims[4 * j + 3] = L.rep.T;
        } else if (!L.sweep_tab.empty() && sweep_plans_on_block(L.sweep_tab[(size_t)e])) {
            // a sweep loop's episode in representative mode: its block behind the distribution blocks of the same tensor
            d_off[j] = L.sweep_tab[(size_t)e].rep_off;
            dims[4 * j] = P_e > 0 ? FOT_DYN_SINGLE : FOT_DYN_NONE;
            dims[4 * j + 1] = 1; dims[4 * j + 2] = P_e; dims[4 * j + 3] = L.sweep_T;
        } else {
            d_off[j] = L.blk_off[e];
            dims[4 * j] = P_e > 0 ? (L.dist_S > 0 ? FOT_DYN_DISTRIBUTION : FOT_DYN_SINGLE) : FOT_DYN_NONE;
            dims[4 * j + 1] = L.dist_S > 0 ? L.count_of((size_t)e) : 1; dims[4 * j + 2] = P_e; dims[4 * j + 3] = L.t_len[e];
        }
        any_dyn = any_dyn || P_e > 0;
    }
    if (!by_scen) s_off[n_req] = n_req * n_static;
    fot_batch b = fot_batch();
    b.n_inst = n_req; b.obstacle_dtype = FOT_F64;
    b.ego = ego.data(); b.target_speed = tgt.data(); b.overrides = ov.data(); b.max_stop_distance = stop.data();
    if (n_static > 0) { b.static_xy = L.dStatic.p; b.static_off = s_off.data(); }
    if (by_scen && s_off[n_req] > 0) {
        if (sizeof(double) * 2 * (size_t)s_off[n_req] > L.dGather.cap) return fail(h, FOT_ERR_INVALID, "internal: static block too small");
        { int r = check_scenarios(h, b, scen.data()); if (r != FOT_OK) return r; }   // (a refused call enqueues nothing)
        { int r = order_begin(h, st); if (r != FOT_OK) return r; }
        LAUNCH_TRY(h, launch_static_gather((const StaticGather *)L.hGather.p, n_req, L.dScenStatic.as<double>(),
                                           L.dGather.as<double>(), st));
        b.static_xy = L.dGather.p; b.static_off = s_off.data();
    }
    if (any_dyn) { b.dyn_xy = L.rep.frame ? L.rep.dBlk.p : L.dyn_ptr; b.dyn_off = d_off.data(); b.dyn_dims = dims.data(); }
    return enqueue_plan(h, b, by_scen ? scen.data() : nullptr, b.static_xy, b.dyn_xy, rec_out, st, sync_caller);
}

// fot_loop_plan; rec_first: the request's records start at record rec_first of the handle's pinned block (the escalation
// levels of a step land behind its level-0 records, which stay where they are)
// ep_scen: the scenario of each episode of the frame (a scenario loop's step), or nullptr: all on scenario 0
// ep_slot: the slot of each episode of the frame (fot_loop_step), or nullptr: episode i is slot i (what the representative
// sample's tables are indexed by)
int loop_plan_impl(fot_handle *h, const fot_loop_frame *frame, int32_t n_req, const fot_loop_request *req,
                   fot_safety *safety_out, const fot_result **records, int32_t rec_first, const int32_t *ep_scen = nullptr,
                   const int32_t *ep_slot = nullptr)
{
    if (!h) return FOT_ERR_INVALID;
    if (!ep_scen && (frame || h->loop.frame_scen.empty()) && !h->sc[0].has_path)
        return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    if (n_req < 0 || (n_req > 0 && (!req || !records))) return fail(h, FOT_ERR_INVALID, "requests");
    LoopState &L = h->loop;
    if (!frame && !L.have_frame) return fail(h, FOT_ERR_INVALID, "no frame: the first fot_loop_plan of a step carries one");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (L.observe_n > 0) {                                       // a fot_loop_observe_begin nobody collected: its launches
        HIP_TRY(h, hipStreamSynchronize(st));                    // still read the frame's pinned block
        L.observe_n = -1;
    }
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    bool metrics = false, rep_pending = false;
    std::vector<int32_t> rep_slots;                              // the frame's slots, where it left representative samples
    if (frame) {
        const int n = frame->n_episodes;
        if (n < 0 || !frame->ped_off) return fail(h, FOT_ERR_INVALID, "frame: n_episodes / ped_off (one offset even for no episode)");
        L.have_frame = false;
        for (int i = 0; i < n; ++i)
            if (frame->ped_off[i + 1] < frame->ped_off[i] || frame->ped_off[0] != 0)
                return fail(h, FOT_ERR_INVALID, "ped_off must start at 0 and be non-decreasing");
        const size_t n_ped = n > 0 ? (size_t)frame->ped_off[n] : 0;
        if (n_ped > 0 && (!frame->ped_pos || !frame->ped_vel)) return fail(h, FOT_ERR_INVALID, "frame: NULL pedestrian array");
        const bool ready = frame->obs_last != nullptr;
        const bool dist = ready && frame->dist_raw != nullptr;
        // (the capacity first: more samples than the handle accepts are FOT_ERR_UNSUPPORTED whatever else the frame holds)
        if (dist && frame->dist_S > h->sample_cap) return refuse_samples(h, "frame: dist_", frame->dist_S);
        if (dist && (frame->dist_S < 1 || (frame->dist_dtype != FOT_F32 && frame->dist_dtype != FOT_F64)))
            return fail(h, FOT_ERR_INVALID, "frame: dist_S / dist_dtype");
        if (ready && !dist && n > 0 && !frame->prepend) return fail(h, FOT_ERR_INVALID, "frame: prepend missing");
        if (ready && (!(frame->rp.sim_dt > 0.0) || !(frame->rp.sgan_dt > 0.0) || frame->pred_len < 1 ||
                      frame->pred_len > FOT_MAX_PRED_LEN))
            return fail(h, FOT_ERR_INVALID, "frame: predictor parameters");
        const int n_dense = ready ? resample_n_dense(frame->rp.sgan_dt, frame->rp.sim_dt, frame->rp.plan_horizon, frame->pred_len) : 1;
        if (n_dense + 1 > FOT_MAX_NT) return fail(h, FOT_ERR_UNSUPPORTED, "more than FOT_MAX_NT time steps");
        // pinned block: ego[n][4] | ped_off | pos | vel | obs_last (widened) | obs_prev (widened) | block offsets | ped -> episode
        const size_t ego_b = align256(sizeof(double) * 4 * (size_t)std::max(n, 1));
        const size_t off_b = align256(sizeof(int32_t) * ((size_t)n + 1));
        const size_t ped_b = align256(sizeof(double) * 2 * std::max<size_t>(n_ped, 1));
        const size_t blk_b = align256(sizeof(int64_t) * ((size_t)n + 1)), pe_b = align256(sizeof(int32_t) * std::max<size_t>(n_ped, 1));
        const bool rep_on = L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE && dist;   // (never a scenario loop: the tail is free)
        // a sweep loop's frame with a distribution needs both tail tables and, behind them, the episodes' SweepEp rows
        const bool sweep_on = L.ep.sweep && ep_scen && dist;
        // ... whose slots keep their own sample counts (fot_loop_set_slot_samples): the episodes' counts behind those; a
        // frame whose episodes all keep the source's count is the frame of before
        bool ragged = false;
        for (int e = 0; sweep_on && !L.slot_S.empty() && e < n; ++e) {
            const int slot = ep_slot ? ep_slot[e] : e;
            if (slot < 0 || slot >= (int)L.slot_S.size()) return fail(h, FOT_ERR_INVALID, "frame: an episode's slot lies outside the loop's sample counts");
            if (L.slot_S[(size_t)slot] > frame->dist_S)
                return fail(h, FOT_ERR_INVALID, "frame: dist_S = " + std::to_string(frame->dist_S) + " is below the sample count of slot " +
                                                std::to_string(slot) + " (fot_loop_set_slot_samples: " + std::to_string(L.slot_S[(size_t)slot]) + ")");
            ragged = ragged || L.slot_S[(size_t)slot] != frame->dist_S;
        }
        const size_t tail = ego_b + off_b + 4 * ped_b + blk_b + pe_b;
        const size_t sweep_b = align256(sizeof(SweepEp) * (size_t)std::max(n, 1));
        HIP_TRY(h, L.hFrame.ensure(tail + (ep_scen || rep_on ? off_b : 0) + (sweep_on ? off_b + sweep_b : 0) + (ragged ? off_b : 0)));
        char *p = (char *)L.hFrame.p;
        double *p_ego = (double *)p;
        int32_t *p_off = (int32_t *)(p + ego_b);
        double *p_pos = (double *)(p + ego_b + off_b), *p_vel = (double *)((char *)p_pos + ped_b);
        double *p_last = (double *)((char *)p_vel + ped_b), *p_prev = (double *)((char *)p_last + ped_b);
        if (frame->ego) std::memcpy(p_ego, frame->ego, sizeof(double) * 4 * (size_t)n);
        std::memcpy(p_off, frame->ped_off, sizeof(int32_t) * ((size_t)n + 1));
        if (n_ped) {
            std::memcpy(p_pos, frame->ped_pos, sizeof(double) * 2 * n_ped);
            std::memcpy(p_vel, frame->ped_vel, sizeof(double) * 2 * n_ped);
            if (ready) for (size_t i = 0; i < 2 * n_ped; ++i) p_last[i] = (double)frame->obs_last[i];   // (exact)
            if (ready && frame->obs_prev) for (size_t i = 0; i < 2 * n_ped; ++i) p_prev[i] = (double)frame->obs_prev[i];
        }
        L.ped_off.assign(frame->ped_off, frame->ped_off + n + 1);
        L.blk_off.assign((size_t)n + 1, 0);
        L.t_len.assign((size_t)std::max(n, 1), 1);
        L.dist_S = dist ? frame->dist_S : 0;
        L.rep.frame = false;
        L.sweep_tab.clear();
        L.ep_S.clear();
        int S_run = dist ? frame->dist_S : 0, P_run = 0;             // the largest count / pedestrian count of the frame
        if (ragged) {
            L.ep_S.resize((size_t)n);
            S_run = sweep_slot_counts(n, ep_slot, L.slot_S.data(), L.ep_S.data());
        }
        for (int e = 0; e < n; ++e) {
            L.t_len[e] = dist ? n_dense + 1 : ready ? n_dense + (frame->prepend[e] ? 1 : 0) : 1;
            L.blk_off[e + 1] = L.blk_off[e] + (int64_t)(dist ? L.count_of((size_t)e) : 1) * (L.ped_off[e + 1] - L.ped_off[e]) * L.t_len[e];
            P_run = std::max(P_run, L.ped_off[e + 1] - L.ped_off[e]);
        }
        L.p_off = p_off; L.p_pos = p_pos; L.p_vel = p_vel;
        L.p_scen = nullptr; L.frame_scen.clear();
        if (ep_scen && n > 0) {                                    // the episodes' scenarios, behind the other tables
            int32_t *p_sc = (int32_t *)(p + ego_b + off_b + 4 * ped_b + blk_b + pe_b);
            std::memcpy(p_sc, ep_scen, sizeof(int32_t) * (size_t)n);
            L.p_scen = p_sc; L.frame_scen.assign(ep_scen, ep_scen + n);
        }
        L.ego_radius = frame->ego_radius; L.ped_radius = frame->ped_radius; L.use_footprint = frame->use_footprint;
        L.dyn_ptr = p_pos;                                         // not ready: the current positions, read in place
        if (dist && n_ped > 0) {
            // every sample of every pedestrian in one launch, each episode's samples into its own [S][P_e][T][2] block
            int64_t *p_blk = (int64_t *)((char *)p_prev + ped_b);
            int32_t *p_pe = (int32_t *)((char *)p_blk + blk_b);
            for (int e = 0; e <= n; ++e) p_blk[e] = L.blk_off[e];
            for (int e = 0; e < n; ++e) for (int q = L.ped_off[e]; q < L.ped_off[e + 1]; ++q) p_pe[q] = e;
            int64_t tensor_pts = L.blk_off[n];
            int32_t *p_slot = (int32_t *)(p + tail + off_b);     // (a sweep frame: the slots behind the scenarios)
            SweepEp *p_sweep = (SweepEp *)(p + tail + 2 * off_b);
            if (sweep_on) {
                for (int e = 0; e < n; ++e) p_slot[e] = ep_slot ? ep_slot[e] : e;
                tensor_pts = sweep_layout(n, L.ped_off.data(), p_slot, L.ep.plan_mode.data(), L.blk_off[n], n_dense + 1, false, p_sweep);
            }
            int32_t *p_eps = (int32_t *)(p + tail + 2 * off_b + sweep_b);    // (... and the episodes' sample counts behind the rows)
            if (ragged) std::memcpy(p_eps, L.ep_S.data(), sizeof(int32_t) * (size_t)n);
            HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * (size_t)tensor_pts));
            L.dyn_ptr = L.dDyn.p;
            if (ragged)
                LAUNCH_TRY(h, launch_resample_slots(frame->rp.sgan_dt, frame->rp.sim_dt, frame->staleness, S_run, frame->pred_len,
                                                    (int)n_ped, n_dense, n, P_run, frame->dist_raw, frame->dist_dtype, p_last, p_pos,
                                                    L.dDyn.as<double>(), p_off, p_blk, p_eps, st));
            else
                LAUNCH_TRY(h, launch_resample(frame->rp.sgan_dt, frame->rp.sim_dt, frame->staleness, frame->dist_S, frame->pred_len,
                                              (int)n_ped, n_dense, 1, 1, 0, frame->dist_raw, frame->dist_dtype, p_last, p_pos,
                                              L.dDyn.p, FOT_F64, 0, st, p_pe, p_off, p_blk));
            if (sweep_on && tensor_pts > L.blk_off[n]) {
                // the selection and the planning blocks of the episodes in representative mode, behind the resample
                { int r = rep_ensure(h, std::max(L.ep.n, n), n, 0, n_dense + 1, frame->dist_S); if (r != FOT_OK) return r; }
                FrameDev fd;
                fd.pos = p_pos; fd.ped0 = p_off; fd.blk = p_blk;
                if (ragged) {
                    LAUNCH_TRY(h, launch_loop_best_sample_slots(p_slot, fd, L.dDyn.as<double>(), p_sweep, p_eps, n, S_run, n_dense,
                                                                L.rep.dDev.as<double>(), best_dev_stride(frame->dist_S),
                                                                L.rep.dBest.as<int32_t>(), (int32_t *)L.rep.hBest.p, st));
                    LAUNCH_TRY(h, launch_loop_rep_block_slots(p_slot, fd, L.dDyn.as<double>(), p_sweep, p_eps, L.rep.dBest.as<int32_t>(),
                                                              n, n_dense, L.dDyn.as<double>(), L.rep.dPre.as<int32_t>(),
                                                              (int32_t *)L.rep.hPre.p, st));
                } else {
                LAUNCH_TRY(h, launch_loop_best_sample_sweep(p_slot, fd, L.dDyn.as<double>(), p_sweep, n, frame->dist_S, n_dense,
                                                            L.rep.dDev.as<double>(), L.rep.dBest.as<int32_t>(),
                                                            (int32_t *)L.rep.hBest.p, st));
                LAUNCH_TRY(h, launch_loop_rep_block_sweep(p_slot, fd, L.dDyn.as<double>(), p_sweep, L.rep.dBest.as<int32_t>(), n,
                                                          frame->dist_S, n_dense, L.dDyn.as<double>(), L.rep.dPre.as<int32_t>(),
                                                          (int32_t *)L.rep.hPre.p, st));
                }
                L.sweep_tab.assign(p_sweep, p_sweep + n);
                L.sweep_T = n_dense + 1;
                rep_pending = true;
                rep_slots.assign(p_slot, p_slot + n);
            }
            if (rep_on) {
                // the selection and every episode's single-sample block behind the resample, on the same stream
                int32_t *p_slot = (int32_t *)(p + ego_b + off_b + 4 * ped_b + blk_b + pe_b);
                int n_tab = std::max(L.ep.n, n);
                for (int e = 0; e < n; ++e) p_slot[e] = ep_slot ? ep_slot[e] : e;
                { int r = rep_ensure(h, n_tab, n, n_ped, n_dense + 1, frame->dist_S); if (r != FOT_OK) return r; }
                FrameDev fd;
                fd.pos = p_pos; fd.ped0 = p_off; fd.blk = p_blk;
                { int r = rep_enqueue(h, p_slot, fd, n, frame->dist_S, n_dense, L.rep.dDev.as<double>(), L.rep.dBest.as<int32_t>(),
                                      (int32_t *)L.rep.hBest.p, st); if (r != FOT_OK) return r; }
            }
        } else if (ready && n_ped > 0) {
            HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * (size_t)L.blk_off[n]));
            L.dyn_ptr = L.dDyn.p;
            // one launch per run of episodes that agree on the prepend (normally one run: the whole frame)
            for (int e0 = 0; e0 < n;) {
                int e1 = e0 + 1;
                while (e1 < n && (frame->prepend[e1] != 0) == (frame->prepend[e0] != 0)) ++e1;
                const int r0 = L.ped_off[e0], cnt = L.ped_off[e1] - r0, pre = frame->prepend[e0] ? 1 : 0;
                if (cnt > 0)
                    LAUNCH_TRY(h, launch_resample(frame->rp.sgan_dt, frame->rp.sim_dt, frame->staleness, 1, frame->pred_len,
                                                  cnt, n_dense, 1, pre, 2, frame->obs_prev ? p_prev + 2 * (size_t)r0 : nullptr,
                                                  FOT_F64, p_last + 2 * (size_t)r0, pre ? p_pos + 2 * (size_t)r0 : nullptr,
                                                  L.dDyn.as<double>() + 2 * L.blk_off[e0], FOT_F64, 0, st));
                e0 = e1;
            }
        }
        if (frame->ego && safety_out && n > 0) {
            HIP_TRY(h, L.hOut.ensure(sizeof(fot_safety) * (size_t)n));
            LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, p_ego, p_off, p_pos, p_vel, L.ego_radius, L.ped_radius,
                                        h->sc[0].params.footprint_radius, L.use_footprint, (fot_safety *)L.hOut.p, st,
                                        L.p_scen, L.dSafScen.as<SafetyScen>()));
            metrics = true;
        }
        if (rep_on) {
            L.rep.frame = true; L.rep.T = n_dense + 1;
            rep_pending = n_ped > 0;
            rep_slots.assign((size_t)n, 0);
            for (int e = 0; e < n; ++e) rep_slots[(size_t)e] = ep_slot ? ep_slot[e] : e;
        }
        L.have_frame = true;
    }
    const int n_ep = (int)L.ped_off.size() - 1;
    if (n_req > 0) {
        if (rec_first > 0 && sizeof(fot_result) * ((size_t)rec_first + (size_t)n_req) > L.hRec.cap)
            return fail(h, FOT_ERR_INVALID, "internal: record block too small for the escalation levels");
        HIP_TRY(h, L.hRec.ensure(sizeof(fot_result) * ((size_t)rec_first + (size_t)n_req)));
        fot_result *rec_out = (fot_result *)L.hRec.p + rec_first;
        {
            // the records' flags instead of the stream (wait_records): the metrics' kernel ran ahead of the plan kernels on
            // this stream and wrote host memory directly, so its results are there once a record behind it is
            arm_records(h, n_req);
            int rc = loop_enqueue_requests(h, n_req, req, rec_out, st, true);
            if (rc != FOT_OK) { h->done_seq_armed = false; return rc; }
            rc = wait_records(h, n_req, st);
            if (rc != FOT_OK) return rc;
        }
    } else {
        int r = order_end(h, st); if (r != FOT_OK) return r;
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    if (metrics) std::memcpy(safety_out, L.hOut.p, sizeof(fot_safety) * (size_t)n_ep);
    if (frame && (L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE || L.ep.sweep))   // (a frame without a distribution chose nothing)
        std::fill(L.rep.last_best.begin(), L.rep.last_best.end(), -1);
    if (frame && (L.rep.frame || !L.sweep_tab.empty())) {        // (the selection ran ahead of the plan on this stream)
        const int32_t *best = (const int32_t *)L.rep.hBest.p;
        for (size_t e = 0; e < rep_slots.size(); ++e) {
            const int slot = rep_slots[e];
            if (!L.sweep_tab.empty() && !sweep_plans_on_block(L.sweep_tab[e])) continue;   // (a sweep's distribution mode)
            if (rep_pending && slot < (int)L.rep.last_best.size() && L.ped_off[e + 1] > L.ped_off[e]) L.rep.last_best[(size_t)slot] = best[slot];
        }
    }
    if (records) *records = n_req > 0 ? (const fot_result *)L.hRec.p + rec_first : nullptr;
    return FOT_OK;
}

// fot_loop_observe_begin; a scenario loop's frame (LoopState::frame_scen): ego i is measured with, and projected on the
// path of, the scenario of episode i.  fpo_slot: the slot of every ego, from the one-call step and the resident step -- with
// fot_loop_footprint_enable on, the footprint observation of the same poses and frame rows follows k_safety
int observe_begin_impl(fot_handle *h, int32_t n, const double *ego5, const double *prev_s, const int32_t *fpo_slot = nullptr)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    const bool by_scen = !L.frame_scen.empty();
    if (!by_scen && !h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    L.observe_n = -1;
    if (!L.have_frame) return fail(h, FOT_ERR_INVALID, "no frame: fot_loop_plan of this step comes first");
    if (n != (int)L.ped_off.size() - 1) return fail(h, FOT_ERR_INVALID, "one ego per episode of the frame");
    if (n <= 0) { L.observe_n = 0; return FOT_OK; }
    if (!ego5) return fail(h, FOT_ERR_INVALID, "ego5 is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    const size_t ego_b = align256(sizeof(double) * 4 * (size_t)n), desc_b = align256(sizeof(InstDesc) * (size_t)n);
    const size_t saf_b = align256(sizeof(fot_safety) * (size_t)n);
    HIP_TRY(h, L.hObserve.ensure(ego_b + desc_b));
    HIP_TRY(h, L.hOut.ensure(saf_b + sizeof(InstState) * (size_t)n));
    double *p_ego = (double *)L.hObserve.p;
    InstDesc *p_desc = (InstDesc *)((char *)L.hObserve.p + ego_b);
    for (int i = 0; i < n; ++i) {
        const double *e = ego5 + 5 * (size_t)i;
        p_ego[4 * i] = e[0]; p_ego[4 * i + 1] = e[1]; p_ego[4 * i + 2] = e[2]; p_ego[4 * i + 3] = e[3];
        InstDesc d = InstDesc();
        d.ego.x = e[0]; d.ego.y = e[1]; d.ego.yaw = e[2]; d.ego.v = e[3]; d.ego.a = e[4];
        const bool cached = prev_s && !std::isnan(prev_s[i]);
        d.ego.has_prev_s = cached ? 1 : 0;
        d.ego.prev_s = cached ? prev_s[i] : 0.0;
        d.scen = by_scen ? L.frame_scen[(size_t)i] : 0;
        p_desc[i] = d;
    }
    LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, p_ego, L.p_off, L.p_pos, L.p_vel, L.ego_radius, L.ped_radius,
                                h->sc[0].params.footprint_radius, L.use_footprint, (fot_safety *)L.hOut.p, st,
                                L.p_scen, L.dSafScen.as<SafetyScen>()));
    if (L.fpo.on && fpo_slot)
        LAUNCH_TRY(h, launch_footprint_steps((const FpoGeom *)L.fpo.hGeom.p, n, p_ego, 4, p_ego + 2, 4, L.p_off, L.p_pos,
                                             (FpoStep *)L.fpo.hRec.p, st));
    InstState *p_state = (InstState *)((char *)L.hOut.p + saf_b);
    PathSet ps = PathSet::single(spline_view(h, 0));
    if (by_scen) {                                               // the handle's path table, as a mixed plan batch passes it
        ps = PathSet();
        ps.table = h->dSplineTab.as<SplineView>();
        ps.mixed = 1;
        std::vector<uint8_t> used(h->sc.size(), 0);
        for (int i = 0; i < n; ++i) used[(size_t)L.frame_scen[(size_t)i]] = 1;
        for (size_t sc = 0; sc < used.size(); ++sc) if (used[sc]) ps.knots[ps.n_knots++] = h->sc[sc].spline.n;
    }
    LAUNCH_TRY(h, launch_frenet_state(h->dP.as<DevParams>(), ps, p_desc, p_state, n, MetaImport(), NanScan(), nullptr, st));
    { int r = order_end(h, st); if (r != FOT_OK) return r; }
    L.observe_n = n;
    return FOT_OK;
}

// The lock step's footprint records into the slots' accumulators: k_footprint_steps ran behind k_safety on the new ego
// states, and the caller has waited for the step's observation.  Ego i belongs to slot[i] and met episode i of the frame.
void fpo_fold_step(LoopState &L, const int32_t *slot, int n)
{
    LoopFootprintObs &F = L.fpo;
    if (!F.on) return;
    const FpoStep *r = (const FpoStep *)F.hRec.p;
    for (int i = 0; i < n; ++i) {
        const size_t e = (size_t)slot[i];
        fpo_acc_step(F.acc[e], F.geom, r[i].legacy, r[i].multi, r[i].rect, L.ped_off[(size_t)i + 1] > L.ped_off[(size_t)i]);
        F.steps[e] += 1;
    }
}

// ---- the whole lock step of n episodes behind ONE call (SURVEY 8 f2 + f4) -------------------------------------------

// FailSafeStateMachine._get_planner_config (state_machine.py:181-247): the planner configuration of `state` on the
// clearance ahead the machine last observed -> target speed, constraint overrides (NaN = absent), stop room (NaN = None)
void sm_config(const fot_loop_config &c, int state, double clear_ahead, double *target, fot_overrides *ov, double *stop)
{
    const bool fin = std::isfinite(clear_ahead), has_env = fin && c.envelope_decel > 0.0;
    const double v_env = std::sqrt(2.0 * c.envelope_decel * std::fmax((fin ? clear_ahead : 0.0) - c.envelope_standoff, 0.0));
    const double stop_room = fin ? std::fmax(clear_ahead - 0.2, 0.05) : NAN;
    *target = c.target_speed;
    ov->max_speed = ov->max_accel = ov->max_curvature = ov->max_lat_accel = NAN;
    *stop = NAN;
    if (state == 0) {
        if (has_env && v_env < c.target_speed) *target = v_env;
    } else if (state == 1) {
        const double t_ca = c.target_speed * c.caution_speed_mult;
        *target = has_env ? std::fmin(t_ca, v_env) : t_ca;
        if (has_env && v_env <= 0.0) *stop = stop_room;
        ov->max_accel = c.caution_accel; ov->max_speed = c.caution_speed;
    } else {
        *target = 0.0;
        ov->max_accel = c.emergency_accel; ov->max_lat_accel = c.emergency_lat_accel;
        if (c.envelope_decel > 0.0) *stop = stop_room;
    }
}

// FailSafeStateMachine.update (state_machine.py:116-179) of episode e: observe the metrics, then the transition
void sm_update(LoopEpisodes &E, int e, bool found, double clearance, double clearance_ahead, double speed)
{
    const fot_loop_config &c = E.cfg_of(e);
    E.clear[e] = clearance; E.clear_ahead[e] = clearance_ahead;
    const int st = E.state[e], fl = E.fails[e];
    const double trigger = c.trigger_clearance_caution + c.trigger_time_headway * std::fmax(speed, 0.0);
    if (st == 0) {
        if (!found) { E.state[e] = 1; E.fails[e] = fl + 1; }
        else if (trigger > 0.0 && clearance < trigger) { E.state[e] = 1; E.fails[e] = 0; }   // preventive escalation
        else E.fails[e] = 0;
    } else if (st == 1) {
        if (found && fl == 0) { if (clearance > std::fmax(c.clearance_caution, trigger)) E.state[e] = 0; }
        else if (!found) { E.state[e] = 2; E.fails[e] = fl + 1; }
        else E.fails[e] = 0;
    } else {
        if (found && clearance > c.clearance_emergency) E.state[e] = 1;
    }
}

// ---- the host side of one lock step, shared by fot_loop_step (records in pinned memory) and fot_loop_run (digests of
//      records that stay in HBM): Rec is fot_result or LoopDigest, which name the fields read here alike
void rec_sample1(const fot_result &r, double *g) { g[0] = r.x[1]; g[1] = r.y[1]; g[2] = r.yaw[1]; g[3] = r.v[1]; g[4] = r.a[1]; }
void rec_sample1(const LoopDigest &r, double *g) { g[0] = r.x1; g[1] = r.y1; g[2] = r.yaw1; g[3] = r.v1; g[4] = r.a1; }

int loop_max_levels(const fot_loop_config &c) { return 1 + c.max_replan < 3 ? 1 + c.max_replan : 3; }   // NORMAL -> CAUTION -> EMERGENCY, then no change

struct StepWork {
    std::vector<int> st0, n_lvl, next_rec, path_rec, keep;
    std::vector<double> speed, ego4, ego5n, jerk, cost;
    std::vector<fot_loop_request> req, more;
    std::vector<fot_safety> m;               // metrics of the current ego states
};

// level 0 of every episode: the configuration of its current state (issued on LAST step's clearance); request i plans
// against episode i of the frame
void step_level0(const LoopEpisodes &E, const int32_t *episode, int n, StepWork &W)
{
    W.st0.assign((size_t)n, 0); W.n_lvl.assign((size_t)n, 0);
    W.speed.assign((size_t)n, 0.0); W.ego4.assign(4 * (size_t)n, 0.0);
    W.req.assign((size_t)n, fot_loop_request());
    W.m.assign((size_t)n, fot_safety());
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);                   // (the episode's own scenario's constants)
        W.st0[i] = E.state[e];
        W.n_lvl[i] = std::min(3 - W.st0[i], loop_max_levels(c));
        const double *g = &E.ego[5 * (size_t)e];
        W.speed[i] = g[3];
        for (int k = 0; k < 4; ++k) W.ego4[4 * (size_t)i + k] = g[k];
        fot_loop_request &r = W.req[i];
        r = fot_loop_request();
        r.ego.x = g[0]; r.ego.y = g[1]; r.ego.yaw = g[2]; r.ego.v = g[3]; r.ego.a = g[4];
        r.ego.last_kappa = E.last_kappa[e];
        r.ego.has_prev_s = std::isnan(E.prev_s[e]) ? 0 : 1;
        r.ego.prev_s = std::isnan(E.prev_s[e]) ? 0.0 : E.prev_s[e];
        sm_config(c, W.st0[i], E.clear_ahead[e], &r.target_speed, &r.overrides, &r.max_stop_distance);
        r.episode = i;
    }
}

// episodes whose first attempt failed: every further escalation level they can reach, for ONE more launch (the
// configurations update(False, ...) would issue on THIS step's metrics, nearest-point cache chained); their records
// follow the n level-0 records
template <class Rec>
void step_escalations(const LoopEpisodes &E, const int32_t *episode, int n, const Rec *rec, StepWork &W)
{
    W.next_rec.assign((size_t)n, -1);
    W.more.clear();
    for (int i = 0; i < n; ++i) {
        if (rec[i].status == FOT_PLAN_OK || W.n_lvl[i] <= 1) continue;
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);
        W.next_rec[i] = n + (int)W.more.size();
        const double nps0 = rec[i].new_prev_s, p = std::isnan(nps0) ? E.prev_s[e] : nps0;
        for (int lvl = 1; lvl < W.n_lvl[i]; ++lvl) {
            fot_loop_request r = W.req[i];
            const bool chain = lvl > 1;
            r.ego.has_prev_s = chain ? FOT_PREV_S_CHAINED : (std::isnan(p) ? 0 : 1);
            r.ego.prev_s = (chain || std::isnan(p)) ? 0.0 : p;
            sm_config(c, W.st0[i] + lvl, W.m[i].clearance_ahead, &r.target_speed, &r.overrides, &r.max_stop_distance);
            W.more.push_back(r);
        }
    }
}

// replay of the retry loop (integrated_simulator.py:576-653) episode by episode, then the ego update (:655-676) or the
// emergency stop (:749-802): E moves on, W gets the followed record, its kept samples and cost, the jerk and the new egos
template <class Rec>
void step_resolve(LoopEpisodes &E, const int32_t *episode, int n, const Rec *rec, StepWork &W)
{
    W.path_rec.assign((size_t)n, -1); W.keep.assign((size_t)n, 0);
    W.jerk.assign((size_t)n, 0.0); W.cost.assign((size_t)n, 0.0); W.ego5n.assign(5 * (size_t)n, 0.0);
    auto adopt = [&](int i, int r) {                             // planner state after a plan() call
        const int e = episode[i];
        if (!std::isnan(rec[r].new_prev_s)) E.prev_s[e] = rec[r].new_prev_s;
        for (int k = 0; k < 8; ++k) E.stats[8 * (size_t)e + k] = rec[r].stats_valid ? rec[r].stats[k] : -1;
        if (rec[r].status == FOT_PLAN_OK) { E.last_kappa[e] = rec[r].new_last_kappa; W.path_rec[i] = r; }
    };
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);
        int cur = i, retries = 0;
        adopt(i, cur);
        bool found = rec[cur].status == FOT_PLAN_OK;
        int issued = W.st0[i];                                    // state of the configuration the attempt ran under
        sm_update(E, e, found, W.m[i].clearance, W.m[i].clearance_ahead, W.speed[i]);
        while (!found && E.state[e] != issued && retries < c.max_replan && retries + 1 < W.n_lvl[i]) {
            cur = retries == 0 ? W.next_rec[i] : cur + 1;
            ++retries;
            adopt(i, cur);
            const bool ok = rec[cur].status == FOT_PLAN_OK;
            found = found || ok;
            issued = E.state[e];
            if (!ok) sm_update(E, e, false, W.m[i].clearance, W.m[i].clearance_ahead, W.speed[i]);
        }
    }
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        const fot_loop_config &c = E.cfg_of(e);
        double *g = &E.ego[5 * (size_t)e];
        const double old_a = g[4];
        const int r = W.path_rec[i];
        const int keep = r >= 0 ? rec[r].n_keep : 0;
        double jerk;
        if (keep >= 2) {
            rec_sample1(rec[r], g);
            jerk = (g[4] - old_a) / c.dt;
        } else {
            // the position integrates along the heading at the OLD speed; the deceleration is what stopping 0.2 m short
            // of the nearest pedestrian ahead needs, bounded to [max_accel, emergency_decel]
            const double v = g[3], clr = E.last_clearance[e];
            const double cap = std::isnan(c.emergency_decel) ? c.max_accel * 2.0 : c.emergency_decel;
            const double required = std::isfinite(clr) ? v * v / (2.0 * std::fmax(clr - 0.2, 0.05)) : cap;
            const double max_dec = std::fmin(std::fmax(required, c.max_accel), cap);
            const double nv = std::fmax(0.0, v - max_dec * c.dt), na = nv > 0.0 ? -max_dec : 0.0;
            g[0] = g[0] + v * std::cos(g[2]) * c.dt; g[1] = g[1] + v * std::sin(g[2]) * c.dt;
            g[3] = nv; g[4] = na;
            jerk = (na - old_a) / c.dt;
            E.last_kappa[e] = 0.0;                                // planner.reset_ego_curvature()
        }
        for (int k = 0; k < 5; ++k) W.ego5n[5 * (size_t)i + k] = g[k];
        W.jerk[i] = jerk; W.keep[i] = keep; W.cost[i] = rec[r >= 0 ? r : 0].cost;
    }
}

// ---- whole replayed episodes: the recording resident in HBM, the lock steps run by the library ------------------------

// Waits until the device has raised *word to seq (k_loop_digest / k_loop_history, in pinned memory); after 20 ms without
// it the stream is synchronised instead, as wait_records does.
int wait_word(fot_handle *h, const int32_t *word, int32_t seq, hipStream_t st)
{
    if (spin_words(word, 1, seq)) return FOT_OK;
    HIP_TRY(h, hipStreamSynchronize(st));
    return FOT_OK;
}

int32_t next_seq(LoopReplay &R)
{
    if (++R.seq == 0) R.seq = 1;                                  // (0 is what a fresh word holds)
    return R.seq;
}

// the regions of LoopReplay::dFrame / hStage for up to n episodes and `rows` pedestrians
struct FrameLayout {
    size_t ped_b, ep_b, off_b, blk_b, pre_b, ego_b;
    FrameLayout(size_t n, size_t rows)
        : ped_b(align256(16 * std::max<size_t>(rows, 1))), ep_b(align256(4 * std::max<size_t>(rows, 1))),
          off_b(align256(4 * (n + 1))), blk_b(align256(8 * (n + 1))), pre_b(align256(4 * std::max<size_t>(n, 1))),
          ego_b(align256(32 * std::max<size_t>(n, 1))) {}
    size_t dev_bytes() const { return 4 * ped_b + ep_b + off_b + blk_b + pre_b + ego_b + pre_b; }
    // the stage block (hStage), which the host fills and k_loop_frame reads (FrameStage): its regions from `base` on and
    // its size; stage_bytes() is this walk's end
    struct Stage { int32_t *slot, *ped0; int64_t *blk; int32_t *prepend; double *ego; int32_t *scen; size_t bytes; };
    Stage stage(void *base) const
    {
        uintptr_t p = (uintptr_t)base;
        Stage s;
        s.slot = (int32_t *)p; p += pre_b;
        s.ped0 = (int32_t *)p; p += off_b;
        s.blk = (int64_t *)p; p += blk_b;
        s.prepend = (int32_t *)p; p += pre_b;
        s.ego = (double *)p; p += ego_b;
        s.scen = (int32_t *)p; p += pre_b;
        s.bytes = (size_t)(p - (uintptr_t)base);
        return s;
    }
    size_t stage_bytes() const { return stage(nullptr).bytes; }
    FrameDev dev(void *base) const
    {
        char *p = (char *)base;
        FrameDev f;
        f.pos = (double *)p; f.vel = (double *)(p + ped_b); f.last = (double *)(p + 2 * ped_b); f.prev = (double *)(p + 3 * ped_b);
        p += 4 * ped_b;
        f.ped_ep = (int32_t *)p; p += ep_b;
        f.ped0 = (int32_t *)p; p += off_b;
        f.blk = (int64_t *)p; p += blk_b;
        f.prepend = (int32_t *)p; p += pre_b;
        f.ego = (double *)p; p += ego_b;
        f.scen = (int32_t *)p;
        return f;
    }
};

// one lock step of the running slots `sel`; step k of the call (outputs row k)
int loop_run_step(fot_handle *h, const std::vector<int32_t> &sel, int k, fot_loop_run_out *out, double *d_hist_step)
{
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    LoopEpisodes &E = L.ep;
    const fot_loop_replay &C = R.cfg;
    hipStream_t st = h->stream;
    const int n = (int)sel.size(), n_slots = C.n_slots;
    { int r = order_begin(h, st); if (r != FOT_OK) return r; }
    L.stepped = true;
    // --- 1. pedestrians + observer
    R.clock.advance();
    const bool ready = R.clock.ready();
    const int f_cur = R.clock.frame, f_last = R.clock.last_frame(), f_prev = R.clock.prev_frame();
    const double stale = R.clock.staleness();
    if (out->frame) out->frame[k] = f_cur;
    if (out->obs_last_frame) out->obs_last_frame[k] = f_last;
    if (out->obs_prev_frame) out->obs_prev_frame[k] = f_prev;
    if (out->staleness) out->staleness[k] = stale;
    // --- 2. the frame of the running episodes: tables on the host, pedestrians on the device
    const FrameLayout FL((size_t)n_slots, (size_t)R.n_cols);
    const FrameLayout::Stage sg = FL.stage(R.hStage.p);
    StepWork W;
    step_level0(E, sel.data(), n, W);
    L.frame_scen.clear();
    if (E.scenarios) L.frame_scen.resize((size_t)n);
    L.ped_off.assign((size_t)n + 1, 0); L.blk_off.assign((size_t)n + 1, 0); L.t_len.assign((size_t)n, 1);
    L.dist_S = 0;
    L.rep.frame = false;
    L.sweep_tab.clear();
    const size_t row_doubles = 2 * (size_t)R.n_cols;
    int rows_run = 0;
    for (int i = 0; i < n; ++i) rows_run += R.ped_off[sel[i] + 1] - R.ped_off[sel[i]];
    const int dist_S = R.dist_S();
    const bool sampled = dist_S > 0 && ready && rows_run > 0;    // this step predicts with the sampler or the recording
    // fot_loop_set_slot_samples: every running episode on its slot's own count; S_move: what the gather or the sampler
    // moves or draws (the largest count among the loop's slots), S_run / P_run: the grid of the ragged resample.  A step
    // whose running slots all keep the source's count is the step of before.
    L.ep_S.clear();
    bool ragged = false;
    int S_move = dist_S, S_run = dist_S, P_run = 0;
    if (sampled && E.sweep && !L.slot_S.empty()) {
        S_move = *std::max_element(L.slot_S.begin(), L.slot_S.end());
        for (int i = 0; i < n; ++i) ragged = ragged || L.slot_S[(size_t)sel[i]] != dist_S;
        if (ragged) {
            L.ep_S.resize((size_t)n);
            S_run = sweep_slot_counts(n, sel.data(), L.slot_S.data(), L.ep_S.data());
            std::memcpy(L.hEpS.p, L.ep_S.data(), sizeof(int32_t) * (size_t)n);
        } else S_move = dist_S;
    }
    const int32_t *ep_S = (const int32_t *)L.hEpS.p;
    R.smp.last_scenes = R.smp.last_rows = 0;                     // (fot_debug_loop_sampler_shape: until the sampler branch runs)
    std::fill(R.smp.last_mscenes.begin(), R.smp.last_mscenes.end(), 0);
    std::fill(R.smp.last_mrows.begin(), R.smp.last_mrows.end(), 0);
    for (int i = 0; i < n; ++i) {
        const int e = sel[i], c0 = R.ped_off[e], P_e = R.ped_off[e + 1] - c0, nf = R.n_frames[e];
        int pre = 0;
        if (!sampled && ready && f_prev >= 0 && P_e > 0) {
            const double *cur = R.pos.data() + (size_t)replay_row(f_cur, nf) * row_doubles + 2 * (size_t)c0;
            const double *last = R.pos.data() + (size_t)replay_row(f_last, nf) * row_doubles + 2 * (size_t)c0;
            const double *prev = R.pos.data() + (size_t)replay_row(f_prev, nf) * row_doubles + 2 * (size_t)c0;
            pre = replay_prepend(P_e, last, prev, cur, C.rp.sgan_dt, C.rp.sim_dt, stale) ? 1 : 0;
        }
        if (sampled) pre = 1;                                    // (the current positions lead EVERY sample, :514-525)
        L.t_len[i] = ready ? R.n_dense + pre : 1;
        L.ped_off[i + 1] = L.ped_off[i] + P_e;
        L.blk_off[i + 1] = L.blk_off[i] + (int64_t)(sampled ? (ragged ? L.ep_S[(size_t)i] : dist_S) : 1) * P_e * L.t_len[i];
        P_run = std::max(P_run, P_e);
        sg.slot[i] = e; sg.ped0[i] = L.ped_off[i]; sg.blk[i] = L.blk_off[i]; sg.prepend[i] = pre;
        if (E.scenarios) sg.scen[i] = L.frame_scen[(size_t)i] = E.scen[(size_t)e];
        for (int q = 0; q < 4; ++q) sg.ego[4 * (size_t)i + q] = W.ego4[4 * (size_t)i + q];
    }
    sg.ped0[n] = L.ped_off[n]; sg.blk[n] = L.blk_off[n];
    const int rows = L.ped_off[n];
    ReplayView rv;
    rv.pos = R.dPos.as<double>(); rv.vel = R.dVel.as<double>();
    rv.slot_ped0 = R.dTab.as<int32_t>(); rv.slot_frames = R.dTab.as<int32_t>() + (n_slots + 1);
    rv.n_cols = R.n_cols;
    FrameStage fs;
    fs.slot = sg.slot; fs.ped0 = sg.ped0; fs.blk = sg.blk; fs.prepend = sg.prepend; fs.ego = sg.ego;
    fs.scen = E.scenarios ? sg.scen : nullptr;
    const FrameDev fd = FL.dev(R.dFrame.p);
    LAUNCH_TRY(h, launch_loop_frame(rv, fs, fd, n, f_cur, ready ? f_last : -1, ready ? f_prev : -1, st));
    L.p_off = fd.ped0; L.p_pos = fd.pos; L.p_vel = fd.vel;
    L.p_scen = E.scenarios ? fd.scen : nullptr;
    L.ego_radius = C.ego_radius; L.ped_radius = C.ped_radius; L.use_footprint = C.use_footprint;
    L.dyn_ptr = fd.pos;                                          // not ready: the current positions, T = 1
    if (sampled && R.rec.on) {
        // row k - first_step of the recording -> the step's raw samples of the running slots -> every episode's
        // [S][P_e][n_dense + 1][2] block, all in HBM behind k_loop_frame (fot_loop_run has checked that the row exists)
        LoopSamples &M = R.rec;
        if (M.sel != sel) {                                      // a slot dropped out (or the first step): the row -> column table
            int32_t *col = (int32_t *)M.hCol.p;                  // (no copy of an earlier step still reads it: every step ends
            sweep_fill_columns(n, L.ped_off.data(), sel.data(), M.slot_col0.data(), col);    //  with the host waiting for its word)
            HIP_TRY(h, hipMemcpyAsync(M.dCol.p, col, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, st));
            M.sel = sel;
        }
        LoopSampleRows a{};
        a.d.S = M.S; a.d.pred_len = C.pred_len; a.d.rows = rows; a.d.n_cols = M.n_rec_cols;
        a.d.rec_row = (int64_t)R.steps[(size_t)sel[0]] - M.first_step;
        a.rec = M.rec; a.col = M.dCol.as<int32_t>(); a.out = M.dRaw.p; a.dtype = M.dtype;
        if (ragged) {                                            // (the largest count's samples only)
            a.d.S = S_move;
            LAUNCH_TRY(h, launch_loop_sample_rows_prefix(a, M.S, st));
        } else
            LAUNCH_TRY(h, launch_loop_sample_rows(a, st));
        L.dyn_ptr = L.dDyn.p;
        L.dist_S = M.S;
        if (ragged)
            LAUNCH_TRY(h, launch_resample_slots(C.rp.sgan_dt, C.rp.sim_dt, stale, S_run, C.pred_len, rows, R.n_dense, n, P_run, M.dRaw.p,
                                                M.dtype, fd.last, fd.pos, L.dDyn.as<double>(), fd.ped0, fd.blk, ep_S, st));
        else
            LAUNCH_TRY(h, launch_resample(C.rp.sgan_dt, C.rp.sim_dt, stale, M.S, C.pred_len, rows, R.n_dense, 1, 1, 0, M.dRaw.p,
                                          M.dtype, fd.last, fd.pos, L.dDyn.p, FOT_F64, 0, st, fd.ped_ep, fd.ped0, fd.blk));
    } else if (sampled && R.smp.models) {
        // One sampling per ACTIVE (CROWD, MODEL) UNIT (fot_loop_set_sampler_models): for every model with an active unit, in
        // ascending id, window -> noise keyed by the crowd -> samples of its units' representatives into its
        // own raw tensor; then ONE gather of all of them into the step's raw tensor of the running episodes -> the blocks
        LoopSampler &M = R.smp;
        const size_t ns = (size_t)std::max(n_slots, 1), N = std::max<size_t>((size_t)R.n_cols, 1), nm = (size_t)M.n_models;
        int32_t *t_off = (int32_t *)M.hCrowdTab.p, *t_rep = t_off + nm * (ns + 1), *t_scene = t_rep + nm * ns;
        const int32_t *d_off = M.dCrowdTab.as<int32_t>(), *d_rep = d_off + nm * (ns + 1), *d_scene = d_rep + nm * ns;
        const size_t raw_stride = (size_t)M.S * (size_t)C.pred_len * N;     // elements of two coordinates of a model's raw tensor
        if (M.sel != sel) {                                      // a slot dropped out (or the first step); no copy of an earlier
            int64_t base[SGAN_MAX_MODELS];                       // step still reads the tables (as LoopSamples::hCol)
            for (size_t m = 0; m < nm; ++m) base[m] = (int64_t)(m * raw_stride);
            sweep_model_tables(n, L.ped_off.data(), sel.data(), M.slot_crowd.data(), M.slot_model.data(), M.n_models, (int32_t)ns,
                               (int32_t)N, M.mshape.data(), t_off, t_scene, t_rep, M.mscene_crowd.data(), M.row_model.data(),
                               M.row_col.data());
            sweep_model_rows(rows, M.row_model.data(), M.row_col.data(), M.mshape.data(), base, (ModelRow *)M.hModelTab.p);
            HIP_TRY(h, hipMemcpyAsync(M.dCrowdTab.p, M.hCrowdTab.p, sizeof(int32_t) * nm * ((ns + 1) + ns + N), hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(M.dModelTab.p, M.hModelTab.p, sizeof(ModelRow) * (size_t)rows, hipMemcpyHostToDevice, st));
            M.sel = sel;
        }
        const size_t win_stride = 2 * (size_t)C.obs_len * N, tab_stride = 3 * (N + ns);
        const size_t noise_stride = M.noise_stride;                         // (sized by the set call for the widest model)
        int n_active = 0;
        for (int m = 0; m < M.n_models; ++m) n_active += M.mshape[(size_t)m].n_scenes > 0;
        // The first active model samples on the loop's stream, every later one on a side stream of its own, forked from the
        // loop's stream behind the frame and the tables and joined to it in front of the gather by events: their scratch is
        // separate, nothing waits on the host (profiles/r24_model_sweep.json: 0.69 against 0.75 ms per lock step)
        const bool side = M.side_on && n_active > 1;
        if (side) HIP_TRY(h, hipEventRecord(M.fork, st));
        int i_active = 0;
        for (int m = 0; m < M.n_models; ++m) {
            const int n_sc = M.mshape[(size_t)m].n_scenes, m_rows = M.mshape[(size_t)m].rows;
            if (n_sc == 0) continue;                             // no active unit: nothing is launched for it
            hipStream_t ms = side && i_active > 0 ? M.side[m] : st;   // the stream model m samples on
            if (ms != st) HIP_TRY(h, hipStreamWaitEvent(ms, M.fork, 0));
            ++i_active;
            if (m_rows > rows || n_sc > n) return fail(h, FOT_ERR_INVALID, "internal: a model's tables exceed the frame");
            const fot_sgan_desc &d = h->sgan[m].desc;
            const bool global_noise = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL;
            const int nd = d.noise_dim, noise_rows = global_noise ? n_sc : m_rows;
            const int32_t *m_off = t_off + (size_t)m * (ns + 1), *m_rep = t_rep + (size_t)m * ns, *m_crowd = M.mscene_crowd.data() + (size_t)m * ns;
            const int32_t *dm_off = d_off + (size_t)m * (ns + 1), *dm_rep = d_rep + (size_t)m * ns, *dm_scene = d_scene + (size_t)m * N;
            float *win = M.dWin.as<float>() + (size_t)m * win_stride, *noise = M.dNoise.as<float>() + (size_t)m * noise_stride;
            if ((size_t)M.S * (size_t)noise_rows * (size_t)nd > noise_stride) return fail(h, FOT_ERR_INVALID, "internal: a model's noise exceeds its block");
            SgWindow w{};
            w.pos = rv.pos; w.slot_ped0 = rv.slot_ped0; w.slot_frames = rv.slot_frames;
            w.ped_ep = dm_scene; w.ep_ped0 = dm_off; w.ep_slot = dm_rep;
            w.n_cols = R.n_cols; w.rows = m_rows; w.obs_len = d.obs_len;
            for (int j = 0; j < d.obs_len; ++j) w.frames.f[j] = R.clock.sample_frame[(size_t)j];
            w.out = win;
            LAUNCH_TRY(h, launch_sgan_window(w, ms));
            if (nd > 0) {
                const size_t cap = (size_t)R.n_cols + (size_t)n_slots;
                int32_t *t_slot = (int32_t *)M.hTab.p + (size_t)m * tab_stride, *t_step = t_slot + cap, *t_idx = t_step + cap;
                int r = 0;
                for (int c = 0; c < n_sc; ++c) {                 // (lock step: the representative's step is its unit's)
                    const int e = m_rep[c], P_c = m_off[c + 1] - m_off[c];
                    for (int p = 0; p < (global_noise ? 1 : P_c); ++p, ++r) { t_slot[r] = m_crowd[c]; t_step[r] = R.steps[(size_t)e]; t_idx[r] = p; }
                }
                SgNoise a{};
                a.seed = M.seed; a.kind = M.kinds[(size_t)m]; a.S = S_move; a.rows = noise_rows; a.nd = nd; a.n_blk = (nd + 3) / 4;
                a.slot = t_slot; a.step = t_step; a.index = t_idx; a.out = (uint32_t *)noise;
                LAUNCH_TRY(h, launch_sgan_noise(a, ms));
            }
            { int r = sgan_enqueue(h, m, n_sc, m_rows, S_move, dm_off, global_noise && nd > 0 ? dm_scene : nullptr, win, noise,
                                   M.dCrowdRaw.as<float>() + 2 * (size_t)m * raw_stride, ms); if (r != FOT_OK) return r; }
            M.last_mscenes[(size_t)m] = n_sc; M.last_mrows[(size_t)m] = m_rows;
            M.last_scenes += n_sc; M.last_rows += m_rows;
            if (ms != st) {
                HIP_TRY(h, hipEventRecord(M.join[m], ms));
                HIP_TRY(h, hipStreamWaitEvent(st, M.join[m], 0));
            }
        }
        LoopModelRows g{};
        g.S = S_move; g.pred_len = C.pred_len; g.rows = rows;
        g.pool = (const float2 *)M.dCrowdRaw.p; g.tab = M.dModelTab.as<ModelRow>(); g.out = (float2 *)M.dRaw.p;
        LAUNCH_TRY(h, launch_loop_model_rows(g, st));
        L.dyn_ptr = L.dDyn.p;
        L.dist_S = M.S;
        if (ragged)
            LAUNCH_TRY(h, launch_resample_slots(C.rp.sgan_dt, C.rp.sim_dt, stale, S_run, C.pred_len, rows, R.n_dense, n, P_run, M.dRaw.p,
                                                FOT_F32, fd.last, fd.pos, L.dDyn.as<double>(), fd.ped0, fd.blk, ep_S, st));
        else
            LAUNCH_TRY(h, launch_resample(C.rp.sgan_dt, C.rp.sim_dt, stale, M.S, C.pred_len, rows, R.n_dense, 1, 1, 0, M.dRaw.p,
                                          FOT_F32, fd.last, fd.pos, L.dDyn.p, FOT_F64, 0, st, fd.ped_ep, fd.ped0, fd.blk));
    } else if (sampled && R.smp.crowds) {
        // One sampling per ACTIVE CROWD (fot_loop_set_sampler_shared): window -> noise keyed by the crowd -> samples of the
        // crowds' representatives -> gathered into the step's raw tensor of the running episodes -> every episode's block
        LoopSampler &M = R.smp;
        const fot_sgan_desc &d = h->sgan[0].desc;
        const bool global_noise = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL;
        const int nd = d.noise_dim;
        const size_t ns = (size_t)std::max(n_slots, 1), N = std::max<size_t>((size_t)R.n_cols, 1);
        int32_t *t_off = (int32_t *)M.hCrowdTab.p, *t_rep = t_off + (ns + 1), *t_scene = t_rep + ns, *t_col = t_scene + N;
        const int32_t *d_off = M.dCrowdTab.as<int32_t>(), *d_rep = d_off + (ns + 1), *d_scene = d_rep + ns, *d_col = d_scene + N;
        if (M.sel != sel) {                                      // a slot dropped out (or the first step); no copy of an earlier
            M.scene_slot.assign((size_t)n, -1);                  // step still reads the tables (as LoopSamples::hCol)
            M.scene_crowd.assign((size_t)n, -1);
            M.shape = sweep_crowd_tables(n, L.ped_off.data(), sel.data(), M.slot_crowd.data(), t_off, t_scene, M.scene_slot.data(),
                                         M.scene_crowd.data(), t_col);
            for (int c = 0; c < M.shape.n_scenes; ++c) t_rep[c] = M.scene_slot[(size_t)c];
            HIP_TRY(h, hipMemcpyAsync(M.dCrowdTab.p, M.hCrowdTab.p, sizeof(int32_t) * ((ns + 1) + ns + 2 * N), hipMemcpyHostToDevice, st));
            M.sel = sel;
        }
        const int n_sc = M.shape.n_scenes, c_rows = M.shape.crowd_rows, noise_rows = global_noise ? n_sc : c_rows;
        if (c_rows > rows || n_sc > n) return fail(h, FOT_ERR_INVALID, "internal: the crowds' tables exceed the frame");
        float *crowd_raw = M.shape.identity ? M.dRaw.as<float>() : M.dCrowdRaw.as<float>();
        SgWindow w{};
        w.pos = rv.pos; w.slot_ped0 = rv.slot_ped0; w.slot_frames = rv.slot_frames;
        w.ped_ep = d_scene; w.ep_ped0 = d_off; w.ep_slot = d_rep;
        w.n_cols = R.n_cols; w.rows = c_rows; w.obs_len = d.obs_len;
        for (int j = 0; j < d.obs_len; ++j) w.frames.f[j] = R.clock.sample_frame[(size_t)j];
        w.out = M.dWin.as<float>();
        LAUNCH_TRY(h, launch_sgan_window(w, st));
        if (nd > 0) {
            const size_t cap = (size_t)R.n_cols + (size_t)n_slots;
            int32_t *t_slot = (int32_t *)M.hTab.p, *t_step = t_slot + cap, *t_idx = t_step + cap;
            int r = 0;
            for (int c = 0; c < n_sc; ++c) {                     // (the slots of a resident loop run in lock step: the
                const int e = M.scene_slot[(size_t)c], P_c = t_off[c + 1] - t_off[c];    //  representative's step is its crowd's)
                for (int p = 0; p < (global_noise ? 1 : P_c); ++p, ++r) { t_slot[r] = M.scene_crowd[(size_t)c]; t_step[r] = R.steps[(size_t)e]; t_idx[r] = p; }
            }
            SgNoise a{};
            a.seed = M.seed; a.kind = M.kind; a.S = S_move; a.rows = noise_rows; a.nd = nd; a.n_blk = (nd + 3) / 4;
            a.slot = t_slot; a.step = t_step; a.index = t_idx; a.out = (uint32_t *)M.dNoise.p;
            LAUNCH_TRY(h, launch_sgan_noise(a, st));
        }
        { int r = sgan_enqueue(h, 0, n_sc, c_rows, S_move, d_off, global_noise && nd > 0 ? d_scene : nullptr, M.dWin.as<float>(),
                               M.dNoise.as<float>(), crowd_raw, st); if (r != FOT_OK) return r; }
        if (!M.shape.identity) {                                 // (one slot per crowd, in the crowds' order: nothing to gather)
            LoopSampleRows a{};
            a.d.S = S_move; a.d.pred_len = C.pred_len; a.d.rows = rows; a.d.n_cols = c_rows; a.d.rec_row = 0;
            a.rec = crowd_raw; a.col = d_col; a.out = M.dRaw.p; a.dtype = FOT_F32;
            LAUNCH_TRY(h, launch_loop_sample_rows(a, st));
        }
        M.last_scenes = n_sc; M.last_rows = c_rows;
        L.dyn_ptr = L.dDyn.p;
        L.dist_S = M.S;
        if (ragged)
            LAUNCH_TRY(h, launch_resample_slots(C.rp.sgan_dt, C.rp.sim_dt, stale, S_run, C.pred_len, rows, R.n_dense, n, P_run, M.dRaw.p,
                                                FOT_F32, fd.last, fd.pos, L.dDyn.as<double>(), fd.ped0, fd.blk, ep_S, st));
        else
            LAUNCH_TRY(h, launch_resample(C.rp.sgan_dt, C.rp.sim_dt, stale, M.S, C.pred_len, rows, R.n_dense, 1, 1, 0, M.dRaw.p,
                                          FOT_F32, fd.last, fd.pos, L.dDyn.p, FOT_F64, 0, st, fd.ped_ep, fd.ped0, fd.blk));
    } else if (sampled) {
        // window -> noise -> samples -> every episode's [S][P_e][n_dense + 1][2] block, all in HBM behind k_loop_frame
        LoopSampler &M = R.smp;
        M.last_scenes = n; M.last_rows = rows;
        const fot_sgan_desc &d = h->sgan[0].desc;
        const bool global_noise = d.noise_mix_type == FOT_SGAN_NOISE_GLOBAL;
        const int nd = d.noise_dim, noise_rows = global_noise ? n : rows;
        SgWindow w{};
        w.pos = rv.pos; w.slot_ped0 = rv.slot_ped0; w.slot_frames = rv.slot_frames;
        w.ped_ep = fd.ped_ep; w.ep_ped0 = fd.ped0; w.ep_slot = sg.slot;
        w.n_cols = R.n_cols; w.rows = rows; w.obs_len = d.obs_len;
        for (int j = 0; j < d.obs_len; ++j) w.frames.f[j] = R.clock.sample_frame[(size_t)j];
        w.out = M.dWin.as<float>();
        LAUNCH_TRY(h, launch_sgan_window(w, st));
        if (nd > 0) {
            const size_t cap = (size_t)R.n_cols + (size_t)n_slots;
            int32_t *t_slot = (int32_t *)M.hTab.p, *t_step = t_slot + cap, *t_idx = t_step + cap;
            int r = 0;
            for (int i = 0; i < n; ++i) {
                const int e = sel[i], P_e = R.ped_off[e + 1] - R.ped_off[e];
                for (int p = 0; p < (global_noise ? 1 : P_e); ++p, ++r) { t_slot[r] = e; t_step[r] = R.steps[(size_t)e]; t_idx[r] = p; }
            }
            SgNoise a{};
            a.seed = M.seed; a.kind = M.kind; a.S = S_move; a.rows = noise_rows; a.nd = nd; a.n_blk = (nd + 3) / 4;
            a.slot = t_slot; a.step = t_step; a.index = t_idx; a.out = (uint32_t *)M.dNoise.p;
            LAUNCH_TRY(h, launch_sgan_noise(a, st));
        }
        { int r = sgan_enqueue(h, 0, n, rows, S_move, fd.ped0, global_noise && nd > 0 ? fd.ped_ep : nullptr, M.dWin.as<float>(),
                               M.dNoise.as<float>(), M.dRaw.as<float>(), st); if (r != FOT_OK) return r; }
        L.dyn_ptr = L.dDyn.p;
        L.dist_S = M.S;
        if (ragged)
            LAUNCH_TRY(h, launch_resample_slots(C.rp.sgan_dt, C.rp.sim_dt, stale, S_run, C.pred_len, rows, R.n_dense, n, P_run, M.dRaw.p,
                                                FOT_F32, fd.last, fd.pos, L.dDyn.as<double>(), fd.ped0, fd.blk, ep_S, st));
        else
            LAUNCH_TRY(h, launch_resample(C.rp.sgan_dt, C.rp.sim_dt, stale, M.S, C.pred_len, rows, R.n_dense, 1, 1, 0, M.dRaw.p,
                                          FOT_F32, fd.last, fd.pos, L.dDyn.p, FOT_F64, 0, st, fd.ped_ep, fd.ped0, fd.blk));
    } else if (ready && rows > 0) {
        L.dyn_ptr = L.dDyn.p;
        LAUNCH_TRY(h, launch_predict_cv_frame(C.rp.sgan_dt, C.rp.sim_dt, stale, rows, R.n_dense, fd, L.dDyn.as<double>(), st));
    }
    const bool scored = R.sc.on && sampled;                      // the step's distributions are scored where they lie
    const bool rep_on = L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE && sampled;   // ... the requests plan on one sample of each
    const bool sweep_on = E.sweep && sampled;                    // ... each in its slot's own mode
    if (sweep_on) {
        // the selection of the episodes that plan on their sample (of all, where the loop scores), into the scores' tables
        // where they are on; then the planning blocks, compacted behind the distribution blocks (fot_sweep.hpp)
        SweepEp *tab = (SweepEp *)L.hSweep.p;
        const int64_t pts = sweep_layout(n, L.ped_off.data(), sel.data(), E.plan_mode.data(), L.blk_off[n], R.n_dense + 1, R.sc.on, tab);
        if (sizeof(double) * 2 * (size_t)pts > L.dDyn.cap) return fail(h, FOT_ERR_INVALID, "internal: the sweep's tensor is too small");
        int32_t *best_tab = R.sc.on ? R.sc.dBest.as<int32_t>() : L.rep.dBest.as<int32_t>();
        bool any_select = false;                                 // (every running slot in distribution mode, no scores: no launch)
        for (int i = 0; i < n; ++i) any_select = any_select || tab[i].select != 0;
        if (any_select && ragged)                                // (the tables' rows were sized for the source's S)
            LAUNCH_TRY(h, launch_loop_best_sample_slots(sg.slot, fd, L.dDyn.as<double>(), tab, ep_S, n, S_run, R.n_dense,
                                                        R.sc.on ? R.sc.dDev.as<double>() : L.rep.dDev.as<double>(),
                                                        best_dev_stride(dist_S), best_tab,
                                                        (int32_t *)(R.sc.on ? R.sc.hBest.p : L.rep.hBest.p), st));
        else if (any_select)
            LAUNCH_TRY(h, launch_loop_best_sample_sweep(sg.slot, fd, L.dDyn.as<double>(), tab, n, dist_S, R.n_dense,
                                                        R.sc.on ? R.sc.dDev.as<double>() : L.rep.dDev.as<double>(), best_tab,
                                                        (int32_t *)(R.sc.on ? R.sc.hBest.p : L.rep.hBest.p), st));
        if (pts > L.blk_off[n] && ragged)
            LAUNCH_TRY(h, launch_loop_rep_block_slots(sg.slot, fd, L.dDyn.as<double>(), tab, ep_S, best_tab, n, R.n_dense,
                                                      L.dDyn.as<double>(), L.rep.dPre.as<int32_t>(), (int32_t *)L.rep.hPre.p, st));
        else if (pts > L.blk_off[n])                             // (some running episode has a planning block to write)
            LAUNCH_TRY(h, launch_loop_rep_block_sweep(sg.slot, fd, L.dDyn.as<double>(), tab, best_tab, n, dist_S, R.n_dense,
                                                      L.dDyn.as<double>(), L.rep.dPre.as<int32_t>(), (int32_t *)L.rep.hPre.p, st));
        L.sweep_tab.assign(tab, tab + n);
        L.sweep_T = R.n_dense + 1;
    } else if (rep_on) {
        // the selection once, into the scores' tables where they are on: a scored and a planning loop read the same choice
        { int r = rep_ensure(h, n_slots, n_slots, (size_t)R.n_cols, R.n_dense + 1, dist_S); if (r != FOT_OK) return r; }
        { int r = rep_enqueue(h, sg.slot, fd, n, dist_S, R.n_dense, R.sc.on ? R.sc.dDev.as<double>() : L.rep.dDev.as<double>(),
                              R.sc.on ? R.sc.dBest.as<int32_t>() : L.rep.dBest.as<int32_t>(),
                              (int32_t *)(R.sc.on ? R.sc.hBest.p : L.rep.hBest.p), st); if (r != FOT_OK) return r; }
        L.rep.frame = true; L.rep.T = R.n_dense + 1;
    } else if (scored)                                           // every episode's representative sample
        LAUNCH_TRY(h, launch_loop_best_sample(sg.slot, fd, L.dDyn.as<double>(), n, dist_S, R.n_dense, R.sc.dDev.as<double>(),
                                              R.sc.dBest.as<int32_t>(), (int32_t *)R.sc.hBest.p, st));
    if (R.sum.on || R.sc.on)                                     // this step's row of every running slot's ring
        LAUNCH_TRY(h, launch_loop_pred_error(rv, sg.slot, fd, L.dDyn.as<double>(), n, ready && rows > 0 ? 1 : 0, f_cur,
                                             R.steps[(size_t)sel[0]], R.sum.shape, R.sum.dRing.as<double>(),
                                             R.sum.dRingP.as<int32_t>(), R.sum.dTotals.as<SummaryTotals>(), st,
                                             scored ? R.sc.dBest.as<int32_t>() : nullptr));
    if (scored && R.sc.std_ok) {                                 // one origin per running episode, the truth from the recording
        PredOriginDev *pd = (PredOriginDev *)R.sc.hDesc.p;
        const double scott = ps_scott(dist_S);
        for (int i = 0; i < n; ++i) {                            // (a count per slot: the origin's own S and bandwidth factor)
            const int S_i = L.count_of((size_t)i);
            pd[i] = PredOriginDev{ L.blk_off[(size_t)i], (int64_t)L.ped_off[(size_t)i], ragged ? ps_scott(S_i) : scott, S_i,
                                   L.ped_off[(size_t)i + 1] - L.ped_off[(size_t)i], R.n_dense + 1, 0, 1, 0 };
        }
        LAUNCH_TRY(h, launch_loop_score_truth(rv, sg.slot, fd, rows, f_cur, R.sc.stride, C.pred_len, R.sc.dTruth.as<double>(), st));
        LAUNCH_TRY(h, launch_pred_scores(pd, n, L.dDyn.p, FOT_F64, R.sc.stride, C.pred_len, R.sc.dTruth.as<double>(),
                                         (fot_pred_score *)R.sc.hRec.p, st, S_run > FOT_MAX_SAMPLES ? 1 : 0));   // (wide: any running origin is)
    }
    LAUNCH_TRY(h, launch_safety(h->dP.as<DevParams>(), n, fd.ego, fd.ped0, fd.pos, fd.vel, L.ego_radius, L.ped_radius,
                                h->sc[0].params.footprint_radius, L.use_footprint, (fot_safety *)L.hOut.p, st,
                                L.p_scen, L.dSafScen.as<SafetyScen>()));
    L.have_frame = true; L.observe_n = -1;
    // --- 3. level 0 of every episode; the records stay in HBM, the host reads their digests
    fot_result *d_rec = R.dRec.as<fot_result>();
    LoopDigest *dig = (LoopDigest *)R.hDigest.p;
    int32_t *word = (int32_t *)R.hWord.p;
    { int rc = loop_enqueue_requests(h, n, W.req.data(), d_rec, st, false); if (rc != FOT_OK) return rc; }
    int32_t seq = next_seq(R);
    LAUNCH_TRY(h, launch_loop_digest(d_rec, n, dig, word, seq, st));
    { int rc = wait_word(h, word, seq, st); if (rc != FOT_OK) return rc; }
    std::memcpy(W.m.data(), L.hOut.p, sizeof(fot_safety) * (size_t)n);   // (k_safety ran ahead of the plan on this stream)
    if (R.sc.on) {                                               // ... and so did the step's scores: into the slots' rings
        LoopScores &Q = R.sc;
        const fot_pred_score *rec = (const fot_pred_score *)Q.hRec.p;
        const int32_t *best = (const int32_t *)Q.hBest.p;
        std::fill(Q.last_best.begin(), Q.last_best.end(), -1);
        for (int i = 0; i < n; ++i) {
            const int e = sel[i];
            // (no prediction, or no horizon that could ever complete; of the slot's own count)
            PredScoreTerms t = ps_zero(L.slot_S.empty() ? dist_S : L.slot_S[(size_t)e]);
            if (scored && Q.std_ok) {
                const fot_pred_score &r = rec[i];
                t.ade_scene = r.ade_scene; t.fde_scene = r.fde_scene; t.ade_agent_sum = r.ade_agent_sum;
                t.fde_agent_sum = r.fde_agent_sum; t.log_lik_sum = r.log_lik_sum;
                t.n_peds = r.n_peds; t.n_samples = r.n_samples; t.nll_count = r.nll_count; t.flags = r.flags;
            }
            score_ring_push(Q.fold[(size_t)e], Q.ring.data() + (size_t)e * (size_t)Q.H, Q.H, R.steps[(size_t)e], t);
            if (scored && L.ped_off[(size_t)i + 1] > L.ped_off[(size_t)i]) Q.last_best[(size_t)e] = best[e];
        }
    }
    if (E.sweep) {                                               // a slot's choice where it planned on it or the loop scores
        const int32_t *best = (const int32_t *)(R.sc.on ? R.sc.hBest.p : L.rep.hBest.p);
        std::fill(L.rep.last_best.begin(), L.rep.last_best.end(), -1);
        for (int i = 0; sweep_on && i < n; ++i)
            if (L.sweep_tab[(size_t)i].select && L.ped_off[(size_t)i + 1] > L.ped_off[(size_t)i]) L.rep.last_best[(size_t)sel[i]] = best[sel[i]];
        L.rep.run_best.insert(L.rep.run_best.end(), L.rep.last_best.begin(), L.rep.last_best.end());
    } else if (L.rep.mode == FOT_LOOP_PLAN_REPRESENTATIVE) {     // the choice the step planned on (fot_loop_last_best_sample)
        const int32_t *best = (const int32_t *)(R.sc.on ? R.sc.hBest.p : L.rep.hBest.p);
        std::fill(L.rep.last_best.begin(), L.rep.last_best.end(), -1);
        for (int i = 0; rep_on && i < n; ++i)
            if (L.ped_off[(size_t)i + 1] > L.ped_off[(size_t)i]) L.rep.last_best[(size_t)sel[i]] = best[sel[i]];
        L.rep.run_best.insert(L.rep.run_best.end(), L.rep.last_best.begin(), L.rep.last_best.end());
    }
    for (int i = 0; i < n; ++i) E.last_clearance[sel[i]] = W.m[i].clearance_ahead;
    step_escalations(E, sel.data(), n, dig, W);
    if (!W.more.empty()) {
        const int n_more = (int)W.more.size();
        int rc = loop_enqueue_requests(h, n_more, W.more.data(), d_rec + n, st, false);
        if (rc != FOT_OK) return rc;
        seq = next_seq(R);
        LAUNCH_TRY(h, launch_loop_digest(d_rec + n, n_more, dig + n, word, seq, st));
        rc = wait_word(h, word, seq, st);
        if (rc != FOT_OK) return rc;
    }
    // --- 4. retry loop, ego update; 5. metrics of the new states + the goal test's nearest point
    step_resolve(E, sel.data(), n, dig, W);
    std::vector<double> gps((size_t)n);
    for (int i = 0; i < n; ++i) gps[i] = E.goal_prev_s[sel[i]];
    { int rc = observe_begin_impl(h, n, W.ego5n.data(), gps.data(), sel.data()); if (rc != FOT_OK) return rc; }
    // the followed paths into the history block, and the word that tells the host the step's results are there
    int32_t *t_src = (int32_t *)R.hHistTab.p, *t_slot = t_src + n_slots;
    for (int i = 0; i < n; ++i) { t_src[i] = W.path_rec[i]; t_slot[i] = sel[i]; }
    seq = next_seq(R);
    LAUNCH_TRY(h, launch_loop_history(d_rec, n, t_src, t_slot, d_hist_step, n_slots, h->sc[0].P.n_total, word + 16, seq, st));
    { int rc = wait_word(h, word + 16, seq, st); if (rc != FOT_OK) return rc; }
    L.observe_n = -1;
    fpo_fold_step(L, sel.data(), n);
    const fot_safety *after = (const fot_safety *)L.hOut.p;
    const InstState *p_state = (const InstState *)((const char *)L.hOut.p + align256(sizeof(fot_safety) * (size_t)n));
    const size_t row = (size_t)k * (size_t)n_slots;
    if (out->followed) for (int e = 0; e < n_slots; ++e) out->followed[row + e] = -1;
    for (int i = 0; i < n; ++i) {
        const int e = sel[i];
        const size_t o = row + (size_t)e;
        const double s_now = p_state[i].new_prev_s;
        E.goal_prev_s[e] = s_now;
        if (out->ego) for (int q = 0; q < 5; ++q) out->ego[5 * o + q] = W.ego5n[5 * (size_t)i + q];
        if (out->jerk) out->jerk[o] = W.jerk[i];
        if (out->state) out->state[o] = E.state[e];
        if (out->stats) for (int q = 0; q < 8; ++q) out->stats[8 * o + q] = E.stats[8 * (size_t)e + q];
        if (out->followed) out->followed[o] = W.path_rec[i] >= 0 ? 1 : 0;
        if (out->keep) out->keep[o] = W.keep[i];
        if (out->cost) out->cost[o] = W.cost[i];
        if (out->after) out->after[o] = after[i];
        if (out->s_now) out->s_now[o] = s_now;
        R.steps[e] += 1;
        if (R.sum.on || R.sc.on) {                               // (calculate_aggregate_metrics, metrics.py:279-308)
            LoopSummaryAcc &A = R.sum;
            const double aj = std::fabs(W.jerk[i]), aa = std::fabs(W.ego5n[5 * (size_t)i + 4]), ttc = after[i].ttc;
            A.min_dist[e] = std::fmin(A.min_dist[e], after[i].min_distance);
            if (after[i].collision != 0) A.collisions[e] += 1;
            if (ttc > 0.0 && ttc != INFINITY && ttc < A.min_ttc[e]) A.min_ttc[e] = ttc;
            A.max_jerk[e] = std::fmax(A.max_jerk[e], aj); A.sum_jerk[e] += aj; A.sum_jerk2[e] += aj * aj;
            A.max_accel[e] = std::fmax(A.max_accel[e], aa); A.sum_accel[e] += aa;
        }
        // the goal of a scenario loop's slot: the end of its own scenario's path (its spline's last knot)
        const double s_end = E.scenarios ? h->sc[(size_t)E.scen[(size_t)e]].spline.s.back() : C.s_end;
        R.termination[e] = replay_termination(after[i].collision, s_end, s_now, C.goal_distance);
        if (R.termination[e] != 0) R.alive[e] = 0;
    }
    return FOT_OK;
}

// The prediction-error ring, its totals and the host's accumulators of a run that has not begun: allocated and zeroed
// (a row with count 0 contributes nothing).  Leaves LoopSummaryAcc::on as it is.
int summary_arm(fot_handle *h, int num_samples, int stride)
{
    LoopReplay &R = h->loop.replay;
    LoopSummaryAcc &A = R.sum;
    const size_t ns = (size_t)std::max(R.cfg.n_slots, 1), nd = (size_t)R.n_dense;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, A.dRing.ensure(sizeof(double) * ns * nd * nd));
    HIP_TRY(h, A.dRingP.ensure(sizeof(int32_t) * ns * nd));
    HIP_TRY(h, A.dTotals.ensure(sizeof(SummaryTotals) * ns));
    HIP_TRY(h, A.hOut.ensure(sizeof(fot_loop_summary) * ns));
    HIP_TRY(h, A.hSteps.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, hipMemsetAsync(A.dRing.p, 0, sizeof(double) * ns * nd * nd, h->stream));
    HIP_TRY(h, hipMemsetAsync(A.dRingP.p, 0, sizeof(int32_t) * ns * nd, h->stream));
    HIP_TRY(h, hipMemsetAsync(A.dTotals.p, 0, sizeof(SummaryTotals) * ns, h->stream));
    A.shape = summary_shape(R.n_dense, stride, R.cfg.pred_len);
    A.num_samples = num_samples;
    A.min_dist.assign(ns, INFINITY); A.min_ttc.assign(ns, INFINITY);
    A.max_jerk.assign(ns, 0.0); A.sum_jerk.assign(ns, 0.0); A.sum_jerk2.assign(ns, 0.0);
    A.max_accel.assign(ns, 0.0); A.sum_accel.assign(ns, 0.0); A.collisions.assign(ns, 0);
    return FOT_OK;
}

// one record per slot from the ring, its totals and the host's accumulators (n_slots > 0, checked by the caller)
int summaries_fill(fot_handle *h, int32_t n_slots, fot_loop_summary *out)
{
    LoopReplay &R = h->loop.replay;
    LoopSummaryAcc &A = R.sum;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int32_t *steps = (int32_t *)A.hSteps.p;
    fot_loop_summary *rec = (fot_loop_summary *)A.hOut.p;
    for (int e = 0; e < n_slots; ++e) steps[e] = R.steps[(size_t)e];
    // totals + the ring's rows with their truncated horizons -> the prediction-error keys; nothing in HBM changes
    LAUNCH_TRY(h, launch_loop_summary(A.shape, A.dRing.as<double>(), A.dRingP.as<int32_t>(), A.dTotals.as<SummaryTotals>(),
                                      steps, n_slots, A.num_samples, rec, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const double dt = R.cfg.rp.sim_dt;
    for (int e = 0; e < n_slots; ++e) {
        fot_loop_summary s = rec[e];
        const int L = R.steps[(size_t)e];
        // an empty history: the reference's values (metrics.py:301-308)
        s.min_dist = L > 0 ? A.min_dist[e] : 0.0;
        s.min_ttc = A.min_ttc[e];
        s.collision_count = A.collisions[e];
        s.max_jerk = A.max_jerk[e]; s.max_accel = A.max_accel[e];
        s.mean_jerk = L > 0 ? A.sum_jerk[e] / (double)L : 0.0;
        s.rms_jerk = L > 0 ? std::sqrt(A.sum_jerk2[e] / (double)L) : 0.0;
        s.mean_accel = L > 0 ? A.sum_accel[e] / (double)L : 0.0;
        s.steps = L; s.termination = R.termination[(size_t)e]; s._pad = 0;
        s.total_time = (double)L * dt;
        out[e] = s;
    }
    return FOT_OK;
}

// fot_loop_set_samples / fot_loop_set_samples_shared (who: the entry's name, for the messages); slot_col0 == nullptr: the
// recording's columns are the replay's own
int set_samples_impl(fot_handle *h, const std::string &who, int32_t S, int32_t n_steps, int32_t first_step, const void *samples,
                     int32_t dtype, int32_t flags, bool shared, int32_t n_rec_cols, const int32_t *slot_col0)
{
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, who + ": fot_loop_set_replay comes first");
    if (R.smp.on) return fail(h, FOT_ERR_INVALID, who + ": a sampler is set (fot_loop_set_sampler): one predictor per run");
    const int n = R.cfg.n_slots;
    bool begun = R.clock.frame != R.cfg.warmup_frames;
    for (int e = 0; e < n; ++e) begun = begun || R.steps[(size_t)e] != 0;
    if (begun) return fail(h, FOT_ERR_INVALID, who + ": the run has begun (set it between fot_loop_set_replay and the first step)");
    if (S < 1) return fail(h, FOT_ERR_INVALID, who + ": S < 1");
    if (n_steps < 1 || first_step < 0) return fail(h, FOT_ERR_INVALID, who + ": n_steps < 1 / first_step < 0");
    if (!samples) return fail(h, FOT_ERR_INVALID, who + ": samples is NULL");
    if (dtype != FOT_F32 && dtype != FOT_F64) return fail(h, FOT_ERR_INVALID, who + ": dtype is FOT_F32 or FOT_F64");
    if (flags & ~FOT_OUT_DEVICE) return fail(h, FOT_ERR_INVALID, who + ": flags");
    const size_t elem = dtype == FOT_F32 ? 2 * sizeof(float) : 2 * sizeof(double);
    // (the gather moves whole elements of two coordinates; hipMalloc allocations and their slices along any axis
    //  but the last are aligned to one)
    if ((flags & FOT_OUT_DEVICE) && (uintptr_t)samples % elem != 0)
        return fail(h, FOT_ERR_INVALID, who + ": device samples must be aligned to one [x, y] element");
    if (S > h->sample_cap) return refuse_samples(h, who + ": ", S);
    if (L.ep.scenarios && !L.ep.sweep) return fail(h, FOT_ERR_UNSUPPORTED, who + ": a scenario loop plans against no distribution");
    if (R.sum.on) return fail(h, FOT_ERR_UNSUPPORTED, who + ": summaries are enabled (their prediction-error ring reads the constant-velocity tensor)");
    if (shared) {
        if (!slot_col0) return fail(h, FOT_ERR_INVALID, who + ": slot_col0 is NULL");
        if (R.n_cols > 0 && n_rec_cols < 1) return fail(h, FOT_ERR_INVALID, who + ": n_rec_cols < 1");
        if (!sweep_columns_fit(n, R.ped_off.data(), slot_col0, n_rec_cols))
            return fail(h, FOT_ERR_INVALID, who + ": a slot's columns (slot_col0[e] .. slot_col0[e] + P_e) lie outside the recording's n_rec_cols");
    } else {
        n_rec_cols = R.n_cols; slot_col0 = R.ped_off.data();
    }
    // --- accepted: everything a step needs is allocated here, so that no block grows (and moves) inside a run
    LoopSamples &M = R.rec;
    const size_t N = std::max<size_t>((size_t)R.n_cols, 1), rows = (size_t)S * N;
    const size_t rec_bytes = (size_t)sr_rec_elems(n_steps, S, R.cfg.pred_len, n_rec_cols) * elem;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    M.on = false; M.rec = nullptr;
    HIP_TRY(h, M.dRaw.ensure(elem * (size_t)S * (size_t)R.cfg.pred_len * N));
    HIP_TRY(h, M.dCol.ensure(sizeof(int32_t) * N));
    HIP_TRY(h, M.hCol.ensure(sizeof(int32_t) * N));
    HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * rows * (size_t)(R.n_dense + 1)));
    if (L.ep.sweep) { int r = sweep_ensure(h, S); if (r != FOT_OK) return r; }
    if (flags & FOT_OUT_DEVICE) {
        M.rec = samples;                                         // used in place, never written
    } else {
        HIP_TRY(h, M.dRec.ensure(std::max<size_t>(rec_bytes, elem)));
        if (rec_bytes) HIP_TRY(h, hipMemcpy(M.dRec.p, samples, rec_bytes, hipMemcpyHostToDevice));
        M.rec = M.dRec.p;
    }
    M.S = S; M.n_steps = n_steps; M.first_step = first_step; M.dtype = dtype;
    M.n_rec_cols = n_rec_cols; M.slot_col0.assign(slot_col0, slot_col0 + n);
    M.sel.clear();
    M.on = true;
    R.sc.on = false;                                             // (a new recording: its scores are enabled again, if wanted)
    L.slot_S.clear(); L.ep_S.clear();                            // ... and the slots' sample counts set anew
    return FOT_OK;
}

// what a sampler step of the resident loop needs of model `model`'s own work arrays, for S samples of up to N pedestrians
int sampler_model_scratch(fot_handle *h, int model, size_t S, size_t N)
{
    fot_handle::Sgan &G = h->sgan[model];
    const fot_sgan_desc &d = G.desc;
    const size_t rows = S * N;
    const int bp = sg_pooled(d) ? G.dev.pool.b_pad : 0;
    HIP_TRY(h, G.dHenc.ensure(sizeof(float) * N * (size_t)d.encoder_h_dim));
    if (bp > 0) HIP_TRY(h, G.dPool.ensure(sizeof(float) * (sg_pool_steps(d) ? rows : N) * (size_t)bp));
    if (sg_has_context(d)) HIP_TRY(h, G.dCtx.ensure(sizeof(float) * N * (size_t)std::max(d.decoder_h_dim - d.noise_dim, 1)));
    if (sg_pool_steps(d)) {
        HIP_TRY(h, G.dH.ensure(sizeof(float) * rows * (size_t)d.decoder_h_dim));
        HIP_TRY(h, G.dC.ensure(sizeof(float) * rows * (size_t)d.decoder_h_dim));
        HIP_TRY(h, G.dXY.ensure(sizeof(float) * rows * 6));
    }
    return FOT_OK;
}

// fot_loop_set_sampler / fot_loop_set_sampler_shared / fot_loop_set_sampler_models (who: the entry's name, for the messages).
// slot_crowd == nullptr: slot e is crowd e.  slot_model == nullptr (the first two entries): one model, the handle's model 0,
// of kind model_kind[0]; otherwise the third entry, whose slots name their models.
int set_sampler_impl(fot_handle *h, const std::string &who, int32_t S, uint64_t seed, int32_t n_models, const int32_t *model_kind,
                     bool shared, int32_t n_crowds, const int32_t *slot_crowd, bool by_model, const int32_t *slot_model)
{
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, who + ": fot_loop_set_replay comes first");
    bool used[SGAN_MAX_MODELS] = { false };                      // the models some slot names
    if (by_model) {
        if (!slot_model || !model_kind) return fail(h, FOT_ERR_INVALID, who + ": slot_model / model_kind is NULL");
        if (n_models < 1 || n_models > SGAN_MAX_MODELS) return fail(h, FOT_ERR_INVALID, who + ": n_models lies outside 1 .. fot_sgan_max_models()");
        for (int e = 0; e < R.cfg.n_slots; ++e) {
            if (slot_model[e] < 0 || slot_model[e] >= n_models)
                return fail(h, FOT_ERR_INVALID, who + ": slot_model[" + std::to_string(e) + "] lies outside 0 .. n_models - 1");
            if (!h->sgan[slot_model[e]].loaded)
                return fail(h, FOT_ERR_INVALID, who + ": slot " + std::to_string(e) + " names model " + std::to_string(slot_model[e]) +
                                                ", which is not loaded (fot_sgan_load_model)");
            used[slot_model[e]] = true;
        }
        if (n_models == 1 && !h->sgan[0].loaded) return fail(h, FOT_ERR_INVALID, who + ": model 0 is not loaded (fot_sgan_load_model)");
    } else {
        if (!h->sgan[0].loaded) return fail(h, FOT_ERR_INVALID, who + ": no model loaded (fot_sgan_load)");
    }
    if (n_models == 1) used[0] = true;                           // (a loop that names one model: the shared entry's step)
    if (R.rec.on) return fail(h, FOT_ERR_INVALID, who + ": recorded samples are set (fot_loop_set_samples): one predictor per run");
    const int n = R.cfg.n_slots;
    bool begun = R.clock.frame != R.cfg.warmup_frames;
    for (int e = 0; e < n; ++e) begun = begun || R.steps[(size_t)e] != 0;
    if (begun) return fail(h, FOT_ERR_INVALID, who + ": the run has begun (set it between fot_loop_set_replay and the first step)");
    if (S < 1) return fail(h, FOT_ERR_INVALID, who + ": S < 1");
    for (int m = 0; m < n_models; ++m)
        if (model_kind[m] != FOT_NOISE_GAUSSIAN && model_kind[m] != FOT_NOISE_UNIFORM_SYM)
            return fail(h, FOT_ERR_INVALID, who + ": kind is FOT_NOISE_GAUSSIAN or FOT_NOISE_UNIFORM_SYM");
    for (int m = 0; m < n_models; ++m)
        if (used[m] && (h->sgan[m].desc.obs_len != R.cfg.obs_len || h->sgan[m].desc.pred_len != R.cfg.pred_len))
            return fail(h, FOT_ERR_INVALID, who + ": the model's obs_len / pred_len differ from the replay's" +
                                            (by_model ? " (model " + std::to_string(m) + ")" : ""));
    if (S > h->sample_cap) return refuse_samples(h, who + ": ", S);
    for (int e = 0; e < n; ++e)
        if (R.ped_off[(size_t)e + 1] - R.ped_off[(size_t)e] > FOT_SGAN_MAX_PEDS)
            return fail(h, FOT_ERR_UNSUPPORTED, who + ": a slot of more than FOT_SGAN_MAX_PEDS pedestrians");
    if (L.ep.scenarios && !L.ep.sweep) return fail(h, FOT_ERR_UNSUPPORTED, who + ": a scenario loop plans against no distribution");
    if (R.sum.on) return fail(h, FOT_ERR_UNSUPPORTED, who + ": summaries are enabled (their prediction-error ring reads the constant-velocity tensor)");
    bool crowds = false;                                         // some slot is not the crowd of its own number
    if (shared) {
        if (!slot_crowd || n_crowds < 1) return fail(h, FOT_ERR_INVALID, who + ": slot_crowd is NULL / n_crowds < 1");
        for (int e = 0; e < n; ++e) {
            if (slot_crowd[e] < 0 || slot_crowd[e] >= n_crowds)
                return fail(h, FOT_ERR_INVALID, who + ": slot_crowd[" + std::to_string(e) + "] lies outside 0 .. n_crowds - 1");
            crowds = crowds || slot_crowd[e] != e;
        }
        // the slots of a crowd replay the same pedestrians: one comparison of their column ranges over the recorded frames
        int32_t a = 0, b = 0;
        const int differ = crowds ? sweep_crowds_consistent(n, R.ped_off.data(), R.n_frames.data(), slot_crowd, R.pos.data(), R.n_cols, &a, &b) : 0;
        if (differ != 0)
            return fail(h, FOT_ERR_INVALID, who + ": slots " + std::to_string(a) + " and " + std::to_string(b) + " of crowd " +
                                            std::to_string(slot_crowd[b]) + " differ in " +
                                            (differ == 1 ? "their pedestrian counts" : differ == 2 ? "n_frames" : "the recorded positions (pos)"));
    }
    // --- accepted: everything a step needs is allocated here, so that no block grows (and moves) inside a run
    LoopSampler &M = R.smp;
    const size_t N = std::max<size_t>((size_t)R.n_cols, 1), rows = (size_t)S * N, ns = (size_t)std::max(n, 1);
    const bool models = n_models > 1;                            // (one model: the shared entry's step on model 0, nothing new)
    const size_t nm = (size_t)n_models, obs_len = (size_t)R.cfg.obs_len, pred_len = (size_t)R.cfg.pred_len;
    int nd_max = 1;
    for (int m = 0; m < n_models; ++m)
        if (used[m]) nd_max = std::max(nd_max, h->sgan[m].desc.noise_dim);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    M.on = false;
    HIP_TRY(h, M.dWin.ensure(sizeof(float) * 2 * obs_len * N * nm));
    const size_t noise_stride = (size_t)S * std::max(N, ns) * (size_t)nd_max;
    HIP_TRY(h, M.dNoise.ensure(sizeof(float) * noise_stride * nm));
    HIP_TRY(h, M.dRaw.ensure(sizeof(float) * 2 * (size_t)S * pred_len * N));
    HIP_TRY(h, M.hTab.ensure(sizeof(int32_t) * 3 * (N + ns) * nm));
    HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * rows * (size_t)(R.n_dense + 1)));
    if (L.ep.sweep) { int r = sweep_ensure(h, S); if (r != FOT_OK) return r; }
    for (int m = 0; m < n_models; ++m)
        if (used[m]) { int r = sampler_model_scratch(h, m, (size_t)S, N); if (r != FOT_OK) return r; }
    if (models) {                                                // every model's raw tensor, scene tables and the rows' table
        HIP_TRY(h, M.dCrowdRaw.ensure(sizeof(float) * 2 * (size_t)S * pred_len * N * nm));
        HIP_TRY(h, M.dCrowdTab.ensure(sizeof(int32_t) * nm * ((ns + 1) + ns + N)));
        HIP_TRY(h, M.hCrowdTab.ensure(sizeof(int32_t) * nm * ((ns + 1) + ns + N)));
        HIP_TRY(h, M.dModelTab.ensure(sizeof(ModelRow) * N));
        HIP_TRY(h, M.hModelTab.ensure(sizeof(ModelRow) * N));
        M.slot_crowd.assign(slot_crowd, slot_crowd + n);
        M.slot_model.assign(slot_model, slot_model + n);
        const char *env = std::getenv("FOT_LOOP_MODEL_STREAMS");    // "0": every model on the loop's stream (measurements)
        M.side_on = !(env && env[0] == '0');
        if (M.side_on && !M.fork) HIP_TRY(h, hipEventCreateWithFlags(&M.fork, hipEventDisableTiming));
        for (int m = 1; M.side_on && m < n_models; ++m) {
            if (M.side[m]) continue;                             // (kept from an earlier set call of this handle)
            HIP_TRY(h, hipStreamCreateWithFlags(&M.side[m], hipStreamNonBlocking));
            HIP_TRY(h, hipEventCreateWithFlags(&M.join[m], hipEventDisableTiming));
        }
    } else if (crowds) {                                         // (slot e -> crowd e: today's step, nothing new)
        HIP_TRY(h, M.dCrowdRaw.ensure(sizeof(float) * 2 * (size_t)S * pred_len * N));
        HIP_TRY(h, M.dCrowdTab.ensure(sizeof(int32_t) * ((ns + 1) + ns + 2 * N)));
        HIP_TRY(h, M.hCrowdTab.ensure(sizeof(int32_t) * ((ns + 1) + ns + 2 * N)));
        M.slot_crowd.assign(slot_crowd, slot_crowd + n);
    }
    M.crowds = crowds && !models;
    M.models = models;
    M.n_models = n_models; M.noise_stride = noise_stride;
    M.kinds.assign(model_kind, model_kind + n_models);
    M.mshape.assign(nm, ModelShape());
    M.mscene_crowd.assign(nm * ns, -1);
    M.row_model.assign(N, 0); M.row_col.assign(N, 0);
    M.last_mscenes.assign(nm, 0); M.last_mrows.assign(nm, 0);
    M.sel.clear();
    M.last_scenes = M.last_rows = 0;
    M.S = S; M.seed = seed; M.kind = model_kind[0];
    M.on = true;
    R.sc.on = false;                                             // (a new sampler: its scores are enabled again, if wanted)
    L.slot_S.clear(); L.ep_S.clear();                            // ... and the slots' sample counts set anew
    return FOT_OK;
}

}  // namespace

extern "C" {

int fot_loop_set_scenario_static(fot_handle *h, int32_t id, int32_t n_points, const double *xy)
{
    if (!h) return FOT_ERR_INVALID;
    if (id < 0 || id >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "unknown scenario id");
    if (n_points < 0 || (n_points > 0 && !xy)) return fail(h, FOT_ERR_INVALID, "static points");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // nothing may still be reading the old copies
    LoopState &L = h->loop;
    if (L.scen_static.size() < h->sc.size()) L.scen_static.resize(h->sc.size());
    L.scen_static[(size_t)id].assign(xy, xy + 2 * (size_t)n_points);
    L.scen_static_dirty = true;                                  // (uploaded by the next scenario loop's step / replay)
    if (id == 0) {                                               // scenario 0 is what a fot_loop_begin loop sees
        L.static_xy = L.scen_static[0];
        L.static_tiles = 0;
    }
    return FOT_OK;
}

int fot_loop_set_static(fot_handle *h, int32_t n_points, const double *xy)
{
    return fot_loop_set_scenario_static(h, 0, n_points, xy);
}

int fot_loop_plan(fot_handle *h, const fot_loop_frame *frame, int32_t n_req, const fot_loop_request *req,
                  fot_safety *safety_out, const fot_result **records)
{
    return loop_plan_impl(h, frame, n_req, req, safety_out, records, 0);
}

int fot_loop_observe_begin(fot_handle *h, int32_t n, const double *ego5, const double *prev_s)
{
    // (the two-call form stays on scenario 0: what fot_loop_plan's frame leaves behind)
    return observe_begin_impl(h, n, ego5, prev_s);
}

int fot_loop_observe_end(fot_handle *h, fot_safety *safety_out, double *new_prev_s)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    const int n = L.observe_n;
    if (n < 0) return fail(h, FOT_ERR_INVALID, "no fot_loop_observe_begin to collect");
    L.observe_n = -1;
    if (n == 0) return FOT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (safety_out) std::memcpy(safety_out, L.hOut.p, sizeof(fot_safety) * (size_t)n);
    const InstState *p_state = (const InstState *)((const char *)L.hOut.p + align256(sizeof(fot_safety) * (size_t)n));
    if (new_prev_s) for (int i = 0; i < n; ++i) new_prev_s[i] = p_state[i].new_prev_s;
    return FOT_OK;
}

int fot_loop_observe(fot_handle *h, int32_t n, const double *ego5, const double *prev_s,
                     fot_safety *safety_out, double *new_prev_s)
{
    int rc = fot_loop_observe_begin(h, n, ego5, prev_s);
    return rc != FOT_OK ? rc : fot_loop_observe_end(h, safety_out, new_prev_s);
}

int fot_loop_begin(fot_handle *h, int32_t n_episodes, const fot_loop_config *cfg, const double *ego5)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_episodes < 0 || !cfg || (n_episodes > 0 && !ego5)) return fail(h, FOT_ERR_INVALID, "fot_loop_begin: arguments");
    if (!(cfg->dt > 0.0) || cfg->max_replan < 0 || cfg->max_replan > 8) return fail(h, FOT_ERR_INVALID, "fot_loop_begin: dt / max_replan");
    LoopEpisodes &E = h->loop.ep;
    const size_t n = (size_t)n_episodes;
    E.n = n_episodes; E.cfg = *cfg;
    E.scenarios = false; E.cfgs.clear(); E.use_fp.clear(); E.scen.clear();
    E.sweep = false; E.plan_mode.clear(); h->loop.sweep_tab.clear();
    h->loop.slot_S.clear(); h->loop.ep_S.clear();            // ... and a sweep's sample counts (fot_loop_set_slot_samples)
    E.max_lvl = loop_max_levels(*cfg);
    h->loop.frame_scen.clear(); h->loop.p_scen = nullptr;
    E.ego.assign(ego5, ego5 + 5 * n);
    E.prev_s.assign(n, NAN); E.last_kappa.assign(n, 0.0); E.goal_prev_s.assign(n, NAN);
    E.last_clearance.assign(n, INFINITY); E.clear.assign(n, INFINITY); E.clear_ahead.assign(n, INFINITY);
    E.state.assign(n, 0); E.fails.assign(n, 0); E.stats.assign(8 * n, -1);
    h->loop.replay.set = false;                                  // (a new loop: the handle's clock, if it had one, is gone)
    h->loop.replay.sum.on = false;                               // ... and the summaries' accumulators with it
    h->loop.replay.smp.on = false;                               // ... and the sampler
    h->loop.replay.rec.on = false; h->loop.replay.rec.rec = nullptr;   // ... or the recorded samples
    h->loop.replay.sc.on = false;                                // ... and its scores
    h->loop.rep.mode = FOT_LOOP_PLAN_DISTRIBUTION; h->loop.rep.frame = false;
    h->loop.rep.last_best.assign(n, -1);
    h->loop.fpo.on = false; h->loop.stepped = false;             // ... and the footprint observation's accumulators
    return FOT_OK;
}

int fot_loop_begin_scenarios(fot_handle *h, int32_t n_episodes, int32_t n_cfg, const fot_loop_config *cfg,
                             const int32_t *use_footprint, const int32_t *slot_scenario, const double *ego5)
{
    if (!h) return FOT_ERR_INVALID;
    if (n_episodes < 0 || n_cfg < 1 || !cfg || (n_episodes > 0 && (!ego5 || !slot_scenario)))
        return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: arguments");
    // --- everything is checked before anything changes
    int first = -1;
    for (int e = 0; e < n_episodes; ++e) {
        const int sc = slot_scenario[e];
        if (sc < 0 || sc >= (int)h->sc.size()) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: unknown scenario id");
        if (sc >= n_cfg) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: n_cfg is smaller than a slot's scenario id");
        if (!h->sc[(size_t)sc].has_path)
            return fail(h, FOT_ERR_NO_PATH_SET, "fot_loop_begin_scenarios: a slot's scenario has no path (fot_set_scenario_path_*)");
        const fot_loop_config &c = cfg[sc];
        if (!(c.dt > 0.0) || c.max_replan < 0 || c.max_replan > 8) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: dt / max_replan");
        if (first < 0) first = sc;
        if (c.dt != cfg[first].dt) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: the scenarios of a loop share dt");
    }
    if (first < 0) {                                             // no slot: nothing is in use but the first configuration
        first = 0;
        if (!(cfg[0].dt > 0.0) || cfg[0].max_replan < 0 || cfg[0].max_replan > 8) return fail(h, FOT_ERR_INVALID, "fot_loop_begin_scenarios: dt / max_replan");
    }
    const size_t n_sc = h->sc.size();
    std::vector<SafetyScen> tab(n_sc);
    for (size_t s = 0; s < n_sc; ++s) {
        tab[s].footprint_radius = h->sc[s].params.footprint_radius;
        tab[s].use_fp = ((int)s < n_cfg && use_footprint && use_footprint[s]) ? 1 : 0;
        tab[s]._pad = 0;
    }
    LoopState &L = h->loop;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // nothing may still be reading the old table
    HIP_TRY(h, L.dSafScen.ensure(sizeof(SafetyScen) * n_sc));
    HIP_TRY(h, hipMemcpy(L.dSafScen.p, tab.data(), sizeof(SafetyScen) * n_sc, hipMemcpyHostToDevice));
    // --- accepted
    LoopEpisodes &E = L.ep;
    const size_t n = (size_t)n_episodes;
    E.n = n_episodes; E.cfg = cfg[first];
    E.scenarios = true;
    E.sweep = false; E.plan_mode.clear(); L.sweep_tab.clear();
    L.slot_S.clear(); L.ep_S.clear();
    E.cfgs.assign(cfg, cfg + n_cfg);
    E.use_fp.assign((size_t)n_cfg, 0);
    for (int s = 0; s < n_cfg; ++s) E.use_fp[(size_t)s] = use_footprint && use_footprint[s] ? 1 : 0;
    E.scen.assign(slot_scenario, slot_scenario + n);
    E.max_lvl = loop_max_levels(cfg[first]);
    for (size_t e = 0; e < n; ++e) E.max_lvl = std::max(E.max_lvl, loop_max_levels(cfg[E.scen[e]]));
    L.frame_scen.clear(); L.p_scen = nullptr; L.have_frame = false;
    E.ego.assign(ego5, ego5 + 5 * n);
    E.prev_s.assign(n, NAN); E.last_kappa.assign(n, 0.0); E.goal_prev_s.assign(n, NAN);
    E.last_clearance.assign(n, INFINITY); E.clear.assign(n, INFINITY); E.clear_ahead.assign(n, INFINITY);
    E.state.assign(n, 0); E.fails.assign(n, 0); E.stats.assign(8 * n, -1);
    L.replay.set = false;
    L.replay.sum.on = false;
    L.replay.smp.on = false;
    L.replay.rec.on = false; L.replay.rec.rec = nullptr;
    L.replay.sc.on = false;
    L.rep.mode = FOT_LOOP_PLAN_DISTRIBUTION; L.rep.frame = false;
    L.rep.last_best.assign(n, -1);
    L.fpo.on = false; L.stepped = false;
    return FOT_OK;
}

int fot_loop_begin_sweep(fot_handle *h, int32_t n_episodes, int32_t n_cfg, const fot_loop_config *cfg,
                         const int32_t *use_footprint, const int32_t *slot_scenario, const int32_t *slot_plan_mode,
                         const double *ego5)
{
    if (!h) return FOT_ERR_INVALID;
    for (int e = 0; slot_plan_mode && e < n_episodes; ++e)
        if (slot_plan_mode[e] != FOT_LOOP_PLAN_DISTRIBUTION && slot_plan_mode[e] != FOT_LOOP_PLAN_REPRESENTATIVE)
            return fail(h, FOT_ERR_INVALID, "fot_loop_begin_sweep: a slot's plan mode is FOT_LOOP_PLAN_DISTRIBUTION or FOT_LOOP_PLAN_REPRESENTATIVE");
    // a scenario loop in every respect (the same arguments, the same refusals) ...
    { int r = fot_loop_begin_scenarios(h, n_episodes, n_cfg, cfg, use_footprint, slot_scenario, ego5); if (r != FOT_OK) return r; }
    // ... whose lock steps may carry a distribution, planned against in each slot's own mode
    LoopEpisodes &E = h->loop.ep;
    E.sweep = true;
    E.plan_mode.assign((size_t)n_episodes, FOT_LOOP_PLAN_DISTRIBUTION);
    if (slot_plan_mode) E.plan_mode.assign(slot_plan_mode, slot_plan_mode + n_episodes);
    return FOT_OK;
}

int fot_loop_step(fot_handle *h, const fot_loop_frame *frame, const int32_t *episode, fot_loop_step_out *out)
{
    if (!h) return FOT_ERR_INVALID;
    if (!frame || !out) return fail(h, FOT_ERR_INVALID, "fot_loop_step: frame / out");
    LoopState &L = h->loop;
    LoopEpisodes &E = L.ep;
    if (L.replay.set) return fail(h, FOT_ERR_INVALID, "fot_loop_step: a replay is set (fot_loop_run steps this handle; fot_loop_begin drops the replay)");
    const int n = frame->n_episodes;
    if (n < 0 || (n > 0 && !episode)) return fail(h, FOT_ERR_INVALID, "fot_loop_step: episode");
    out->records = nullptr; out->n_records = 0;
    if (n == 0) return FOT_OK;
    std::vector<uint8_t> seen((size_t)std::max(E.n, 1), 0);
    for (int i = 0; i < n; ++i) {
        if (episode[i] < 0 || episode[i] >= E.n || seen[(size_t)episode[i]]) return fail(h, FOT_ERR_INVALID, "fot_loop_step: episode slots must be distinct and below fot_loop_begin's count");
        seen[(size_t)episode[i]] = 1;
    }
    std::vector<int32_t> ep_scen;
    if (E.scenarios) {
        if (frame->dist_raw && !E.sweep) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_step: a scenario loop takes the constant-velocity predictor only (no dist_raw)");
        ep_scen.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            ep_scen[(size_t)i] = E.scen[(size_t)episode[i]];
            if (ep_scen[(size_t)i] >= (int)h->sc.size() || !h->sc[(size_t)ep_scen[(size_t)i]].has_path)
                return fail(h, FOT_ERR_NO_PATH_SET, "fot_loop_step: a slot's scenario has no path");
        }
    }
    L.stepped = true;
    StepWork W;
    step_level0(E, episode, n, W);
    HIP_TRY(h, hipSetDevice(h->device));
    if (L.observe_n > 0) { HIP_TRY(h, hipStreamSynchronize(h->stream)); L.observe_n = -1; }
    // (all records of the step in one pinned block that must not move between the two plan calls)
    HIP_TRY(h, L.hRec.ensure(sizeof(fot_result) * (size_t)n * (size_t)E.max_lvl));
    fot_loop_frame fr = *frame;
    fr.ego = W.ego4.data();
    const fot_result *rec = nullptr;
    { int rc = loop_plan_impl(h, &fr, n, W.req.data(), W.m.data(), &rec, 0, E.scenarios ? ep_scen.data() : nullptr, episode); if (rc != FOT_OK) return rc; }
    rec = (const fot_result *)L.hRec.p;
    for (int i = 0; i < n; ++i) E.last_clearance[episode[i]] = W.m[i].clearance_ahead;
    step_escalations(E, episode, n, rec, W);
    int n_rec = n;
    if (!W.more.empty()) {
        const fot_result *unused = nullptr;
        int rc = loop_plan_impl(h, nullptr, (int)W.more.size(), W.more.data(), nullptr, &unused, n);
        if (rc != FOT_OK) return rc;
        rec = (const fot_result *)L.hRec.p;
        n_rec += (int)W.more.size();
    }
    step_resolve(E, episode, n, rec, W);
    for (int i = 0; i < n; ++i) {
        if (out->ego) for (int k = 0; k < 5; ++k) out->ego[5 * (size_t)i + k] = W.ego5n[5 * (size_t)i + k];
        if (out->jerk) out->jerk[i] = W.jerk[i];
        if (out->record) out->record[i] = W.path_rec[i];
        if (out->keep) out->keep[i] = W.keep[i];
        if (out->cost) out->cost[i] = W.cost[i];
    }
    // --- result metrics on the new ego states and the goal test's nearest point (:864-883): enqueued, the rest of the
    //     outputs filled while they run
    std::vector<double> gps((size_t)n);
    for (int i = 0; i < n; ++i) gps[i] = E.goal_prev_s[episode[i]];
    { int rc = observe_begin_impl(h, n, W.ego5n.data(), gps.data(), episode); if (rc != FOT_OK) return rc; }
    for (int i = 0; i < n; ++i) {
        const int e = episode[i];
        if (out->state) out->state[i] = E.state[e];
        if (out->stats) for (int k = 0; k < 8; ++k) out->stats[8 * (size_t)i + k] = E.stats[8 * (size_t)e + k];
        if (out->before) out->before[i] = W.m[i];
    }
    std::vector<fot_safety> after((size_t)n);
    { int rc = fot_loop_observe_end(h, after.data(), gps.data()); if (rc != FOT_OK) return rc; }
    fpo_fold_step(L, episode, n);
    for (int i = 0; i < n; ++i) {
        E.goal_prev_s[episode[i]] = gps[i];
        if (out->after) out->after[i] = after[i];
        if (out->s_now) out->s_now[i] = gps[i];
    }
    out->records = rec;
    out->n_records = n_rec;
    return FOT_OK;
}

int fot_loop_set_replay(fot_handle *h, const fot_loop_replay *rp)
{
    if (!h) return FOT_ERR_INVALID;
    if (!rp) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: replay is NULL");
    LoopState &L = h->loop;
    const LoopEpisodes &E = L.ep;
    if (!E.scenarios && !h->sc[0].has_path) return fail(h, FOT_ERR_NO_PATH_SET, "fot_set_path_* has not been called");
    for (int e = 0; E.scenarios && e < E.n; ++e)
        if (E.scen[(size_t)e] >= (int)h->sc.size() || !h->sc[(size_t)E.scen[(size_t)e]].has_path)
            return fail(h, FOT_ERR_NO_PATH_SET, "fot_loop_set_replay: a slot's scenario has no path");
    if (!(E.cfg.dt > 0.0)) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: fot_loop_begin comes first");
    const int n = rp->n_slots;
    if (n != E.n) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: n_slots differs from fot_loop_begin's episode count");
    if (!rp->ped_off || (n > 0 && !rp->n_frames) || rp->n_frames_max < 1 || rp->warmup_frames < 0)
        return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: ped_off / n_frames / n_frames_max / warmup_frames");
    for (int i = 0; i < n; ++i)
        if (rp->ped_off[i + 1] < rp->ped_off[i] || rp->ped_off[0] != 0)
            return fail(h, FOT_ERR_INVALID, "ped_off must start at 0 and be non-decreasing");
    for (int i = 0; i < n; ++i)
        if (rp->n_frames[i] < 1 || rp->n_frames[i] > rp->n_frames_max)
            return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: every slot needs 1 .. n_frames_max recorded frames");
    const size_t cols = n > 0 ? (size_t)rp->ped_off[n] : 0;
    if (cols > 0 && (!rp->pos || !rp->vel)) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: NULL recording");
    if (rp->obs_len < 2) return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: obs_len < 2 (the predictor needs two samples)");
    if (!(rp->rp.sim_dt > 0.0) || !(rp->rp.sgan_dt > 0.0) || rp->pred_len < 1)
        return fail(h, FOT_ERR_INVALID, "fot_loop_set_replay: predictor parameters");
    if (rp->pred_len > FOT_MAX_PRED_LEN) return fail(h, FOT_ERR_UNSUPPORTED, "pred_len > FOT_MAX_PRED_LEN");
    const int n_dense = resample_n_dense(rp->rp.sgan_dt, rp->rp.sim_dt, rp->rp.plan_horizon, rp->pred_len);
    if (n_dense + 1 > FOT_MAX_NT) return fail(h, FOT_ERR_UNSUPPORTED, "more than FOT_MAX_NT time steps");
    // --- accepted: everything the steps need is allocated here, so that no block grows (and moves) inside a run
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // nothing may still read what is replaced below
    LoopReplay &R = L.replay;
    R.set = false;
    R.sum.on = false;                                            // (a new recording: summaries are enabled again, if wanted)
    R.smp.on = false;                                            // ... and so is a sampler
    R.rec.on = false; R.rec.rec = nullptr;                       // ... or recorded samples
    R.sc.on = false;                                             // ... and its scores
    L.slot_S.clear(); L.ep_S.clear();                            // ... and the slots' sample counts, which were the source's
    const size_t rec_doubles = (size_t)rp->n_frames_max * cols * 2;
    const int max_lvl = E.max_lvl;
    const size_t n_rec = (size_t)std::max(n, 1) * (size_t)max_lvl;
    const FrameLayout FL((size_t)n, cols);
    HIP_TRY(h, R.dPos.ensure(sizeof(double) * std::max<size_t>(rec_doubles, 2)));
    HIP_TRY(h, R.dVel.ensure(sizeof(double) * std::max<size_t>(rec_doubles, 2)));
    HIP_TRY(h, R.dTab.ensure(sizeof(int32_t) * (2 * (size_t)n + 1)));
    HIP_TRY(h, R.dFrame.ensure(FL.dev_bytes()));
    HIP_TRY(h, R.dRec.ensure_zeroed(sizeof(fot_result) * n_rec));
    HIP_TRY(h, L.dDyn.ensure(sizeof(double) * 2 * std::max<size_t>(cols, 1) * (size_t)(n_dense + 1)));
    HIP_TRY(h, R.hStage.ensure(FL.stage_bytes()));
    HIP_TRY(h, R.hDigest.ensure(sizeof(LoopDigest) * n_rec));
    HIP_TRY(h, R.hHistTab.ensure(sizeof(int32_t) * 2 * (size_t)std::max(n, 1)));
    HIP_TRY(h, R.hWord.ensure(sizeof(int32_t) * 32));
    HIP_TRY(h, L.hOut.ensure(align256(sizeof(fot_safety) * (size_t)std::max(n, 1)) + sizeof(InstState) * (size_t)std::max(n, 1)));
    HIP_TRY(h, L.hObserve.ensure(align256(sizeof(double) * 4 * (size_t)std::max(n, 1)) + align256(sizeof(InstDesc) * (size_t)std::max(n, 1))));
    if (E.scenarios) { int r = ensure_scen_static(h, (int)n_rec, h->stream); if (r != FOT_OK) return r; }
    if (rec_doubles) {
        HIP_TRY(h, hipMemcpy(R.dPos.p, rp->pos, sizeof(double) * rec_doubles, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(R.dVel.p, rp->vel, sizeof(double) * rec_doubles, hipMemcpyHostToDevice));
    }
    std::vector<int32_t> tab(2 * (size_t)n + 1);
    for (int i = 0; i <= n; ++i) tab[(size_t)i] = rp->ped_off[i];
    for (int i = 0; i < n; ++i) tab[(size_t)n + 1 + (size_t)i] = rp->n_frames[i];
    HIP_TRY(h, hipMemcpy(R.dTab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice));
    R.cfg = *rp;
    R.cfg.ped_off = nullptr; R.cfg.n_frames = nullptr; R.cfg.pos = nullptr; R.cfg.vel = nullptr;
    R.n_cols = (int)cols; R.n_dense = n_dense; R.max_lvl = max_lvl;
    R.ped_off.assign(rp->ped_off, rp->ped_off + n + 1);
    R.n_frames.assign(rp->n_frames, rp->n_frames + n);
    R.pos.assign(rp->pos, rp->pos + rec_doubles);
    R.vel.clear();                                               // (the host needs the positions only: the prepend test)
    R.alive.assign((size_t)n, 1); R.steps.assign((size_t)n, 0); R.termination.assign((size_t)n, 0);
    R.clock.reset(rp->obs_len, rp->rp.sim_dt, rp->rp.sgan_dt);
    for (int i = 0; i < rp->warmup_frames; ++i) R.clock.advance();   // fills the observer (integrated_simulator.py:406-422)
    L.have_frame = false; L.observe_n = -1;
    R.set = true;
    return FOT_OK;
}

int fot_loop_summary_enable(fot_handle *h, int32_t on, int32_t num_samples)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: fot_loop_set_replay comes first");
    const int n = R.cfg.n_slots;
    for (int e = 0; e < n; ++e)
        if (R.steps[(size_t)e] != 0) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: the run has begun (enable between fot_loop_set_replay and the first step)");
    if (R.clock.frame != R.cfg.warmup_frames) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: the run has begun (enable between fot_loop_set_replay and the first step)");
    LoopSummaryAcc &A = R.sum;
    if (!on) { A.on = false; return FOT_OK; }
    if (R.smp.on) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_summary_enable: a sampler is set (fot_loop_set_sampler): the prediction-error ring reads the constant-velocity tensor");
    if (R.rec.on) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_summary_enable: recorded samples are set (fot_loop_set_samples): the prediction-error ring reads the constant-velocity tensor");
    if (num_samples < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: num_samples < 1");
    const int stride = summary_stride(R.cfg.rp.sgan_dt, R.cfg.rp.sim_dt);
    if (stride < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_summary_enable: sgan_dt must be a multiple of sim_dt");
    { int r = summary_arm(h, num_samples, stride); if (r != FOT_OK) return r; }
    A.on = true;
    return FOT_OK;
}

int fot_loop_summaries(fot_handle *h, int32_t n_slots, fot_loop_summary *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: fot_loop_set_replay comes first");
    if (!R.sum.on) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: summaries are not enabled (fot_loop_summary_enable)");
    if (n_slots != R.cfg.n_slots) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: n_slots differs from the loop's");
    if (n_slots > 0 && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_summaries: out is NULL");
    if (n_slots == 0) return FOT_OK;
    return summaries_fill(h, n_slots, out);
}

int fot_loop_scores_enable(fot_handle *h, int32_t on)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: fot_loop_set_replay comes first");
    if (!R.smp.on && !R.rec.on)
        return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: no sampler or recording is set (fot_loop_set_sampler / fot_loop_set_samples comes first)");
    const int n = R.cfg.n_slots;
    bool begun = R.clock.frame != R.cfg.warmup_frames;
    for (int e = 0; e < n; ++e) begun = begun || R.steps[(size_t)e] != 0;
    if (begun) return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: the run has begun (enable between fot_loop_set_sampler / fot_loop_set_samples and the first step)");
    LoopScores &Q = R.sc;
    if (!on) { Q.on = false; return FOT_OK; }
    const int stride = summary_stride(R.cfg.rp.sgan_dt, R.cfg.rp.sim_dt);
    if (stride < 1) return fail(h, FOT_ERR_INVALID, "fot_loop_scores_enable: sgan_dt must be a multiple of sim_dt");
    // --- accepted: everything the mode needs is allocated here
    Q.on = false;
    { int r = summary_arm(h, R.dist_S(), stride); if (r != FOT_OK) return r; }
    const size_t ns = (size_t)std::max(n, 1), cols = (size_t)std::max(R.n_cols, 1), E = (size_t)R.cfg.pred_len;
    HIP_TRY(h, Q.dBest.ensure(sizeof(int32_t) * ns));
    const size_t dev_stride = (size_t)best_dev_stride(R.dist_S());   // (the table rows of the loop's own S)
    HIP_TRY(h, Q.dDev.ensure(sizeof(double) * ns * dev_stride));
    HIP_TRY(h, Q.dTruth.ensure(sizeof(double) * 2 * cols * E));
    HIP_TRY(h, Q.hBest.ensure(sizeof(int32_t) * ns));
    HIP_TRY(h, Q.hDesc.ensure(sizeof(PredOriginDev) * ns));
    HIP_TRY(h, Q.hRec.ensure(sizeof(fot_pred_score) * ns));
    HIP_TRY(h, hipMemsetAsync(Q.dBest.p, 0xFF, sizeof(int32_t) * ns, h->stream));
    HIP_TRY(h, hipMemsetAsync(Q.dDev.p, 0, sizeof(double) * ns * dev_stride, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::memset(Q.hBest.p, 0xFF, sizeof(int32_t) * ns);
    std::memset(Q.hRec.p, 0, sizeof(fot_pred_score) * ns);
    Q.stride = stride; Q.H = stride * R.cfg.pred_len;
    Q.std_ok = ps_horizon_fits(stride, R.cfg.pred_len, R.n_dense + 1, 1);
    Q.ring.assign(ns * (size_t)Q.H, ps_zero(R.dist_S()));
    for (size_t e = 0; e < h->loop.slot_S.size(); ++e)           // (a count per slot; no record of the fresh ring is ever folded)
        std::fill(Q.ring.begin() + (ptrdiff_t)(e * (size_t)Q.H), Q.ring.begin() + (ptrdiff_t)((e + 1) * (size_t)Q.H), ps_zero(h->loop.slot_S[e]));
    Q.fold.assign(ns, score_fold_zero());
    Q.last_best.assign(ns, -1);
    Q.on = true;
    return FOT_OK;
}

int fot_loop_score_summaries(fot_handle *h, int32_t n_slots, fot_loop_summary *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set || !R.sc.on) return fail(h, FOT_ERR_INVALID, "fot_loop_score_summaries: scores are not enabled (fot_loop_scores_enable)");
    if (n_slots != R.cfg.n_slots) return fail(h, FOT_ERR_INVALID, "fot_loop_score_summaries: n_slots differs from the loop's");
    if (n_slots > 0 && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_score_summaries: out is NULL");
    if (n_slots == 0) return FOT_OK;
    { int r = summaries_fill(h, n_slots, out); if (r != FOT_OK) return r; }
    // the ring's standard-cadence totals are the representative sample's: the best-of-N and KDE keys are the fold's
    for (int e = 0; e < n_slots; ++e) {
        double m[5];
        int32_t samples = 0;
        const ScoreFold &F = R.sc.fold[(size_t)e];
        score_fold_means(F, m, &samples);
        fot_loop_summary &s = out[e];
        s.ade = m[0]; s.fde = m[1]; s.ade_per_agent = m[2]; s.fde_per_agent = m[3]; s.nll = m[4];
        s.ade_eval_count = (int32_t)F.count; s.nll_eval_count = (int32_t)F.nll_count; s.pred_samples = samples;
    }
    return FOT_OK;
}

int fot_loop_last_best_sample(fot_handle *h, int32_t n_slots, int32_t *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    const LoopRep &Q = h->loop.rep;
    const bool scores = R.set && R.sc.on, planned = Q.mode == FOT_LOOP_PLAN_REPRESENTATIVE || h->loop.ep.sweep;
    if (!scores && !planned)
        return fail(h, FOT_ERR_INVALID, "fot_loop_last_best_sample: scores are not enabled (fot_loop_scores_enable)");
    // (a stepwise loop planning on the representative sample: the slots of fot_loop_begin)
    if (n_slots != (scores ? R.cfg.n_slots : h->loop.ep.n)) return fail(h, FOT_ERR_INVALID, "fot_loop_last_best_sample: n_slots differs from the loop's");
    if (n_slots > 0 && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_last_best_sample: out is NULL");
    for (int e = 0; e < n_slots; ++e) out[e] = scores ? R.sc.last_best[(size_t)e] : Q.last_best[(size_t)e];
    return FOT_OK;
}

int fot_loop_plan_sample(fot_handle *h, int32_t mode)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    if (mode != FOT_LOOP_PLAN_DISTRIBUTION && mode != FOT_LOOP_PLAN_REPRESENTATIVE)
        return fail(h, FOT_ERR_INVALID, "fot_loop_plan_sample: mode is FOT_LOOP_PLAN_DISTRIBUTION or FOT_LOOP_PLAN_REPRESENTATIVE");
    if (!(L.ep.cfg.dt > 0.0)) return fail(h, FOT_ERR_INVALID, "fot_loop_plan_sample: fot_loop_begin comes first");
    if (L.ep.sweep) return fail(h, FOT_ERR_INVALID, "fot_loop_plan_sample: a sweep loop's plan modes were given per slot (fot_loop_begin_sweep)");
    if (L.ep.scenarios) return fail(h, FOT_ERR_UNSUPPORTED, "fot_loop_plan_sample: a scenario loop plans against no distribution");
    if (R.set) {
        bool begun = R.clock.frame != R.cfg.warmup_frames;
        for (int e = 0; e < R.cfg.n_slots; ++e) begun = begun || R.steps[(size_t)e] != 0;
        if (begun) return fail(h, FOT_ERR_INVALID, "fot_loop_plan_sample: the run has begun (choose between fot_loop_set_replay and the first step)");
    }
    if (mode == FOT_LOOP_PLAN_REPRESENTATIVE && R.set) {
        // a resident run: everything its steps need is allocated here, so that no block grows (and moves) inside the run
        HIP_TRY(h, hipSetDevice(h->device));
        int r = rep_ensure(h, R.cfg.n_slots, R.cfg.n_slots, (size_t)R.n_cols, R.n_dense + 1, R.dist_S());   // (a predictor set later: grown at its first step)
        if (r != FOT_OK) return r;
    }
    L.rep.mode = mode;
    L.rep.frame = false;                                         // (the next frame decides what its requests plan against)
    L.rep.last_best.assign((size_t)L.ep.n, -1);
    L.rep.run_best.clear();
    return FOT_OK;
}

int fot_loop_run_best_samples(fot_handle *h, int32_t n_steps, int32_t n_slots, int32_t *out)
{
    if (!h) return FOT_ERR_INVALID;
    const LoopState &L = h->loop;
    if (!L.replay.set || (L.rep.mode != FOT_LOOP_PLAN_REPRESENTATIVE && !L.ep.sweep))
        return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: no resident run plans on the representative sample (fot_loop_plan_sample)");
    if (n_slots != L.replay.cfg.n_slots) return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: n_slots differs from the loop's");
    if (n_steps < 0 || (size_t)n_steps * (size_t)n_slots != L.rep.run_best.size())
        return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: n_steps differs from the steps of the most recent fot_loop_run");
    if (!L.rep.run_best.empty() && !out) return fail(h, FOT_ERR_INVALID, "fot_loop_run_best_samples: out is NULL");
    if (!L.rep.run_best.empty()) std::memcpy(out, L.rep.run_best.data(), sizeof(int32_t) * L.rep.run_best.size());
    return FOT_OK;
}

int fot_debug_loop_block(fot_handle *h, int32_t episode, int32_t cap_points, double *xy, int32_t *P, int32_t *T,
                         int32_t *prepended)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    if (!L.have_frame) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: no frame");
    const int n_ep = (int)L.ped_off.size() - 1;
    if (episode < 0 || episode >= n_ep) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: episode out of range");
    if (cap_points < 0 || (cap_points > 0 && !xy)) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: cap_points / xy");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t e = (size_t)episode;
    const int P_e = L.ped_off[e + 1] - L.ped_off[e];
    int t_len = 0, pre = -1;
    int64_t first = 0, n_pts = 0;
    const void *base = nullptr;
    if (L.rep.frame) {
        t_len = L.rep.T; first = (int64_t)L.ped_off[e] * t_len; n_pts = (int64_t)P_e * t_len; base = L.rep.dBlk.p;
        if (P_e > 0) pre = ((const int32_t *)L.rep.hPre.p)[e];
    } else if (!L.sweep_tab.empty() && sweep_plans_on_block(L.sweep_tab[e])) {   // (a sweep's episode in representative mode)
        t_len = L.sweep_T; first = L.sweep_tab[e].rep_off; n_pts = sweep_block_points(P_e, t_len); base = L.dyn_ptr;
        if (P_e > 0) pre = ((const int32_t *)L.rep.hPre.p)[e];
    } else {
        t_len = L.t_len[e]; first = L.blk_off[e]; n_pts = (int64_t)std::max(L.count_of(e), 1) * P_e * t_len; base = L.dyn_ptr;
    }
    if (P) *P = P_e;
    if (T) *T = t_len;
    if (prepended) *prepended = pre;
    if (n_pts > cap_points) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_block: the block holds more than cap_points points");
    if (n_pts > 0 && base)
        HIP_TRY(h, hipMemcpy(xy, (const double *)base + 2 * first, sizeof(double) * 2 * (size_t)n_pts, hipMemcpyDefault));
    return FOT_OK;
}

int fot_loop_set_sampler(fot_handle *h, int32_t S, uint64_t seed, int32_t kind)
{
    if (!h) return FOT_ERR_INVALID;
    return set_sampler_impl(h, "fot_loop_set_sampler", S, seed, 1, &kind, false, 0, nullptr, false, nullptr);
}

int fot_loop_set_sampler_shared(fot_handle *h, int32_t S, uint64_t seed, int32_t kind, int32_t n_crowds, const int32_t *slot_crowd)
{
    if (!h) return FOT_ERR_INVALID;
    return set_sampler_impl(h, "fot_loop_set_sampler_shared", S, seed, 1, &kind, true, n_crowds, slot_crowd, false, nullptr);
}

int fot_loop_set_sampler_models(fot_handle *h, int32_t S, uint64_t seed, int32_t n_models, const int32_t *model_kind,
                                int32_t n_crowds, const int32_t *slot_crowd, const int32_t *slot_model)
{
    if (!h) return FOT_ERR_INVALID;
    return set_sampler_impl(h, "fot_loop_set_sampler_models", S, seed, n_models, model_kind, true, n_crowds, slot_crowd, true, slot_model);
}

int fot_debug_loop_sampler_shapes(fot_handle *h, int32_t cap, int32_t *n_scenes, int32_t *n_rows)
{
    if (!h) return FOT_ERR_INVALID;
    LoopReplay &R = h->loop.replay;
    if (!R.set || !R.smp.on) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_sampler_shapes: no sampler is set (fot_loop_set_sampler)");
    if (cap < 0 || (cap > 0 && (!n_scenes || !n_rows))) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_sampler_shapes: cap / NULL array");
    for (int m = 0; m < cap; ++m) {                              // (ids the loop does not name: nothing was handed to them)
        const bool named = m < R.smp.n_models;
        n_scenes[m] = !named ? 0 : R.smp.models ? R.smp.last_mscenes[(size_t)m] : R.smp.last_scenes;
        n_rows[m] = !named ? 0 : R.smp.models ? R.smp.last_mrows[(size_t)m] : R.smp.last_rows;
    }
    return FOT_OK;
}

int fot_debug_loop_sampler_shape(fot_handle *h, int32_t *n_scenes, int32_t *n_rows)
{
    if (!h) return FOT_ERR_INVALID;
    const LoopReplay &R = h->loop.replay;
    if (!R.set || !R.smp.on) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_sampler_shape: no sampler is set (fot_loop_set_sampler)");
    if (n_scenes) *n_scenes = R.smp.last_scenes;
    if (n_rows) *n_rows = R.smp.last_rows;
    return FOT_OK;
}

int fot_loop_set_samples(fot_handle *h, int32_t S, int32_t n_steps, int32_t first_step, const void *samples, int32_t dtype,
                         int32_t flags)
{
    if (!h) return FOT_ERR_INVALID;
    return set_samples_impl(h, "fot_loop_set_samples", S, n_steps, first_step, samples, dtype, flags, false, 0, nullptr);
}

int fot_loop_set_samples_shared(fot_handle *h, int32_t S, int32_t n_steps, int32_t first_step, const void *samples,
                                int32_t dtype, int32_t flags, int32_t n_rec_cols, const int32_t *slot_col0)
{
    if (!h) return FOT_ERR_INVALID;
    return set_samples_impl(h, "fot_loop_set_samples_shared", S, n_steps, first_step, samples, dtype, flags, true, n_rec_cols, slot_col0);
}

int fot_loop_set_slot_samples(fot_handle *h, int32_t n_slots, const int32_t *slot_S)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    const std::string who = "fot_loop_set_slot_samples: ";
    if (!(L.ep.cfg.dt > 0.0)) return fail(h, FOT_ERR_INVALID, who + "fot_loop_begin_sweep comes first");
    if (!L.ep.sweep) return fail(h, FOT_ERR_UNSUPPORTED, who + "the slots of a sweep loop (fot_loop_begin_sweep) take sample counts of their own; this loop's share one");
    if (!slot_S) return fail(h, FOT_ERR_INVALID, who + "slot_S is NULL");
    if (n_slots != L.ep.n) return fail(h, FOT_ERR_INVALID, who + "n_slots differs from the loop's");
    // the source's count: the recording's or the sampler's of a resident loop; a stepwise loop's frames bring theirs
    // (fot_loop_frame.dist_S, held against the counts by every fot_loop_step), so the handle's capacity bounds them here
    int S = h->sample_cap;
    if (R.set) {
        if (!R.smp.on && !R.rec.on)
            return fail(h, FOT_ERR_INVALID, who + "no sampler or recording is set (fot_loop_set_sampler* / fot_loop_set_samples* comes first)");
        S = R.dist_S();
    }
    bool begun = L.stepped || (R.set && R.clock.frame != R.cfg.warmup_frames);
    for (int e = 0; R.set && e < R.cfg.n_slots; ++e) begun = begun || R.steps[(size_t)e] != 0;
    if (begun) return fail(h, FOT_ERR_INVALID, who + "the loop has stepped (set the counts between the source and the first step)");
    for (int e = 0; e < n_slots; ++e)
        if (slot_S[e] < 1 || slot_S[e] > S)
            return fail(h, FOT_ERR_INVALID, who + "slot_S[" + std::to_string(e) + "] = " + std::to_string(slot_S[e]) + " lies outside 1 .. " +
                                            std::to_string(S) + (R.set ? " (the source's samples)" : " (the handle's sample capacity)"));
    if (R.set && sweep_slot_capacity_points(n_slots, R.ped_off.data(), slot_S, R.n_dense + 1) >
                     sweep_capacity_points(S, std::max(R.n_cols, 1), R.n_dense + 1))
        return fail(h, FOT_ERR_INVALID, who + "internal: the counts need more than the sweep's tensor holds");
    // --- accepted
    HIP_TRY(h, L.hEpS.ensure(sizeof(int32_t) * (size_t)std::max(n_slots, 1)));
    L.slot_S.assign(slot_S, slot_S + n_slots);
    L.ep_S.clear();
    return FOT_OK;
}

int fot_debug_loop_slot_samples(fot_handle *h, int32_t n_slots, int32_t *out)
{
    if (!h) return FOT_ERR_INVALID;
    const LoopState &L = h->loop;
    if (!L.have_frame) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_slot_samples: no frame");
    const int n_ep = (int)L.ped_off.size() - 1;
    if (n_slots < n_ep || (n_slots > 0 && !out)) return fail(h, FOT_ERR_INVALID, "fot_debug_loop_slot_samples: room for fewer entries than the frame has episodes / out is NULL");
    for (int i = 0; i < n_slots; ++i) out[i] = i < n_ep ? L.count_of((size_t)i) : -1;   // (0: the frame carried no distribution)
    return FOT_OK;
}

int fot_loop_run(fot_handle *h, int32_t max_steps, fot_loop_run_out *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    LoopReplay &R = L.replay;
    if (!R.set) return fail(h, FOT_ERR_INVALID, "fot_loop_run: fot_loop_set_replay comes first");
    if (max_steps < 0 || !out) return fail(h, FOT_ERR_INVALID, "fot_loop_run: max_steps / out");
    const int n_slots = R.cfg.n_slots;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const size_t step_doubles = 15 * (size_t)n_slots * (size_t)h->sc[0].P.n_total;
    const bool keep_paths = out->paths != nullptr && step_doubles > 0 && max_steps > 0;
    if (keep_paths) {
        HIP_TRY(h, R.dHist.ensure(sizeof(double) * step_doubles * (size_t)max_steps));
        HIP_TRY(h, hipMemsetAsync(R.dHist.p, 0, sizeof(double) * step_doubles * (size_t)max_steps, st));
    }
    int done = 0;
    std::vector<int32_t> sel;
    L.rep.run_best.clear();
    for (; done < max_steps; ++done) {
        sel.clear();
        for (int e = 0; e < n_slots; ++e) if (R.alive[(size_t)e]) sel.push_back(e);
        if (sel.empty()) break;
        if (R.rec.on) {
            // Would this step predict, and is its row recorded?  The clock does not depend on the ego, so the host knows
            // before anything of the step is enqueued: a step outside the recording is not run.
            ReplayClock next = R.clock;
            next.advance();
            int rows_run = 0;
            for (int32_t e : sel) rows_run += R.ped_off[(size_t)e + 1] - R.ped_off[(size_t)e];
            const int step = R.steps[(size_t)sel[0]];
            if (next.ready() && rows_run > 0 && !sr_covers(R.rec.first_step, R.rec.n_steps, step)) {
                if (done > 0) break;
                return fail(h, FOT_ERR_INVALID, "fot_loop_run: lock step " + std::to_string(step) + " predicts, but the recorded samples (fot_loop_set_samples) cover steps " +
                                                std::to_string(R.rec.first_step) + " .. " + std::to_string((int64_t)R.rec.first_step + R.rec.n_steps - 1));
            }
        }
        int rc = loop_run_step(h, sel, done, out, keep_paths ? R.dHist.as<double>() + step_doubles * (size_t)done : nullptr);
        if (rc != FOT_OK) return rc;
    }
    if (done > 0) { int r = order_end(h, st); if (r != FOT_OK) return r; }
    if (keep_paths && done > 0) {                                // the call's history block, in one copy
        HIP_TRY(h, hipMemcpyAsync(out->paths, R.dHist.p, sizeof(double) * step_doubles * (size_t)done, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    for (int e = 0; e < n_slots; ++e) {
        if (out->steps) out->steps[e] = R.steps[(size_t)e];
        if (out->termination) out->termination[e] = R.termination[(size_t)e];
    }
    return done;
}

// ---- the observational footprint metrics of a loop (include/fot.h; fot_footprint_obs.hpp) ---------------------------------
int fot_loop_footprint_enable(fot_handle *h, const fot_footprint_geom *geom)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    const std::string who = "fot_loop_footprint_enable: ";
    if (!(L.ep.cfg.dt > 0.0)) return fail(h, FOT_ERR_INVALID, who + "fot_loop_begin* comes first");
    if (L.stepped) return fail(h, FOT_ERR_INVALID, who + "the loop has stepped (enable between fot_loop_begin* and the first step)");
    LoopFootprintObs &F = L.fpo;
    if (!geom) { F.on = false; return FOT_OK; }
    const char *why = "";
    if (fpo_check_geom(geom->vehicle_length, geom->vehicle_width, geom->ped_radius, geom->legacy_radius, geom->n_circles, &why))
        return fail(h, FOT_ERR_INVALID, who + why);
    const size_t n = (size_t)std::max(L.ep.n, 1);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // nothing may still read the geometry that is replaced
    HIP_TRY(h, F.hGeom.ensure(sizeof(FpoGeom)));
    HIP_TRY(h, F.hRec.ensure(sizeof(FpoStep) * n));
    F.geom = fpo_geom(geom->vehicle_length, geom->vehicle_width, geom->ped_radius, geom->legacy_radius, geom->n_circles);
    std::memcpy(F.hGeom.p, &F.geom, sizeof F.geom);
    F.acc.assign(n, fpo_acc_zero());
    F.steps.assign(n, 0);
    F.on = true;
    return FOT_OK;
}

int fot_loop_footprint_obs(fot_handle *h, int32_t n_slots, fot_footprint_obs *out)
{
    if (!h) return FOT_ERR_INVALID;
    LoopState &L = h->loop;
    const std::string who = "fot_loop_footprint_obs: ";
    if (!(L.ep.cfg.dt > 0.0)) return fail(h, FOT_ERR_INVALID, who + "fot_loop_begin* comes first");
    if (!L.fpo.on) return fail(h, FOT_ERR_INVALID, who + "not enabled (fot_loop_footprint_enable)");
    if (n_slots != L.ep.n) return fail(h, FOT_ERR_INVALID, who + "n_slots differs from the loop's");
    if (n_slots > 0 && !out) return fail(h, FOT_ERR_INVALID, who + "out is NULL");
    for (int e = 0; e < n_slots; ++e) {
        const FpoRecord r = fpo_acc_record(L.fpo.acc[(size_t)e], L.fpo.geom, L.fpo.steps[(size_t)e]);
        std::memcpy(&out[e], &r, sizeof r);
    }
    return FOT_OK;
}

}  // extern "C"
