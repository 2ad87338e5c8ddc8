// The three evaluation kernels, included three times by fot_kernels.hip: as k_evaluate / k_evaluate_split /
// k_evaluate_group (FOT_EVAL_LEAN false: the general form), as k_evaluate_lean / k_evaluate_split_lean /
// k_evaluate_group_lean (FOT_EVAL_LEAN true: FusedSink<true>) and as k_evaluate_split_lean_flat /
// k_evaluate_group_lean_flat (FOT_EVAL_FLAT true on top: the walk of exactly straight reference paths,
// frenet_to_cart<., true>); and twice more with FOT_EVAL_WORDS = WIDE_MASK_WORDS, as k_evaluate_wide / _split_wide /
// _group_wide and k_evaluate_lean_wide / _split_lean_wide / _group_lean_wide: the launches with an instance of more than
// FOT_MAX_SAMPLES prediction samples (FusedSink<., WIDE_MASK_WORDS>).  The per-wave kernel has no flat form: it came out with one lane-spilled scalar register
// more than k_evaluate_lean (10 against 9), and a flat-eligible launch of that shape runs k_evaluate_lean.
// Inclusions rather than a template body behind wrappers: each kernel
// then reads its argument struct in place, exactly as the single form did (through a wrapper the struct is copied and
// every field loaded at entry -- three more lane-spilled SGPRs in the grouped kernel).

// One wave per tile.  The grid deals the tiles out position-major and XCD-aligned: workgroup b serves the instances
// x, x + 8, ... with x = b mod 8 -- the XCD that, under round-robin placement, also ran k_cull's workgroups for them,
// so their lists sit in its L2 (speed only) -- and an instance's LAST tile comes first (late horizons and the brake
// ladder run longest), so the long tiles start early and the short ones fill the end of the launch.  The waves of a
// workgroup share nothing but the staged spline: each has its own slice of LDS.
#if !FOT_EVAL_FLAT
__global__ void __launch_bounds__(EVAL_WG) __attribute__((amdgpu_waves_per_eu(3, 3)))
FOT_EVAL_KERNEL(k_evaluate)(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc, const InstState *__restrict__ state,
           const int32_t *__restrict__ tile_cand0, const int32_t *__restrict__ tile_n,
           const TileStep *__restrict__ wave_rng, const f2 *__restrict__ ent32, const EvalKernArgs a)
{
    // (eval_kernargs() addresses the struct's fields in the argument segment, behind the EVAL_LEAD_PTRS pointers)
    const int waves_per_wg = (int)blockDim.x / WAVE;
    const int wave_doubles = eval_wave_doubles(a.row_budget);
#ifdef FOT_TIMELINE
    if (threadIdx.x == 0) s_tl_entry[0] = __builtin_amdgcn_s_memrealtime();
#endif
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const int lane = threadIdx.x & (WAVE - 1);
    double *my_rows = s_lon + wv * wave_doubles;
    const int x = (int)blockIdx.x & (N_XCD - 1);
    const int m_x = (a.n_inst - x + N_XCD - 1) / N_XCD;            // instances x, x + 8, ...
    // the tile of wave w of this workgroup: instance (-1: none) and position
    const auto wave_inst = [&](int w, int &pos_w) {
        const int q = ((int)blockIdx.x >> 3) * waves_per_wg + w;
        if (m_x <= 0 || q >= m_x * a.max_tiles) return -1;
        pos_w = q / m_x;
        const int i = x + N_XCD * (q - pos_w * m_x);
        return pos_w < desc[i].n_tiles ? i : -1;                  // (a shorter lattice than the batch's longest: none)
    };
    int pos = 0;
    const int inst = wave_inst(wv, pos);
    // LDS: per wave [rows | summaries | row offsets], then the spline (shared by the workgroup's waves).  The waves of a
    // workgroup serve different instances: in a mixed batch the spline is staged when all of them are on one scenario,
    // otherwise every wave reads its own scenario's spline from HBM (no LDS taken from the row tables).
    SplineView sp_stage = a.sp;
    if (a.mixed) {
        int common = -1;                                         // -1: none yet, -2: the waves disagree
        for (int w = 0; w < waves_per_wg; ++w) {                 // (uniform: every wave walks the same workgroup)
            int pw;
            const int iw = wave_inst(w, pw);
            if (iw < 0) continue;
            const int sw = desc[iw].scen;
            common = common == -1 || common == sw ? sw : -2;
        }
        if (common >= 0) sp_stage = load_const(a.sp_table, common);
        else sp_stage.n = a.lds_knots + 1;                       // nothing staged: no wave reads sp_stage
        if (inst >= 0) Pp += desc[inst].scen;
    }
    SplineView sp_lds = stage_spline(sp_stage, a.lds_knots, s_lon + waves_per_wg * wave_doubles);
    if (a.mixed && inst >= 0 && sp_stage.n > a.lds_knots) sp_lds = load_const(a.sp_table, desc[inst].scen);
#ifdef FOT_TIMELINE
    if (threadIdx.x == 0) s_tl_entry[1] = __builtin_amdgcn_s_memrealtime();
    __syncthreads();
#endif
    if (inst < 0) return;
    const int n_tiles = desc[inst].n_tiles;
    TilePart tp = tile_part_empty();
    evaluate_tile<TILE_WAVE, FOT_EVAL_LEAN, FOT_EVAL_FLAT, FOT_EVAL_WORDS>(Pp, desc, state, tile_cand0, tile_n, wave_rng, ent32, a, sp_lds, my_rows, inst,
                         n_tiles - 1 - pos, lane, x, tp);
    tile_done(inst, n_tiles - 1 - pos, lane, tp);
}
#endif

// The same for a handful of egos (fewer tiles than the GPU has SIMDs): a tile alone on its SIMD is a chain of
// ~50 dependent time steps of ~1.1 us, so the workgroup's waves (blockDim.x / 64 <= SEG_MAX) take a time segment
// each of ONE tile and its first wave merges them.  One workgroup per tile, same tile order.
__global__ void __launch_bounds__(SEG_MAX * WAVE)
FOT_EVAL_KERNEL(k_evaluate_split)(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc,
                 const InstState *__restrict__ state, const int32_t *__restrict__ tile_cand0,
                 const int32_t *__restrict__ tile_n, const TileStep *__restrict__ wave_rng,
                 const f2 *__restrict__ ent32, const EvalKernArgs a)
{
    const int n_seg = (int)blockDim.x / WAVE;
    const int wave_doubles = eval_wave_doubles(a.row_budget);
    // LDS: [rows | summaries | row offsets] of the tile, the segments' hand-over, then the spline
    double *s_part = s_lon + wave_doubles;
    const int seg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const int lane = threadIdx.x & (WAVE - 1);
    const int x = (int)blockIdx.x & (N_XCD - 1), q = (int)blockIdx.x >> 3;
    const int m_x = (a.n_inst - x + N_XCD - 1) / N_XCD;
    if (m_x <= 0) return;                                        // (the whole workgroup: one tile, one instance)
    if (q >= m_x * a.max_tiles) return;
    const int pos = q / m_x, j = q - pos * m_x;
    const int inst = x + N_XCD * j;
    const int n_tiles = desc[inst].n_tiles;
    if (pos >= n_tiles) return;
    SplineView sp_hbm = a.sp;
    if (a.mixed) { Pp += desc[inst].scen; sp_hbm = load_const(a.sp_table, desc[inst].scen); }
    const SplineView sp_lds = stage_spline(sp_hbm, a.lds_knots, s_part + (SEG_MAX - 1) * seg_doubles(FOT_EVAL_LEAN ? 1 : FOT_EVAL_WORDS));
    const int tile = n_tiles - 1 - pos;
    TilePart tp = tile_part_empty();
    evaluate_tile<TILE_SPLIT, FOT_EVAL_LEAN, FOT_EVAL_FLAT, FOT_EVAL_WORDS>(Pp, desc, state, tile_cand0, tile_n, wave_rng, ent32, a, sp_lds, s_lon, inst, tile, lane, x,
                              tp, seg, n_seg, s_part);
    if (seg == 0) tile_done(inst, tile, lane, tp);               // (the wave that merged the segments and holds the results)
}

// The grouped cut (fot_math.hpp): one workgroup per group of GROUP_TILES tiles, one shared row table, four such
// workgroups per CU -- four waves per SIMD.  Same order as above with groups in the place of tiles: queue x holds the
// groups of the instances x, x + 8, ... position-major, an instance's last group first.
#ifndef FOT_GROUP_WAVES
#define FOT_GROUP_WAVES 4
#endif
// (FOT_EVAL_GROUP_WAVES: FOT_GROUP_WAVES, but for the one inclusion that needs another figure -- see fot_kernels.hip)
#ifndef FOT_EVAL_GROUP_WAVES
#define FOT_EVAL_GROUP_WAVES FOT_GROUP_WAVES
#endif
__global__ void __launch_bounds__(GROUP_TILES * WAVE) __attribute__((amdgpu_waves_per_eu(FOT_EVAL_GROUP_WAVES, FOT_EVAL_GROUP_WAVES)))
FOT_EVAL_KERNEL(k_evaluate_group)(const DevParams *__restrict__ Pp, const InstDesc *__restrict__ desc,
                 const InstState *__restrict__ state, const int32_t *__restrict__ tile_cand0,
                 const int32_t *__restrict__ tile_n, const TileStep *__restrict__ wave_rng,
                 const f2 *__restrict__ ent32, const EvalKernArgs a)
{
#ifdef FOT_TIMELINE
    if (threadIdx.x == 0) s_tl_entry[0] = __builtin_amdgcn_s_memrealtime();
#endif
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const int lane = threadIdx.x & (WAVE - 1);
    const int x = (int)blockIdx.x & (N_XCD - 1), q = (int)blockIdx.x >> 3;
    const int m_x = (a.n_inst - x + N_XCD - 1) / N_XCD;
    const int n_pos = a.max_tiles / GROUP_TILES;                  // group positions of an instance
    const int n_entries = m_x * n_pos;                            // groups in this queue
    if (m_x <= 0 || q >= n_entries) return;                      // (the whole workgroup: one group, one instance)
    const int pos = q / m_x, j = q - pos * m_x;
    int inst = x + N_XCD * j;
    // (the general form: one register across the loop, not the two it is made of -- two lane-spilled SGPRs less; the
    //  lean form has room for both and its time step comes out two vector instructions shorter without this)
    if (!FOT_EVAL_LEAN) asm volatile("" : "+s"(inst));
    // LDS: the rows of the group, its header (GroupHead: k_frenet_state has built it), then the spline.  The header's
    // address follows from the arguments alone: one coalesced load, issued with the spline's, both behind ONE barrier.
    GroupHead *s_head = (GroupHead *)(s_lon + GROUP_ROWS * ROW_FIELDS);
    constexpr int HEAD_WORDS = (int)(sizeof(GroupHead) / sizeof(unsigned long long));
    static_assert(HEAD_WORDS <= GROUP_TILES * WAVE, "one 8-byte word per thread");
    const unsigned long long *head_src = (const unsigned long long *)(eval_kernargs().heads + ((int64_t)inst * n_pos + pos));
    unsigned long long head_word = 0ull;
    if ((int)threadIdx.x < HEAD_WORDS) head_word = head_src[threadIdx.x];
    SplineView sp_hbm = a.sp;
    if (a.mixed) { Pp += desc[inst].scen; sp_hbm = load_const(a.sp_table, desc[inst].scen); }
    double *s_knots = s_lon + eval_group_doubles();
    const bool staged = sp_hbm.n <= a.lds_knots;
    if (staged) stage_spline_copy(sp_hbm, s_knots);
    if ((int)threadIdx.x < HEAD_WORDS) ((unsigned long long *)s_head)[threadIdx.x] = head_word;
    __syncthreads();
#ifdef FOT_TIMELINE
    if (threadIdx.x == 0) s_tl_entry[1] = __builtin_amdgcn_s_memrealtime();   // header and spline in LDS
#endif
    const SplineView sp_lds = staged ? staged_spline_view(sp_hbm, s_knots) : sp_hbm;
    const int present = __builtin_amdgcn_readfirstlane(s_head->present);
    if (present == GROUP_HEAD_ABSENT) return;                    // a shorter lattice than the batch's longest: all waves
    const int tile0 = __builtin_amdgcn_readfirstlane(s_head->grp_tile0);
    TilePart tp = tile_part_empty();
    // (GROUP_HEAD_EMPTY -- no Frenet state, or the brake ladder of a standing ego: the tiles count as done, nothing found)
    evaluate_group_tile<FOT_EVAL_LEAN, FOT_EVAL_FLAT, FOT_EVAL_WORDS>(Pp, desc, wave_rng, ent32, a, sp_lds, s_lon, inst, tile0 + wv, wv, lane, x, tp,
                                       present == GROUP_HEAD_FULL);
    tile_done(inst, tile0 + wv, lane, tp);
}
#undef FOT_EVAL_GROUP_WAVES
