// fot_pred_scores_body.inc -- the body of k_pred_scores and k_pred_scores_wide (fot_loop_kernels.hip), included once by
// each with PS_ROWS defined: the rows of the per-sample tables in LDS (S <= PS_ROWS, checked by the host).  One text, so
// that the two kernels cannot drift apart and the narrow one stays, instruction for instruction, what it was before the
// wide one existed (a shared device function came out of the inliner with two instructions swapped).
// In scope: TO, desc, tensor, stride, E, truth, out.
    __shared__ double s_g[PS_TILE_PAIRS * 2];
    __shared__ double s_scene[2][PS_ROWS][PS_WAVES];
    __shared__ double s_part[3][PS_WAVES];
    const PredOriginDev D = desc[blockIdx.x];
    const int S = D.S, P = D.P, T = D.T, skip = D.skip, tmajor = D.tmajor;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if (P <= 0) {                                                    // (uniform)
        if (tid == 0) {
            fot_pred_score r;
            r.ade_scene = r.fde_scene = r.ade_agent_sum = r.fde_agent_sum = r.log_lik_sum = 0.0;
            r.n_peds = 0; r.n_samples = S; r.nll_count = 0; r.flags = 0;
            out[blockIdx.x] = r;
        }
        return;
    }
    const TO *base = tensor + 2 * D.offset;
    auto at = [&](int s, int p, int k) {                             // dense sample k: the prepended entry skipped
        const int kk = k + skip;
        return base + (tmajor ? ((int64_t)kk * S + s) * P + p : ((int64_t)s * P + p) * T + kk) * 2;
    };
    for (int i = tid; i < 2 * PS_ROWS * PS_WAVES; i += PS_THREADS) (&s_scene[0][0][0])[i] = 0.0;
    const int tile_peds = P < PS_TILE_PAIRS / E ? P : PS_TILE_PAIRS / E;
    double agent_a = 0.0, agent_f = 0.0, ll = 0.0;
    int varies = 0, nonfinite = 0;
    for (int p0 = 0; p0 < P; p0 += tile_peds) {
        const int np = P - p0 < tile_peds ? P - p0 : tile_peds;
        __syncthreads();                                             // the tile before is done with s_g (first: the zeros)
        const double *g_src = truth + ((int64_t)D.truth_row + p0) * E * 2;
        for (int i = tid; i < np * E * 2; i += PS_THREADS) {
            const double v = g_src[i];
            nonfinite |= !ps_finite(v);
            s_g[i] = v;
        }
        __syncthreads();
        // ---- displacement terms: lanes over the tile's pedestrians
        for (int c = 0; c < np; c += PS_THREADS) {                   // (every lane takes every turn: the butterflies)
            const int pl = c + tid, p = p0 + pl;
            const bool active = pl < np;
            double best_a = 0.0, best_f = 0.0;
            for (int s = 0; s < S; ++s) {
                double row = 0.0, last = 0.0;
                if (active)
                    for (int j = 0; j < E; ++j) {
                        const TO *e = at(s, p, stride * (j + 1) - 1);
                        const double qx = (double)e[0], qy = (double)e[1];
                        nonfinite |= !ps_finite(qx) || !ps_finite(qy);
                        last = ps_dist(qx, qy, s_g[(pl * E + j) * 2], s_g[(pl * E + j) * 2 + 1]);
                        row += last;
                    }
                const double a = row / (double)E;
                best_a = s == 0 ? a : ps_min(best_a, a);
                best_f = s == 0 ? last : ps_min(best_f, last);
                const double w_row = wave_sum_f64(row), w_last = wave_sum_f64(last);
                if (lane == 0) { s_scene[0][s][wave] += w_row; s_scene[1][s][wave] += w_last; }
            }
            agent_a += best_a; agent_f += best_f;                    // (a lane past the tile: 0.0)
        }
        // ---- KDE terms: lanes over the tile's (p, j) pairs
        if (S >= 2)
            for (int i = tid; i < np * E; i += PS_THREADS) {
                const int pl = i / E, j = i - pl * E, p = p0 + pl, k = stride * (j + 1) - 1;
                auto qx = [&](int s) { return (double)at(s, p, k)[0]; };
                auto qy = [&](int s) { return (double)at(s, p, k)[1]; };
                bool vx, vy;
                const double bx = ps_bandwidth(S, D.scott, qx, &vx), by = ps_bandwidth(S, D.scott, qy, &vy);
                varies |= vx || vy;
                ll += ps_log_p(S, qx, qy, s_g[i * 2], s_g[i * 2 + 1], bx, by);
            }
    }
    const double w_a = wave_sum_f64(agent_a), w_f = wave_sum_f64(agent_f), w_l = wave_sum_f64(ll);
    if (lane == 0) { s_part[0][wave] = w_a; s_part[1][wave] = w_f; s_part[2][wave] = w_l; }
    varies = __syncthreads_or(varies);                               // (also orders s_part and s_scene for thread 0)
    nonfinite = __syncthreads_or(nonfinite);
    if (tid != 0) return;
    double tot[3];
    for (int q = 0; q < 3; ++q) {
        tot[q] = s_part[q][0];
        for (int w = 1; w < PS_WAVES; ++w) tot[q] += s_part[q][w];
    }
    fot_pred_score r;
    r.ade_scene = r.fde_scene = 0.0;
    for (int s = 0; s < S; ++s) {
        double a = s_scene[0][s][0], f = s_scene[1][s][0];
        for (int w = 1; w < PS_WAVES; ++w) { a += s_scene[0][s][w]; f += s_scene[1][s][w]; }
        a /= (double)P * (double)E; f /= (double)P;
        r.ade_scene = s == 0 ? a : ps_min(r.ade_scene, a);
        r.fde_scene = s == 0 ? f : ps_min(r.fde_scene, f);
    }
    r.ade_agent_sum = tot[0]; r.fde_agent_sum = tot[1];
    r.log_lik_sum = varies ? tot[2] : 0.0;
    r.n_peds = P; r.n_samples = S;
    r.nll_count = varies ? P * E : 0;
    r.flags = (varies ? PS_FLAG_NLL : 0) | (nonfinite ? PS_FLAG_NONFINITE : 0);
    out[blockIdx.x] = r;
