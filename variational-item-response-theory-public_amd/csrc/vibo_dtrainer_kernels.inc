// vibo_dtrainer_kernels.inc -- the four kernels of vibo_dtrainer.hip that exist once per posterior.  Included twice: DT_COND 0 gives
// dt_*_kernel(arg) for the unconditional posterior, DT_COND 1 gives dt_*_cond_kernel(arg, DCond c) for the conditional one.  The
// DT_COND 0 text is the unconditional kernels' own: whatever the conditional posterior needs sits inside #if DT_COND.
#if DT_COND
#define DT_KERNEL(name) name##_cond_kernel
#define DT_COND_ARG , const DCond c
#else
#define DT_KERNEL(name) name##_kernel
#define DT_COND_ARG
#endif

// ---- prologue --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDThreads) void DT_KERNEL(dt_prologue)(const DPrologue a) {
#if !DT_COND
    __shared__ float h1[2 * kDW], h2[2 * kDW];
#endif
    const int tid = threadIdx.x;
    const DParams& p = a.p;
    if (blockIdx.x == 0) {
        if (tid == 0) a.step_count[0] += 1;
#if DT_COND
        const int H = p.H;                            // (the table has 2 I rows: dt_table_fwd_kernel)
#else
        const int H = p.H, O = 2 * p.A;
        const MlpOffsets o = mlp_offsets(H, O);
        mlp2_layer0(a.P, o, H, O, h1, tid, kDThreads);
        __syncthreads();
        mlp2_layer1(a.P, o, H, O, h1, h2, tid, kDThreads);
        __syncthreads();
        mlp2_layer2(a.P, o, H, O, h1, h2, tid, kDThreads, a.table, a.saved_h);
#endif
        // the per-term network's second and third layer, 64 wide (decoder._pad_hidden)
        for (int e = tid; e < kDW * kDW; e += kDThreads) {
            const int j = e >> 6, k = e & 63;
            a.w2p[e] = (j < H && k < H) ? a.P[p.t2w + j * H + k] : 0.f;
        }
        if (tid < kDW) {
            const bool in = tid < H;
            a.b2p[tid] = in ? a.P[p.t2b + tid] : 0.f;
            a.w3p[tid] = in ? a.P[p.t4w + tid] : 0.f;
            a.w1p[tid] = (in && p.kind == VIBO_DECODER_LINK) ? a.P[p.t0w + tid] : 0.f;
            if (tid == 0) a.b3p[0] = a.P[p.t4b];
        }
        return;
    }
    if ((int)blockIdx.x > a.n_item_blocks) {          // ability noise (stream ab_stream)
        ability_noise_block(blockIdx.x - 1 - a.n_item_blocks, kDThreads, tid, a.eps_ab, a.n_ab, (uint32_t)a.step_count[1], a.ab_stream,
                            a.seed_lo, a.seed_hi);
        return;
    }
    item_prologue_block(blockIdx.x - 1, tid, a.I, p.D, a.mu, a.lv, a.eps, a.eps_w, a.gen, a.step_count + 1, a.seed_lo, a.seed_hi,
                        a.item_feat, a.kl_parts);
    if (a.guess != nullptr) {                         // 3PL: guess = sigmoid(item_feat[:, A + 1]) (this thread's own store)
        const int k = (blockIdx.x - 1) * 256 + tid;
        if (k < a.I * p.D) {
            const int idx = item_entry_index(k, a.I, p.D);
            if (idx % p.D == p.A + 1) a.guess[idx / p.D] = 1.0f / (1.0f + expf(-a.item_feat[idx]));
        }
    }
}

// ---- person side -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDThreads) void DT_KERNEL(dt_person_fwd)(const DPerson a DT_COND_ARG) {
    __shared__ float Ws[kDW * kDLd], Ts[kDRows * kDW];
    const DParams& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = p.H, A = p.A, D = p.D, I = a.I, wg = blockIdx.x;
    const int r16 = tid >> 4, a16 = tid & 15;
    for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
        const int row = t * kDRows + r16;
        if (row < a.nb && a16 < A) {
#if DT_COND
            const Poe q = cpoe_forward(c, row, a16, a.counts[row], I, a.prior);
#else
            const Poe q = poe_forward(a.counts[row], a.table, A, a16, I, a.prior);
#endif
            const float mu = q.smu / q.lam, lv = logf(1.0f / q.lam);
            a.post[(size_t)row * 2 * A + a16] = mu;
            a.post[(size_t)row * 2 * A + A + a16] = lv;
            a.ability[(size_t)row * A + a16] = fmaf(expf(0.5f * lv), a.eps[(size_t)row * A + a16], mu);
        }
    }
    if (p.kind == VIBO_DECODER_LINK) {
        for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
            for (int e = tid; e < kDRows * kDW; e += kDThreads) {
                const int row = t * kDRows + (e >> 6), j = e & 63;
                if (row < a.nb) a.V[(size_t)row * kDW + j] = j < H ? a.P[p.t0b + j] : 0.f;
            }
        }
    } else {
        // (fwd_layer starts with a barrier: this workgroup's ability rows are visible to all of its threads)
        fwd_layer(Ws, Ts, a.P + p.fa.w0, A, H, A, a.P + p.fa.b0, a.ability, A, A, a.h1, a.nb, true, wg, a.nwg);
        fwd_layer(Ws, Ts, a.P + p.fa.w1, H, H, H, a.P + p.fa.b1, a.h1, kDW, kDW, a.h2, a.nb, true, wg, a.nwg);
        fwd_layer(Ws, Ts, a.P + p.fa.w2, H, H, H, a.P + p.fa.b2, a.h2, kDW, kDW, a.hid, a.nb, false, wg, a.nwg);
        fwd_layer(Ws, Ts, a.P + p.t0w + H, 2 * H, H, H, a.P + p.t0b, a.hid, kDW, kDW, a.V, a.nb, false, wg, a.nwg);
    }
    if (a.L != nullptr) {                             // decoder.irt_logit: a wave per row, lanes over the items
        __syncthreads();
        for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
            for (int rr = 0; rr < 4; ++rr) {
                const int row = t * kDRows + 4 * w + rr;
                if (row >= a.nb) continue;
                const float* ab = a.ability + (size_t)row * A;
                for (int i = lane; i < I; i += 64) {
                    float s;
                    if (a.irt == VIBO_IRT_1PL) {
                        s = 0.f;
                        for (int q = 0; q < A; ++q) s += ab[q];
                        s += a.item_feat[i];
                    } else {
                        s = 0.f;
                        for (int q = 0; q < A; ++q) s = fmaf(ab[q], -a.item_feat[(size_t)i * D + q], s);
                        s += a.item_feat[(size_t)i * D + A];
                    }
                    a.L[(size_t)row * I + i] = s;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kDThreads) void DT_KERNEL(dt_person_bwd)(const DPerson a DT_COND_ARG) {
    __shared__ float Ws[kDW * kDLd], Tin[kDRows * kDW], Td[kDRows * kDW];
    __shared__ float gl[kDRows * 16], wsum[4];
    const DParams& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = p.H, A = p.A, D = p.D, I = a.I, wg = blockIdx.x;
    float* rec = a.rec + (size_t)wg * a.rec_stride;
    // d LL / d V = the fixed-order sum of the decoder kernel's records
    float vb = 0.f;                                   // link: d link[0].bias = sum over the persons (column tid & 63, rows w, w + 4, ...)
    for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
        for (int e = tid; e < kDRows * kDW; e += kDThreads) {
            const int row = t * kDRows + (e >> 6), j = e & 63;
            if (row >= a.nb) continue;
            float s = 0.f;
            for (int k = 0; k < a.n_dv; ++k) s += a.dV[((size_t)k * a.nb + row) * kDW + j];
            a.da[(size_t)row * kDW + j] = s;
            vb += s;
        }
    }
    if (p.kind == VIBO_DECODER_LINK) {
        __syncthreads();
        Td[tid] = vb;
        __syncthreads();
        if (tid < H) rec[a.r_vb + tid] = (Td[tid] + Td[64 + tid]) + (Td[128 + tid] + Td[192 + tid]);
    } else {
        float* rf = rec + a.r_fa - p.fa.w0;           // (mlp_ability in its parameter layout)
        bwd_layer(Ws, Tin, Td, a.P + p.t0w + H, 2 * H, H, H, a.da, a.hid, kDW, kDW, false, a.db, kDW, a.nb, rec + a.r_wcp, H, rec + a.r_vb, wg,
                  a.nwg);
        bwd_layer(Ws, Tin, Td, a.P + p.fa.w2, H, H, H, a.db, a.h2, kDW, kDW, true, a.da, kDW, a.nb, rf + p.fa.w2, H, rf + p.fa.b2, wg, a.nwg);
        bwd_layer(Ws, Tin, Td, a.P + p.fa.w1, H, H, H, a.da, a.h1, kDW, kDW, true, a.db, kDW, a.nb, rf + p.fa.w1, H, rf + p.fa.b1, wg, a.nwg);
        bwd_layer(Ws, Tin, Td, a.P + p.fa.w0, A, H, A, a.db, a.ability, A, A, false, a.gab, A, a.nb, rf + p.fa.w0, A, rf + p.fa.b0, wg, a.nwg);
    }
    // d LL / d ability -> (mu, logvar) -> the 2-row table; KL and its gradient.  Thread (r16, a16) = (row of the tile, dimension).
    const int r16 = tid >> 4, a16 = tid & 15;
    float tg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // [set][c][mu | logvar] of dimension a16
    float kl = 0.f;
    for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
        __syncthreads();
#if DT_COND
        for (int e = tid; e < kDRows * kDW; e += kDThreads) {      // the columns of d [lambda | s] no dimension writes
            const int row = t * kDRows + (e >> 6), j = e & 63;
            if (row < a.nb && j >= 4 * A) c.dsum[(size_t)row * kDW + j] = 0.f;
        }
#endif
        if (a.dL != nullptr) {                        // gl[r][q] = sum_i d L[row][i] (-item[i][q]): a wave per row, lanes over the items
            for (int rr = 0; rr < 4; ++rr) {
                const int r = 4 * w + rr, row = t * kDRows + r;
                float acc[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = 0.f;
                if (row < a.nb) {
                    for (int i = lane; i < I; i += 64) {
                        const float g = a.dL[(size_t)row * I + i];
                        if (a.irt == VIBO_IRT_1PL) {
                            acc[0] += g;
                        } else {
#pragma unroll
                            for (int q = 0; q < 16; ++q)
                                if (q < A) acc[q] = fmaf(g, -a.item_feat[(size_t)i * D + q], acc[q]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (q < A) {
                        const float s = wave_total(acc[a.irt == VIBO_IRT_1PL ? 0 : q]);
                        if (lane == 0) gl[r * 16 + q] = s;
                    }
                }
            }
        }
        __syncthreads();
        const int row = t * kDRows + r16;
        if (row < a.nb && a16 < A) {
            float g = p.kind == VIBO_DECODER_LINK ? 0.f : a.gab[(size_t)row * A + a16];
            if (a.dL != nullptr) g += gl[r16 * 16 + a16];
#if DT_COND
            const Poe q = cpoe_forward(c, row, a16, a.counts[row], I, a.prior);
#else
            const Poe q = poe_forward(a.counts[row], a.table, A, a16, I, a.prior);
#endif
            const float mu = a.post[(size_t)row * 2 * A + a16], lv = a.post[(size_t)row * 2 * A + A + a16];
            const float var = expf(lv);
            kl += -0.5f * (1.0f + lv - mu * mu - var);
            const float inv = 1.0f / q.lam;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // set 0: d LL through the sample; set 1: d KL
                const float dmu = s == 0 ? g : mu;
                const float dlv = s == 0 ? g * a.eps[(size_t)row * A + a16] * (0.5f * expf(0.5f * lv)) : 0.5f * (var - 1.0f);
                const float dsmu = dmu * inv;
                const float dlam = -fmaf(dmu, mu, dlv) * inv;
#if DT_COND
                // mu = s / lambda, logvar = -log lambda: the table comes behind the sums (tg stays 0)
                c.dsum[(size_t)row * kDW + 2 * A * s + a16] = dlam;
                c.dsum[(size_t)row * kDW + 2 * A * s + A + a16] = dsmu;
#else
                tg[4 * s + 0] += q.n0 * q.tau0 * dsmu;
                tg[4 * s + 1] += q.n0 * fmaf(dsmu, q.m0, dlam) * (-q.e0 * q.tau0 * q.tau0);
                tg[4 * s + 2] += q.n1 * q.tau1 * dsmu;
                tg[4 * s + 3] += q.n1 * fmaf(dsmu, q.m1, dlam) * (-q.e1 * q.tau1 * q.tau1);
#endif
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 8; ++v) Ws[tid * 8 + v] = tg[v];
    kl = wave_total(kl);
    if (lane == 0) wsum[w] = kl;
    __syncthreads();
    if (tid < 8 * A) {
        const int v = tid / A, q = tid % A;
        float s = 0.f;
        for (int r = 0; r < kDRows; ++r) s += Ws[(r * 16 + q) * 8 + v];
        // v = 4 set + 2 c + part -> grad_table layout [set][c][part A + q]
        rec[a.r_tab + (v >> 2) * 4 * A + ((v >> 1) & 1) * 2 * A + (v & 1) * A + q] = s;
    }
    if (tid == 0) rec[a.r_kl] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ---- epilogue --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEpiThreads) void DT_KERNEL(dt_epilogue)(const DEpilogue a DT_COND_ARG) {
#if !DT_COND
    __shared__ EpiLds L;
#endif
    const int tid = threadIdx.x;
    const DParams& p = a.p;
    const DRec& r = a.r;
    const float beta = *a.beta, lr = *a.lr;
    const AdamBias bc = adam_bias(a.step_count[0]);
    constexpr int BS = kEpiThreads;
    const int H = p.H;
    if (blockIdx.x == 0) {
        if (tid == 0) a.step_count[1] += 1;           // completed steps: the noise counter of the NEXT step
#if DT_COND
        // the loss; the encoder's gradient is the reduced table records (c.s_enc), applied by the parameter blocks below
        item_kl_loss(tid, a.kl_parts, kl_part_count(a.n_item_entries), a.flat8, beta, a.loss);
#else
        // the 2-row encoder: sc = [LL, KL_ability, ...], gtab = d LL / d table then d KL / d table (the person records' sums)
        float pv[kEpiU], mv[kEpiU], vv[kEpiU];
        const MlpOffsets o = mlp_offsets(H, 2 * p.A);
        epi_mlp_prefetch(o.total, a.P, a.M, a.V, pv, mv, vv, tid);
        if (H == 64) epi_mlp_block<64>(L, H, 2 * p.A, kl_part_count(a.n_item_entries), a.flat8, a.s_p + r.tab, a.saved_h, a.kl_parts, beta, lr,
                                       bc, a.P, o, nullptr, a.P, a.M, a.V, pv, mv, vv, a.loss, tid);
        else epi_mlp_block<0>(L, H, 2 * p.A, kl_part_count(a.n_item_entries), a.flat8, a.s_p + r.tab, a.saved_h, a.kl_parts, beta, lr, bc,
                              a.P, o, nullptr, a.P, a.M, a.V, pv, mv, vv, a.loss, tid);
#endif
        return;
    }
    if ((int)blockIdx.x <= a.n_dec_blocks) {          // Adam on the decoder parameters: d loss = -d LL
#if DT_COND
        const int k = ((int)blockIdx.x - 1) * BS + tid;            // (the encoder's parameters too)
#else
        const int k = p.dec + ((int)blockIdx.x - 1) * BS + tid;
#endif
        if (k >= p.total) return;
        float g;
#if DT_COND
        if (k < p.enc) {
            g = -c.s_enc[k];                          // (records of d loss: adam_update below takes -g)
        } else
#endif
        if (k >= p.t2w) {                             // the per-term network's second and third layer: the decoder kernel's records
            if (k < p.t2b) {
                const int e = k - p.t2w;
                g = a.s_dW2[(e / H) * kDW + e % H];
            } else if (k < p.t4w) {
                g = a.s_dvec[k - p.t2b];
            } else if (k < p.t4b) {
                g = a.s_dvec[kDW + (k - p.t4w)];
            } else {
                g = a.s_dvec[3 * kDW];
            }
        } else if (p.kind == VIBO_DECODER_LINK) {
            g = k < p.t0b ? a.s_dvec[2 * kDW + (k - p.t0w)] : a.s_p[r.vb + (k - p.t0b)];
        } else if (k >= p.t0b) {
            g = a.s_p[r.vb + (k - p.t0b)];
        } else if (k >= p.fa.w0 && k < p.t0w) {
            g = a.s_p[r.fa + (k - p.fa.w0)];
        } else {
            // mlp_item_feat, or the item half of mlp_concat[0].weight: the item workgroups' records, in order
            int e;
            if (k < p.fa.w0) {
                e = r.fi + (k - p.fi.w0);
            } else {
                const int j = (k - p.t0w) / (2 * H), c = (k - p.t0w) % (2 * H);
                e = c < H ? r.wci + j * H + c : -1;
                if (e < 0) g = a.s_p[r.wcp + j * H + (c - H)];
            }
            if (e >= 0) {
                g = 0.f;
                for (int q = 0; q < a.n_irec; ++q) g += a.irec[(size_t)q * r.itotal + e];
            }
        }
        float pv = a.P[k], mv = a.M[k], vv = a.V[k];
        adam_update(pv, mv, vv, -g, lr, bc);
        a.P[k] = pv; a.M[k] = mv; a.V[k] = vv;
        return;
    }
    const int idx = ((int)blockIdx.x - 1 - a.n_dec_blocks) * BS + tid;
    if (idx < a.n_item_entries) {                     // d loss / d item_feat = -d LL / d item_feat
        float g = 0.f;
        if (a.has_l) g += a.s_ditem[idx];
        if (a.gx != nullptr) g += a.gx[idx];
        if (a.has_g && idx % p.D == p.A + 1) {
            const float gs = a.guess[idx / p.D];
            g += a.s_dguess[idx / p.D] * gs * (1.0f - gs);
        }
#if DT_COND
        {                                             // the encoder reads the item sample: rows (0, i) and (1, i) of the table
            const int i = idx / p.D, q = idx % p.D, xin = p.D + 1;
            g -= c.gx[(size_t)i * xin + 1 + q] + c.gx[(size_t)(a.I + i) * xin + 1 + q];
        }
#endif
        float pm, pl;
        epi_item_update(idx, a.n_item_entries, -g, a.eps[idx], beta, lr, bc, a.mu, a.lv, a.im, a.iv, pm, pl);
    }
}

#undef DT_KERNEL
#undef DT_COND_ARG
