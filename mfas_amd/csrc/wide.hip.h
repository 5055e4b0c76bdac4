// wide.hip.h — the WIDE path: batch sizes and widths whose activations do not fit the LDS of one workgroup (plan.hip.h decides:
// exactly the geometries the chain_body / sweep_body schedules cannot hold).  Two plain kernels, launch per phase — chain, then
// sweep — that LOOP OVER THE BATCH: kernel boundaries carry every dependency, no workgroup ever waits for another one.
//   k_chain_wide  one 8-wave workgroup per candidate; a wave owns 16-column blocks of the cell and walks the batch in 16-row tiles
//                 (two staged at a time); out_i / dy_i / saved activations / x-hat / dlogits live in the candidate's step buffers.
//   k_sweep_wide  one workgroup per (candidate, segment, column chunk, row-block group): a wave owns ONE row block and the chunk's
//                 <= 8 k-blocks, whose dW tiles stay in registers while the batch is staged in slices of <= 64 rows.
// Same arithmetic, in the same order, as chain_body / tile_run (activation before BN, biased variance to normalise, unbiased for
// the running statistics, hash dropout indexed (cell, batch row * R + column, step)); the tile images, adam4, the transposed wt
// image and the partial-slab format are the existing ones (common.hip.h, sweep.hip.h).
// (part of the single translation unit mfas_hip.hip; see the header comment there and DESIGN.md)
#pragma once

// (WIDE_SLICE, WIDE_KB, WIDE_RBG, WIDE_TROWS and the LDS floats of k_chain_wide, wide_chain_lds_floats: records.hip.h — the kernel lays
//  its buffers out in the formula's order; k_sweep_wide takes its buffers from wide_sweep_lds, lds.hip.h)

// Softmax cross-entropy of the <= 32 staged rows (batch rows row0 ...), 16 lanes per row, <= 16 classes per lane (C <= 256): the
// arithmetic of softmax_rows_nc (chain.hip.h) at any batch size.  dlogits = (softmax - onehot) / nvalid in place, the row's loss in
// red[b], its top-1 hit in red[Bp + b] (multitask: argmax of central + visual + skeleton logits).
__device__ __forceinline__ void wide_softmax_rows(const ChainArgs& a, const ChainStep& cs, float* lg_l, const int SC, float* red_l,
                                                  const int row0, const int nvalid, const float nf, const int tid, const int32_t* ord) {
    constexpr int NC = 16, LPR = 16;
    const Geo& g = a.g;
    const int C = g.C, Cp = g.Cp, Bp = g.Bp;
    const int bl = tid >> 4, sub = tid & 15, b = row0 + bl;
    float* row = lg_l + bl * SC;
    const bool ok = b < nvalid;
    int64_t grow = 0;
    int lab = 0;
    if (ok) {
        grow = ord ? (int64_t)ord[cs.pos_t + b] : (int64_t)(cs.base_t + b);
        lab = a.tab.label[grow];
    }
    float xv[NC], ev[NC];
    float mx = -3.0e38f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = sub + j * LPR;
        xv[j] = c < C ? row[c] : -3.0e38f;
        mx = fmaxf(mx, xv[j]);
    }
    mx = row_max<LPR>(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = sub + j * LPR;
        ev[j] = c < C ? expf(xv[j] - mx) : 0.f;
        se += ev[j];
    }
    se = row_sum<LPR>(se);
    float bv = -3.0e38f;
    int bi = 0x7FFFFFFF;
    const float* vl = nullptr;
    const float* sl = nullptr;
    if (g.multitask && ok) {
        vl = a.tab.vlogit + grow * C;
        sl = a.tab.slogit + grow * C;
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = sub + j * LPR;
        if (c < C) {
            float t = xv[j];
            if (vl) t = (t + vl[c]) + sl[c];
            if (t > bv) { bv = t; bi = c; }
        }
    }
    row_argmax<LPR>(bv, bi);
    const float lse = mx + logf(se);
    if (sub == 0 && b < Bp) {
        float ls = ok ? -(row[lab] - lse) : 0.f;
        if (vl) ls = (ls + row_ce(vl, C, lab)) + row_ce(sl, C, lab);
        red_l[b] = ls;
        red_l[Bp + b] = (ok && bi == lab) ? 1.f : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = sub + j * LPR;
        if (c < Cp) {
            float dl = 0.f;
            if (ok && c < C) {
                dl = ev[j] / se;
                if (c == lab) dl -= 1.0f;
                dl = dl / nf;
            }
            row[c] = dl;
        }
    }
}

// WeightedCrossEntropyWithLogits of the staged rows (bce_rows' arithmetic, chain.hip.h; 16 lanes per row): the mean runs over the
// REAL rows of the whole batch (nvalid), not over the rows staged
__device__ __forceinline__ void wide_bce_rows(const ChainArgs& a, const ChainStep& cs, float* lg_l, const int SC, float* red_l,
                                              const int row0, const int nvalid, const int tid, const int32_t* ord) {
    const Geo& g = a.g;
    const int C = g.C, Cp = g.Cp, Bp = g.Bp;
    const int bl = tid >> 4, sub = tid & 15, b = row0 + bl;
    float* row = lg_l + bl * SC;
    const bool ok = b < nvalid;
    const float* z = nullptr;
    if (ok) z = a.tab.multilabel + (ord ? (int64_t)ord[cs.pos_t + b] : (int64_t)(cs.base_t + b)) * C;
    float ls = 0.f;
    const float inv = 1.0f / ((float)nvalid * (float)C);
    for (int c = sub; c < Cp; c += 16) {
        float dl = 0.f;
        if (ok && c < C) {
            const float sg = 1.0f / (1.0f + expf(-row[c]));
            const float zz = z[c], w = a.pos_w[c];
            ls += w * zz * -logf(sg) + (1.0f - zz) * -logf(1.0f - sg);
            dl = (-w * zz * (1.0f - sg) + (1.0f - zz) * sg) * inv;
        }
        row[c] = dl;
    }
    ls = row_sum<16>(ls);
    if (sub == 0 && b < Bp) {
        red_l[b] = ls / (float)C;
        red_l[Bp + b] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// k_chain_wide — forward chain, loss, backward chain and the Adam step of the vector parameters of ONE candidate at any batch
// size: wave w owns the 16-column blocks w, w + 8, ... of every cell, so a column's batch statistics never leave the wave.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(STEP_THREADS, 2) k_chain_wide(const ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ChainStep cs = chain_step_of(a);
    const CandDev& cd = a.cands[blockIdx.x];
    const Geo& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int Rp = g.Rp, nrb = g.nrb, Cp = g.Cp, ncb = g.ncb, R = g.R, C = g.C, L = cd.L, MB = g.MB, Bp = g.Bp;
    const int SX = (Rp > Cp ? Rp : Cp) + 4, SC = Cp + 4;
    constexpr int RBW = 4;                       // row blocks per wave (Rp <= 512)
    float* xt_l = lds;                           // [32][SX]  the A operand's rows in flight: out_{i-1} / dy_{i+1} / dlogits
    float* lg_l = xt_l + WIDE_TROWS * SX;        // [32][SC]  logits -> dlogits of the rows in flight
    float* rstd_l = lg_l + WIDE_TROWS * SC;      // [L][Rp]
    float* red_l = rstd_l + MFAS_MAX_CELLS * Rp; // [2 Bp] loss / correct per row, then [8] alpha partials
    const int64_t sav_plane = (int64_t)MFAS_MAX_CELLS * nrb * MB * 256;
    float* W = a.plane;
    float* Mv = a.plane + a.plane_stride;
    float* Vv = Mv + a.plane_stride;
    float* sb = a.stepbuf + cd.step_off;
    float* sav = sb + g.sb_sav;                  // [3][L][nrb][MB][256]: act, xhat, (yS - yV)
    const int64_t cvec_off = cd.vec_off;
    const float* vecW = W + cvec_off;
    const float* vecM = Mv + cvec_off;
    const float* vecV = Vv + cvec_off;
    const int cgidx = cd.gidx;
    const int nvalid = cs.nvalid;
    const float nf = (float)nvalid;
    const AdamC ac = adam_consts(a.ac, cs.ss, cs.bc2s);
    const uint32_t h0 = lowbias32(cd.drop_seed + 0x9E3779B9U * (uint32_t)(cs.gstep + 1));
    const int32_t* ord = cand_order(a.order, g, cgidx);
    const int npair = (MB + 1) >> 1;

    // rows row0 .. row0 + 31 of a row-major [Bp][src_stride] step buffer -> xt_l (rows beyond the padded batch: zeros)
    auto stage_rows = [&](const float* src, const int src_stride, const int ncols, const int row0) {
        const int vpr = ncols >> 2;
        for (int e = tid; e < WIDE_TROWS * vpr; e += CHAIN_THREADS) {
            const int b = e / vpr, c = (e - b * vpr) << 2;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row0 + b < Bp) v = *reinterpret_cast<const f32x4*>(src + (int64_t)(row0 + b) * src_stride + c);
            *reinterpret_cast<f32x4*>(xt_l + b * SX + c) = v;
        }
    };

    // ------------------------------------------------------------------ forward chain
    for (int i = 0; i < L; ++i) {
        const int nl = cd.conf[i][2] & 3;
        const int64_t vb = cvec_off + (int64_t)i * g.vec_cell_stride;
        const int vbl = i * g.vec_cell_stride;
        float sgS = 1.0f, sgV = 1.0f;
        if (g.alphas) {
            const float sg = 1.0f / (1.0f + expf(-vecW[vbl + 5 * Rp]));
            sgS = sg;
            sgV = 1.0f - sg;
            if (tid == 0) { sb[g.sb_gsc + i * 2] = sgS; sb[g.sb_gsc + i * 2 + 1] = sgV; }
        }
        const int ns = cd.nch_s[i], nch = ns + cd.nch_v[i];
        const float* part0 = sb + g.sb_part + (((int64_t)cd.part_cell_off[i] * nrb * MB) << 8) + lane * 4;
        float s_[RBW] = {0.f, 0.f, 0.f, 0.f};
        // pass 1 over the row tiles: y = feature sums + out_{i-1} W_out^T + b, activation (saved), column sums
        for (int p = 0; p < npair; ++p) {
            if (i > 0) {
                __syncthreads();     // (p == 0: out_{i-1} is out; later: the previous rows have been consumed)
                stage_rows(sb + g.sb_xo + (int64_t)(i - 1) * Bp * Rp, Rp, Rp, p * WIDE_TROWS);
                __syncthreads();
            }
#pragma unroll
            for (int rbi = 0; rbi < RBW; ++rbi) {
                const int rb = wave + rbi * CHAIN_NW;
                if (rb < nrb) {
                    const float bias = vecW[vbl + VEC_B * Rp + rb * 16 + l15];
                    f32x4 acc[2];
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int mb = 2 * p + t;
                        acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                        if (mb < MB) {      // the sweep's column-chunk partial sums, fixed order (chain_body's phase 0)
                            const int64_t o = ((((int64_t)i * nrb + rb) * MB + mb) << 8) + lane * 4;
                            const float* part = part0 + ((rb * MB + mb) << 8);
                            f32x4 accS = {0.f, 0.f, 0.f, 0.f}, accV = {0.f, 0.f, 0.f, 0.f};
                            for (int ch = 0; ch < nch; ++ch) {
                                const f32x4 p4 = *reinterpret_cast<const f32x4*>(part + (((int64_t)ch * nrb * MB) << 8));
                                if (ch < ns) accS += p4; else accV += p4;
                            }
                            if (g.alphas) {
                                *reinterpret_cast<f32x4*>(sav + 2 * sav_plane + o) = accS - accV;
                                acc[t] = accS * sgS + accV * sgV;
                            } else acc[t] = accS + accV;
                        }
                    }
                    if (i > 0) lds_x_times_tiles<2, false, 8>(acc, xt_l, SX, W, cd.seg_off[i][2] + (int64_t)rb * nrb * 256, 256, nrb, lane);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int mb = 2 * p + t;
                        if (mb < MB) {
                            f32x4 a4;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int b = mb * 16 + 4 * lg + q;
                                const float v = act_fwd(acc[t][q] + bias, nl);
                                a4[q] = v;
                                if (b < nvalid) s_[rbi] += v;
                            }
                            *reinterpret_cast<f32x4*>(sav + ((((int64_t)i * nrb + rb) * MB + mb) << 8) + lane * 4) = a4;
                        }
                    }
                }
            }
        }
        // passes 2 and 3 (a wave re-reads what its own lanes saved): variance about the mean, then normalise + dropout -> out_i
#pragma unroll
        for (int rbi = 0; rbi < RBW; ++rbi) {
            const int rb = wave + rbi * CHAIN_NW;
            if (rb < nrb) {
                const int r = rb * 16 + l15;
                const bool colok = r < R;
                const float* sav_a = sav + ((((int64_t)i * nrb + rb) * MB) << 8) + lane * 4;
                float gam = 1.f, bet = 0.f, mu = 0.f, rstd = 1.f;
                if (g.bn) {
                    gam = vecW[vbl + VEC_G * Rp + r]; bet = vecW[vbl + VEC_BE * Rp + r];
                    mu = colsum(s_[rbi]) / nf;
                    float s2 = 0.f;
                    for (int mb = 0; mb < MB; ++mb) {
                        const f32x4 a4 = *reinterpret_cast<const f32x4*>(sav_a + (mb << 8));
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int b = mb * 16 + 4 * lg + q;
                            const float dlt = a4[q] - mu;
                            if (b < nvalid) s2 += dlt * dlt;
                        }
                    }
                    const float var = colsum(s2) / nf;
                    rstd = 1.0f / sqrtf(var + g.bn_eps);
                    if (lg == 0) {
                        rstd_l[i * Rp + r] = rstd;
                        if (colok) {   // running stats: momentum 0.1, unbiased variance
                            float rm = vecW[vbl + VEC_RM * Rp + r], rv = vecW[vbl + VEC_RV * Rp + r];
                            const float unb = var * (nf / (nf - 1.0f));
                            rm += g.bn_mom * (mu - rm);
                            rv += g.bn_mom * (unb - rv);
                            W[vb + VEC_RM * Rp + r] = rm;
                            W[vb + VEC_RV * Rp + r] = rv;
                        }
                    }
                }
                float* xo_g = sb + g.sb_xo + (int64_t)i * Bp * Rp;
                for (int mb = 0; mb < MB; ++mb) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(sav_a + (mb << 8));
                    f32x4 z4 = a4;
                    if (g.bn) {
                        f32x4 xh4;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float xh = (a4[q] - mu) * rstd;
                            xh4[q] = xh;
                            z4[q] = xh * gam + bet;
                        }
                        *reinterpret_cast<f32x4*>(sav + sav_plane + ((((int64_t)i * nrb + rb) * MB + mb) << 8) + lane * 4) = xh4;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int b = mb * 16 + 4 * lg + q;
                        float o = z4[q];
                        if (g.use_drop) o = drop_keep(h0, i, (uint32_t)(b * R + r), g.drop_thr) ? o * g.drop_scale : 0.0f;
                        if (!(colok && b < nvalid)) o = 0.0f;
                        xo_g[(int64_t)b * Rp + r] = o;
                    }
                }
            }
        }
    }

    // ------------------------------------------------------------------ head + loss, 32 rows at a time
    for (int p = 0; p < npair; ++p) {
        const int row0 = p * WIDE_TROWS;
        __syncthreads();
        stage_rows(sb + g.sb_xo + (int64_t)(L - 1) * Bp * Rp, Rp, Rp, row0);
        __syncthreads();
        for (int cb = wave; cb < ncb; cb += CHAIN_NW) {
            f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
            const int c = cb * 16 + l15;
            const float bias = vecW[g.vec_head + c];
            lds_x_times_tiles<2, false, 8>(acc, xt_l, SX, W, cd.head_off + (int64_t)cb * nrb * 256, 256, nrb, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) lg_l[(t * 16 + 4 * lg + q) * SC + c] = acc[t][q] + bias;
        }
        __syncthreads();
        if (a.logits_out) {   // train-mode forward only
            for (int e = tid; e < WIDE_TROWS * C; e += CHAIN_THREADS) {
                const int bl = e / C, c = e - bl * C;
                if (row0 + bl < nvalid) a.logits_out[(int64_t)(row0 + bl) * C + c] = lg_l[bl * SC + c];
            }
            continue;
        }
        if (a.dlogits_in) {   // the caller's dL/dlogits instead of the loss gradient (rows / classes beyond the batch: 0)
            for (int e = tid; e < WIDE_TROWS * Cp; e += CHAIN_THREADS) {
                const int bl = e / Cp, c = e - bl * Cp;
                lg_l[bl * SC + c] = (row0 + bl < nvalid && c < C) ? a.dlogits_in[(int64_t)(row0 + bl) * C + c] : 0.f;
            }
        } else if (g.loss_mode == 1) wide_bce_rows(a, cs, lg_l, SC, red_l, row0, nvalid, tid, ord);
        else wide_softmax_rows(a, cs, lg_l, SC, red_l, row0, nvalid, nf, tid, ord);
        __syncthreads();
        for (int e = tid; e < WIDE_TROWS * Cp; e += CHAIN_THREADS) {      // dlogits -> global (dy operand of the HEAD segment)
            const int bl = e / Cp, c = e - bl * Cp;
            if (row0 + bl < Bp) sb[g.sb_dlog + (int64_t)(row0 + bl) * Cp + c] = lg_l[bl * SC + c];
        }
    }
    if (a.logits_out) return;
    __syncthreads();
    chain_step_stats(a, cs, red_l, Bp, tid, cgidx);
    if (tid < C)              // head-bias Adam over the dlogits of the whole batch
        head_bias_adam(W, Mv, Vv, cvec_off + g.vec_head + tid, vecW[g.vec_head + tid], vecM[g.vec_head + tid], vecV[g.vec_head + tid],
                       sb + g.sb_dlog + tid, Cp, Bp, ac);

    // ------------------------------------------------------------------ backward chain
    for (int i = L - 1; i >= 0; --i) {
        const int nl = cd.conf[i][2] & 3;
        const int64_t vb = cvec_off + (int64_t)i * g.vec_cell_stride;
        const int vbl = i * g.vec_cell_stride;
        const bool from_head = (i == L - 1);
        const float* src = from_head ? sb + g.sb_dlog : sb + g.sb_dy + (int64_t)(i + 1) * Bp * Rp;
        const int sstride = from_head ? Cp : Rp;
        const int nkk = from_head ? ncb : nrb;
        const int64_t Tidx = from_head ? cd.headT_off : cd.outT_off[i + 1];
        float* dy_g = sb + g.sb_dy + (int64_t)i * Bp * Rp;
        float sdz_[RBW] = {0.f, 0.f, 0.f, 0.f}, sdzx_[RBW] = {0.f, 0.f, 0.f, 0.f};
        // pass 1: d out_i = dy_{i+1} W_out / dlogits Wc through the transposed tiles, dropout mask, the BatchNorm column sums
        // (the masked gradient is parked in dy_i's own buffer: every element belongs to one lane)
        for (int p = 0; p < npair; ++p) {
            __syncthreads();
            stage_rows(src, sstride, sstride, p * WIDE_TROWS);
            __syncthreads();
#pragma unroll
            for (int rbi = 0; rbi < RBW; ++rbi) {
                const int rb = wave + rbi * CHAIN_NW;
                if (rb < nrb) {
                    const int r = rb * 16 + l15;
                    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
                    lds_x_times_tiles<2, false, 8>(acc, xt_l, SX, a.wt, Tidx + (int64_t)rb * nkk * 256, 256, nkk, lane);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int mb = 2 * p + t;
                        if (mb < MB) {
                            f32x4 xh4 = {0.f, 0.f, 0.f, 0.f};
                            if (g.bn) xh4 = *reinterpret_cast<const f32x4*>(sav + sav_plane + ((((int64_t)i * nrb + rb) * MB + mb) << 8) + lane * 4);
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int b = mb * 16 + 4 * lg + q;
                                float d = acc[t][q];
                                if (g.use_drop) d = drop_keep(h0, i, (uint32_t)(b * R + r), g.drop_thr) ? d * g.drop_scale : 0.0f;
                                if (!(b < nvalid)) d = 0.f;
                                sdz_[rbi] += d;
                                if (g.bn) sdzx_[rbi] += d * xh4[q];
                                dy_g[(int64_t)b * Rp + r] = d;
                            }
                        }
                    }
                }
            }
        }
        // pass 2: BatchNorm backward with the whole batch's sums, activation backward -> dy_i; Adam on the column's vector parameters
        float dalpha = 0.f;
#pragma unroll
        for (int rbi = 0; rbi < RBW; ++rbi) {
            const int rb = wave + rbi * CHAIN_NW;
            if (rb < nrb) {
                const int r = rb * 16 + l15;
                const bool colok = r < R;
                float gr = 0.f;
                if (g.bn) gr = vecW[vbl + VEC_G * Rp + r] * rstd_l[i * Rp + r];
                const int64_t ob = vb + VEC_B * Rp + r, og = vb + VEC_G * Rp + r, obe = vb + VEC_BE * Rp + r;
                float pw[3] = {0.f, 0.f, 0.f}, pm[3] = {0.f, 0.f, 0.f}, pv[3] = {0.f, 0.f, 0.f};
                if (lg == 0 && colok) {
                    const int lb = vbl + VEC_B * Rp + r, lgm = vbl + VEC_G * Rp + r, lbe = vbl + VEC_BE * Rp + r;
                    pw[0] = vecW[lb]; pm[0] = vecM[lb]; pv[0] = vecV[lb];
                    if (g.bn) {
                        pw[1] = vecW[lgm]; pm[1] = vecM[lgm]; pv[1] = vecV[lgm];
                        pw[2] = vecW[lbe]; pm[2] = vecM[lbe]; pv[2] = vecV[lbe];
                    }
                }
                float dgam = 0.f, dbet = 0.f, k1 = 0.f, k2 = 0.f;
                if (g.bn) {
                    dbet = colsum(sdz_[rbi]);
                    dgam = colsum(sdzx_[rbi]);
                    k1 = dbet / nf; k2 = dgam / nf;
                }
                float sdy = 0.f;
                for (int mb = 0; mb < MB; ++mb) {
                    const int64_t o = ((((int64_t)i * nrb + rb) * MB + mb) << 8) + lane * 4;
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(sav + o);
                    f32x4 xh4 = {0.f, 0.f, 0.f, 0.f}, df4 = {0.f, 0.f, 0.f, 0.f};
                    if (g.bn) xh4 = *reinterpret_cast<const f32x4*>(sav + sav_plane + o);
                    if (g.alphas) df4 = *reinterpret_cast<const f32x4*>(sav + 2 * sav_plane + o);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int b = mb * 16 + 4 * lg + q;
                        float d = dy_g[(int64_t)b * Rp + r];
                        if (g.bn) {
                            const float da = gr * (d - k1 - xh4[q] * k2);
                            d = b < nvalid ? da : 0.f;
                        }
                        float dy = act_bwd(a4[q], d, nl);
                        if (!colok) dy = 0.f;
                        sdy += dy;
                        dalpha += dy * df4[q];
                        dy_g[(int64_t)b * Rp + r] = dy;
                    }
                }
                const float db = colsum(sdy);
                if (lg == 0 && colok) column_vec_adam(W, Mv, Vv, ob, og, obe, pw, pm, pv, db, dgam, dbet, g.bn, ac);
            }
        }
        if (g.alphas) {   // d(alpha_i) = sigma'(alpha) * sum_{b,r} dy[b,r] * (yS_raw - yV_raw)[b,r], waves summed in order
            for (int o = 32; o > 0; o >>= 1) dalpha += __shfl_xor(dalpha, o);
            if (lane == 0) red_l[2 * Bp + wave] = dalpha;
            __syncthreads();
            if (tid == 0) {
                float tot = 0.f;
                for (int w = 0; w < CHAIN_NW; ++w) tot += red_l[2 * Bp + w];
                alpha_adam(W, Mv, Vv, vb + 5 * Rp, vecW[vbl + 5 * Rp], vecM[vbl + 5 * Rp], vecV[vbl + 5 * Rp], tot, ac);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_sweep_wide — dW + Adam + next-step forward of one unit: row blocks rb0 .. rb0 + rows_p / 16 (one per wave) x k-blocks
// sub_kb0 .. sub_kb0 + sub_nkb of the descriptor's layout chunk.  dW = x_t^T dy accumulates over the batch slices in registers
// (v_mfma_f32_16x16x4_f32, batch blocks in ascending order like DW_BATCH_LOOP); then Adam on the tiles, which stay in registers
// for the next step's forward partials, slice by slice.
// ------------------------------------------------------------------------------------------------
template <bool NT>
__global__ void __launch_bounds__(STEP_THREADS, 2) k_sweep_wide(const StepArgs sa_) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SweepArgs& a = sa_.sa;
    const SegDesc d = a.desc[blockIdx.x];
    const CandDev& cd = a.cands[d.cand];
    const Geo& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int MB = g.MB, Bp = g.Bp;
    const int nrbg = d.rows_p >> 4, nkbl = d.cc >> 4, kbu0 = d.sub_kb0, nkbu = d.sub_nkb, ccu = nkbu * 16, col0 = d.k0 + kbu0 * 16;
    const WideSweepLds<float*> m = wide_sweep_lds(lds, ccu, d.rows_p);    // (lds.hip.h)
    const int ST = m.ST, SN = m.SN, SD = m.SD;
    float* xt = m.xt.at;
    float* xn = m.xn.at;
    float* dyl = m.dy.at;
    const bool feat = d.kind <= KIND_V;
    const bool upd = a.do_update != 0;
    const bool fwd = (a.do_forward != 0) && feat;
    if (!upd && !fwd) return;
    const int64_t sbo = cd.step_off;
    const bool active = wave < nrbg;
    const int rb = wave;
    const int32_t* ordp = cand_order(a.order, g, cd.gidx);
    const void* tp = feat ? (d.kind == KIND_S ? a.tab.s[d.tap] : a.tab.v[d.tap]) : nullptr;

    f32x4 tw[WIDE_KB];      // dW^T tiles, then the updated weight tiles
#pragma unroll
    for (int kb = 0; kb < WIDE_KB; ++kb) tw[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float* Wp = a.plane + d.w_off;
    float* Mp = Wp + a.plane_stride;
    float* Vp = Mp + a.plane_stride;
    if (upd) {
        const int xcell = d.kind == KIND_OUT ? d.cell - 1 : cd.L - 1;
        const int64_t dsrc = d.kind == KIND_HEAD ? sbo + g.sb_dlog : sbo + g.sb_dy + (int64_t)d.cell * Bp * g.Rp;
        const int dld = d.seg_nrb * 16;
        for (int s0 = 0; s0 < Bp; s0 += WIDE_SLICE) {
            const int ns = min(WIDE_SLICE, Bp - s0);
            if (s0) __syncthreads();
            if (feat) stage_table(xt, ST, tp, a.tab.dtype, d.width, col0, ccu, ordp, a.pos_t + s0, a.base_t + s0, a.nvalid_t - s0, ns, tid, STEP_THREADS);
            else stage_f32<false>(xt, ST, a.stepbuf, sbo + g.sb_xo + ((int64_t)xcell * Bp + s0) * g.Rp + col0, g.Rp, ccu, ns, tid, STEP_THREADS);
            stage_f32<false>(dyl, SD, a.stepbuf, dsrc + (int64_t)s0 * dld + d.rb0 * 16, dld, d.rows_p, ns, tid, STEP_THREADS);
            __syncthreads();
            if (active)
                for (int j = 0; j < (ns >> 2); ++j) {
                    const float dyf = dyl[(4 * j + lg) * SD + rb * 16 + l15];
                    const float* xr = xt + (4 * j + lg) * ST + l15;
#pragma unroll
                    for (int kb = 0; kb < WIDE_KB; ++kb)
                        if (kb < nkbu) tw[kb] = MFMA16(xr[kb * 16], dyf, tw[kb]);
                }
        }
        if (active) {
            float gsc = 1.0f;
            if (g.alphas && feat) gsc = a.stepbuf[sbo + g.sb_gsc + d.cell * 2 + d.kind];
            const float a_ss = a.ac.ss, a_bc2s = a.ac.bc2s, a_w1 = a.ac.w1, a_b2 = a.ac.b2, a_w2 = a.ac.w2, a_eps = a.ac.eps, a_wd = a.ac.wd;
            float* T = d.wt_off >= 0 ? a.wt + d.wt_off : nullptr;
#pragma unroll
            for (int k0 = 0; k0 < WIDE_KB; k0 += 4) {
                f32x4 w4[4], m4[4], v4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k0 + u < nkbu) {
                        const int64_t off = ((int64_t)rb * nkbl + kbu0 + k0 + u) * 256 + lane * 4;
                        w4[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Wp + off)) : *reinterpret_cast<const f32x4*>(Wp + off);
                        m4[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Mp + off)) : *reinterpret_cast<const f32x4*>(Mp + off);
                        v4[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Vp + off)) : *reinterpret_cast<const f32x4*>(Vp + off);
                    }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k0 + u < nkbu) {
                        const int64_t off = ((int64_t)rb * nkbl + kbu0 + k0 + u) * 256 + lane * 4;
                        f32x4 w = w4[u], m = m4[u], v = v4[u];
                        adam4(w, m, v, tw[k0 + u] * gsc, a_ss, a_bc2s, a_w1, a_b2, a_w2, a_eps, a_wd);
                        tw[k0 + u] = w;
                        if (NT) {
                            __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(Wp + off));
                            __builtin_nontemporal_store(m, reinterpret_cast<f32x4*>(Mp + off));
                            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(Vp + off));
                        } else {
                            *reinterpret_cast<f32x4*>(Wp + off) = w;
                            *reinterpret_cast<f32x4*>(Mp + off) = m;
                            *reinterpret_cast<f32x4*>(Vp + off) = v;
                        }
                        if (T) {   // the transposed copy the backward chain reads (tile_run's image)
                            float* Tt = T + ((int64_t)((d.k0 >> 4) + kbu0 + k0 + u) * d.seg_nrb + d.rb0 + rb) * 256;
                            const int base = (((l15 >> 2) * 16 + 4 * lg) << 2) + (l15 & 3);
#pragma unroll
                            for (int q = 0; q < 4; ++q) Tt[base + 4 * q] = w[q];
                        }
                    }
            }
        }
    } else if (active) {
#pragma unroll
        for (int kb = 0; kb < WIDE_KB; ++kb)
            if (kb < nkbu) tw[kb] = *reinterpret_cast<const f32x4*>(Wp + ((int64_t)rb * nkbl + kbu0 + kb) * 256 + lane * 4);
    }
    if (!fwd) return;
    // next step's forward partials of this chunk, [seg_nrb][MB][256] in MFMA D layout: this unit owns row blocks rb0 ...
    const int64_t part = sbo + g.sb_part + (((int64_t)(cd.part_cell_off[d.cell] + d.part_idx) * d.seg_nrb * MB) << 8) + (((int64_t)d.rb0 * MB) << 8);
    for (int s0 = 0; s0 < Bp; s0 += WIDE_SLICE) {
        const int ns = min(WIDE_SLICE, Bp - s0);
        __syncthreads();
        stage_table(xn, SN, tp, a.tab.dtype, d.width, col0, ccu, ordp, a.pos_n + s0, a.base_n + s0, a.nvalid_n - s0, ns, tid, STEP_THREADS);
        __syncthreads();
        if (active)
            for (int mbl = 0; mbl < (ns >> 4); ++mbl) {
                f32x4 yacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < WIDE_KB; ++kb)
                    if (kb < nkbu) {
                        const f32x4 x4 = *reinterpret_cast<const f32x4*>(xn + (mbl * 16 + l15) * SN + kb * 16 + 4 * lg);
#pragma unroll
                        for (int q = 0; q < 4; ++q) yacc = MFMA16(x4[q], tw[kb][q], yacc);
                    }
                *reinterpret_cast<f32x4*>(a.stepbuf + part + ((rb * MB + (s0 >> 4) + mbl) << 8) + lane * 4) = yacc;
            }
    }
}
