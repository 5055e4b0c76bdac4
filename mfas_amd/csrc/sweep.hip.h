// sweep.hip.h — the HBM-bound sweep: dW + Adam + next-step forward per weight tile (per-segment and tap-major decompositions)
// (part of the single translation unit mfas_hip.hip; see the header comment there and DESIGN.md)
#pragma once
#include "launches.hip.h"     // LAUNCH_PLAIN / _VIRTUAL / _DOUBLE
// ------------------------------------------------------------------------------------------------
// tile_run — the fused per-tile work shared by both sweep decompositions, for ONE row block `rb` over the k-blocks
// kb0, kb0+kbs, ... < nkb of a chunk: request SWEEP_U tiles of W/m/v, then per tile
//   dW^T = x_t^T dy (4*MB f32 MFMAs; D image == the tile image)  ->  Adam(+L2) on 4 elements/lane in registers  ->
//   store W, m, v (+ transposed copy T for OUT/HEAD)  ->  y_{t+1} += x_{t+1} W_new^T (4*MB f32 MFMAs) into yacc.
// Deferred stores (launches.hip.h): a virtual pass (`store` = false, wave-uniform) leaves the three stores out — the next sweep of the
// group loads the same tiles again.  That sweep is the double pass, DBL: before its own step it replays the step left out, dW from
// xp / dyp (the previous batch's rows in the ST layout, its dy in LDS, row stride SDp) -> Adam with that step's ss_p / bc2s_p — the same
// instructions on the same bits, so what it stores is what two plain sweeps store.  DBL is a template argument so that the plain walk
// keeps its registers: the caller branches once per row block, and the double walk takes both steps' dy from LDS per tile (dyc: this
// step's, laid out like dyp) and asks for half as many tiles at a time (the full count spills in every 128-register build).
// ------------------------------------------------------------------------------------------------
template <int MB, bool NT, int SWEEP_U, bool COH = false, bool DBL = false>
__device__ __forceinline__ void tile_run(float* Wp, float* Mp, float* Vp, const int rb, const int nkb, const int kb0,
                                         const int kbs, const float* xt, const int ST, const float* xn, const int SN,
                                         const float (&dyf)[MB * 4], const float gsc, const AdamC& ac, const bool upd,
                                         const bool fwd, f32x4 (&yacc)[MB], float* T, const int tstride_rb,
                                         const int lane, const int nj, const bool store = true, const float* xp = nullptr,
                                         const float* dyp = nullptr, const float* dyc = nullptr, const int SDp = 0,
                                         const float ss_p = 0.f, const float bc2s_p = 1.f) {
    static_assert(!(DBL && COH), "the same-group launch defers nothing");
    // nj = ceil(B / 4): batch blocks that hold data (DW_BATCH_LOOP, common.hip.h)
    const int l15 = lane & 15, lg = lane >> 4;
    const float a_ss = ac.ss, a_bc2s = ac.bc2s, a_w1 = ac.w1, a_b2 = ac.b2, a_w2 = ac.w2, a_eps = ac.eps, a_wd = ac.wd;
    for (int kbb = kb0; kbb < nkb; kbb += SWEEP_U * kbs) {
        f32x4 w4[SWEEP_U], m4[SWEEP_U], v4[SWEEP_U];
#pragma unroll
        for (int u = 0; u < SWEEP_U; ++u) {
            const int kb = kbb + u * kbs;
            if (kb < nkb) {
                const int64_t off = ((int64_t)rb * nkb + kb) * 256 + lane * 4;
                // state larger than the Infinity Cache is streamed once per step: nontemporal (+5 % HBM rate)
                w4[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Wp + off))
                           : *reinterpret_cast<const f32x4*>(Wp + off);
                if (upd) {
                    m4[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Mp + off))
                               : *reinterpret_cast<const f32x4*>(Mp + off);
                    v4[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Vp + off))
                               : *reinterpret_cast<const f32x4*>(Vp + off);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SWEEP_U; ++u) {
            const int kb = kbb + u * kbs;
            if (kb < nkb) {
                const int64_t off = ((int64_t)rb * nkb + kb) * 256 + lane * 4;
                if (upd) {
                    int dq = lg * SDp + rb * 16 + l15;      // (DBL) this lane's dy column of the row block, batch row lg
                    // (opaque per tile: as a loop invariant the 2 * MB * 4 dy values would be hoisted into registers for the whole walk)
                    if constexpr (DBL) asm volatile("" : "+v"(dq));
                    if constexpr (DBL) {      // the step the group's previous sweep left unstored, from the same version of the tile
                        f32x4 accp = {0.f, 0.f, 0.f, 0.f};
                        DW_BATCH_LOOP(MB, nj, accp = MFMA16(xp[(4 * j + lg) * ST + kb * 16 + l15], dyp[dq + 4 * j * SDp], accp))
                        f32x4 w = w4[u], m = m4[u], v = v4[u];
                        adam4(w, m, v, accp * gsc, ss_p, bc2s_p, a_w1, a_b2, a_w2, a_eps, a_wd);
                        w4[u] = w; m4[u] = m; v4[u] = v;
                        __builtin_amdgcn_sched_barrier(0);      // (this step's dW operands are not fetched under the replay: registers)
                    }
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    // (COH = the same-group fused launch: its 128-register budget has no room for two loop bodies, so it keeps the
                    // padded blocks — they add +0, which can only turn an accumulator of -0 into +0, and Adam's m, v and w come out
                    // the same for g = -0 and g = +0: tests/test_gpu_parity.py::test_same_group_launch_fuzz_bit_identical)
                    if constexpr (DBL) { DW_BATCH_LOOP(MB, nj, acc = MFMA16(xt[(4 * j + lg) * ST + kb * 16 + l15], dyc[dq + 4 * j * SDp], acc)) }
                    else { DW_BATCH_LOOP(MB, (COH ? MB * 4 : nj), acc = MFMA16(xt[(4 * j + lg) * ST + kb * 16 + l15], dyf[j], acc)) }
                    { f32x4 w = w4[u], m = m4[u], v = v4[u];
                      adam4(w, m, v, acc * gsc, a_ss, a_bc2s, a_w1, a_b2, a_w2, a_eps, a_wd);
                      w4[u] = w; m4[u] = m; v4[u] = v; }
                    if (!COH && !DBL && !store) {
                        // (the tile goes on to the forward product and is dropped: the group's next sweep replays this step)
                    } else if (NT) {
                        __builtin_nontemporal_store(w4[u], reinterpret_cast<f32x4*>(Wp + off));
                        __builtin_nontemporal_store(m4[u], reinterpret_cast<f32x4*>(Mp + off));
                        __builtin_nontemporal_store(v4[u], reinterpret_cast<f32x4*>(Vp + off));
                    } else {
                        // (COH = the same-group launch, one launch per step: the chain that reads OUT / HEAD runs in the NEXT launch, so plain
                        //  stores do — the write-through forms the removed multi-step persistent kernel needed here cost the OUT units
                        //  their L2 residency)
                        *reinterpret_cast<f32x4*>(Wp + off) = w4[u];
                        *reinterpret_cast<f32x4*>(Mp + off) = m4[u];
                        *reinterpret_cast<f32x4*>(Vp + off) = v4[u];
                    }
                    if (T) {   // keep the transposed copy used by the backward chain in step (OUT / HEAD only)
                        float* Tt = T + ((int64_t)kb * tstride_rb + rb) * 256;
                        const int base = (((l15 >> 2) * 16 + 4 * lg) << 2) + (l15 & 3);
#pragma unroll
                        for (int q = 0; q < 4; ++q) Tt[base + 4 * q] = w4[u][q];
                    }
                }
                if (fwd) {
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        const f32x4 x4 = *reinterpret_cast<const f32x4*>(xn + (mb * 16 + l15) * SN + kb * 16 + 4 * lg);
#pragma unroll
                        for (int q = 0; q < 4; ++q) yacc[mb] = MFMA16(x4[q], w4[u][q], yacc[mb]);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_sweep — fused dW + Adam + next-step forward.  One workgroup = ALL row blocks of one weight segment
// over a chunk of `cc` columns: x_t / x_{t+1} / dy are staged ONCE in LDS, then every wave streams whole
// row blocks (contiguous 1 KiB tiles), requesting the W/m/v tiles of 4 k-blocks before consuming them.
// (STEP_NW waves, STEP_THREADS: records.hip.h)
// ------------------------------------------------------------------------------------------------
struct SweepArgs {
    const SegDesc* desc;
    const TapDesc* tdesc;   // tap-major work list (may be empty)
    int32_t ntap, _padt;
    const CandDev* cands;
    float* plane;
    int64_t plane_stride;
    float* wt;
    float* stepbuf;
    mfas_table tab;
    const int32_t* order;
    int64_t pos_t, pos_n;
    int32_t base_t, base_n, nvalid_t, nvalid_n;
    int32_t do_update, do_forward;
    AdamC ac;
    Geo g;
    // reduce-in-sweep (small populations, general chain): per (candidate, cell) arrival counters; the LAST feature workgroup of a
    // cell to finish sums the cell's partial slabs (fixed order = the chain's phase 0) into the step buffer's yf area, so the
    // next launch's chain reads 1 (or 2, alphas) reduced slab per cell instead of pulling every partial through its one CU
    uint32_t* red_cnt;
    // same-group fused launch: this unit's dy is published by a chain workgroup of the SAME launch (cellflag != nullptr): wait
    // for cellflag[candidate][cell] >= flag_target before reading it; flag_status[] receives an abort mark on timeout
    const uint32_t* cellflag;
    uint32_t flag_target;
    int32_t* flag_status;
    // gathered rows (two-group streaming schedule with per-candidate sample orders, see gather_body): when set, a feature unit
    // stages x_t / x_{t+1} from its candidate's gathered copy [parity][tap][Bp][width] instead of from the table through the order
    const char* gather;
    int64_t g_cand_stride, g_par_stride;   // bytes between two candidates' buffers / between the two parities of one
    int32_t g_par_t, g_par_n;              // parity that holds the rows of batch t / of batch t + 1
    // deferred stores (launches.hip.h): what the feature units of this launch do with W / m / v, and for LAUNCH_DOUBLE the step they
    // replay first: rows of batch t - 1 (table position / gathered parity), its dy area inside a candidate's step buffers, its step scalars
    int32_t mode, g_par_p;
    int64_t pos_p, sb_dy_prev;
    int32_t base_p, nvalid_p;
    float ss_p, bc2s_p;
};

// byte offset of tap (kind, tap)'s [Bp][width] block inside one parity of a candidate's gathered rows (S taps first, then V)
__device__ __forceinline__ int64_t gather_tap_off(const Geo& g, const int kind, const int tap, const int eb) {
    int64_t o = 0;
#pragma unroll
    for (int u = 0; u < MFAS_MAX_TAPS; ++u) {
        if (kind == KIND_V || u < tap) o += g.sw[u];
        if (kind == KIND_V && u < tap) o += g.vw[u];
    }
    return o * g.Bp * eb;
}

// ------------------------------------------------------------------------------------------------
// gather_body — one workgroup per candidate of the group whose CHAIN runs in this launch: copies the candidate's OWN table rows of
// its next batch(es) (per-candidate sample order) into its gathered buffer, tap by tap for the taps its configuration uses — the
// table is read in whole-row pieces of 256 B .. 4 KB instead of the 128-byte pieces the feature units would fetch one by one
// (240 K random 128-byte reads per launch cost the HBM far more than their bytes), and every row is read from the table once
// instead of twice (as x_{t+1} of one step and x_t of the next).  The sweep of this group runs in the NEXT launch.
// ------------------------------------------------------------------------------------------------
struct GatherArgs {
    const CandDev* cands;                  // the group's candidates (one workgroup each)
    char* buf;
    int64_t cand_stride, par_stride;       // bytes
    int64_t pos[2];
    int32_t base[2], nvalid[2], par[2];
    int32_t nsets, nblocks;
};

__device__ __forceinline__ void gather_body(const GatherArgs& ga, const CandDev& cd, const Geo& g, const mfas_table& tab,
                                            const int32_t* order, const int tid) {
    const int eb = tab.dtype == MFAS_DT_F32 ? 4 : 2;
    const int32_t* ordp = cand_order(order, g, cd.gidx);
    uint32_t used = 0;            // bit kind * MFAS_MAX_TAPS + tap
    for (int i = 0; i < cd.L; ++i) used |= (1u << cd.conf[i][0]) | (1u << (MFAS_MAX_TAPS + cd.conf[i][1]));
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (s >= ga.nsets) break;
        char* dst0 = ga.buf + (int64_t)cd.gidx * ga.cand_stride + (int64_t)ga.par[s] * ga.par_stride;
        for (int kt = 0; kt < 2 * MFAS_MAX_TAPS; ++kt) {
            if (!((used >> kt) & 1u)) continue;
            const int kind = kt < MFAS_MAX_TAPS ? KIND_S : KIND_V, tap = kt & (MFAS_MAX_TAPS - 1);
            const int w = kind == KIND_S ? g.sw[tap] : g.vw[tap];
            const char* src0 = reinterpret_cast<const char*>(kind == KIND_S ? tab.s[tap] : tab.v[tap]);
            char* dst = dst0 + gather_tap_off(g, kind, tap, eb);
            const int vpr = (w * eb) >> 4, nvec = ga.nvalid[s] * vpr;      // 16-byte vectors per row (widths are multiples of 16 elements)
            for (int e0 = tid; e0 < nvec; e0 += 4 * STEP_THREADS) {
                u32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * STEP_THREADS;
                    if (e < nvec) {
                        const int b = e / vpr, c = e - b * vpr;
                        const int64_t row = ordp ? (int64_t)ordp[ga.pos[s] + b] : (int64_t)(ga.base[s] + b);
                        v[u] = *reinterpret_cast<const u32x4*>(src0 + (row * w) * eb + ((int64_t)c << 4));
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * STEP_THREADS;
                    if (e < nvec) {
                        const int b = e / vpr, c = e - b * vpr;
                        *reinterpret_cast<u32x4*>(dst + ((int64_t)b * w) * eb + ((int64_t)c << 4)) = v[u];
                    }
                }
            }
        }
    }
}

// what changes from one train step to the next (k_step takes it from the launch arguments, the persistent loop computes it)
struct SweepStep {
    int64_t pos_t, pos_n;
    int32_t base_t, base_n, nvalid_t, nvalid_n;
    int32_t upd, fwd;
    float ss, bc2s;
};
__device__ __forceinline__ SweepStep sweep_step_of(const SweepArgs& a) {
    SweepStep s;
    s.pos_t = a.pos_t; s.pos_n = a.pos_n; s.base_t = a.base_t; s.base_n = a.base_n;
    s.nvalid_t = a.nvalid_t; s.nvalid_n = a.nvalid_n; s.upd = a.do_update; s.fwd = a.do_forward;
    s.ss = a.ac.ss; s.bc2s = a.ac.bc2s;
    return s;
}


#ifdef MFAS_CHAIN_TIMING
// (timing build, same-group launch of step 3 with a 4-part chain: flag_target = 4 * 4) when the LAST sweep unit of the launch ended and when
// the FIRST unit of cell 0 saw its flag, 100 MHz ticks, next to the chain's absolute stamps (status slots 64 + 27 / 28)
#define SW_UNIT_STAMP(k) do { if (COH && a.cellflag && a.flag_target == 16u && threadIdx.x == 0 && d.cell == 0 && d.kind == KIND_S && d.k0 == 0 && d.cand == 0) a.flag_status[64 + 29 + (k)] = (int32_t)wall_clock64(); } while (0)
#define SW_END_STAMP() do { if (COH && a.cellflag && a.flag_target == 16u && threadIdx.x == 0) { atomicMax(reinterpret_cast<uint32_t*>(&a.flag_status[64 + 27]), (uint32_t)wall_clock64()); \
        atomicMax(reinterpret_cast<uint32_t*>(&a.flag_status[128 + d.cell * 4 + d.kind]), (uint32_t)wall_clock64()); } } while (0)
#else
#define SW_END_STAMP() do { } while (0)
#define SW_UNIT_STAMP(k) do { } while (0)
#endif
// (DEFER = false: a build whose plans never defer stores — the same-group launch, the lean chain's k_step — carries no double walk)
template <int MB, bool NT, int U, bool COH = false, bool DEFER = !COH>
__device__ __forceinline__ void sweep_body(const SweepArgs& a, const SweepStep& st, const int bid, float* lds) {
    const SegDesc d = a.desc[bid];
    const CandDev& cd = a.cands[d.cand];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    constexpr int Bp = MB * 16;
    const int cc = d.cc, rows_p = d.rows_p, nrb = rows_p >> 4, nkb = cc >> 4;
    const int ST = cc + 16;   // x_t stride: conflict-free ds_read_b32 column reads
    const int SN = cc + 4;    // x_{t+1} stride: 16 B aligned rows for ds_read_b128
    const int SD = rows_p + 16;
    float* xt = lds;
    float* xn = xt + Bp * ST;
    float* dyl = xn + Bp * SN;
    const bool feat = d.kind <= KIND_V;
    const bool upd = st.upd != 0;
    const bool fwd = (st.fwd != 0) && feat;
    if (!upd && !fwd) return;
    float* wred = dyl + Bp * SD;   // [nrb][8 waves][MB][256], only when the chunk is k-split over waves
    // Work split: with >= 8 row blocks every wave owns whole row blocks (streams contiguous tiles, no
    // reduction); with fewer (R < 128, or a row-split unit) the waves split the k blocks and reduce through LDS.
    const bool split_k = nrb < STEP_NW;
    // deferred stores: the mode of this launch's feature units (OUT / HEAD units store every step).  A double pass also stages the rows
    // and the dy of the step it replays (xp, dyp) behind the three tiles of a plain pass; in a k-split unit over the slabs of the LAST
    // row block, which the waves write only after a barrier behind the last tile (the host defers only where plan.hip.h's
    // sweep_unit_lds_double fits the plan's LDS)
    const int mode = (DEFER && feat && upd) ? a.mode : LAUNCH_PLAIN;
    const bool dbl = mode == LAUNCH_DOUBLE;
    float* xp = wred + (split_k ? (nrb - 1) * STEP_NW * MB * 256 : 0);
    float* dyp = xp + Bp * ST;
    const int64_t sbo = cd.step_off;   // this candidate's step buffers inside a.stepbuf
    const bool red = a.red_cnt != nullptr;

    // ---- the k_step builds: a unit's staged streams are requested TOGETHER (common.hip.h, staging in two halves: the first pass of every
    // stream, 512 threads x 16 bytes, which is the whole stream of an MB = 1 unit), then written to the LDS, then the streams' remainders go
    // through the loops.  The loops alone are a load -> wait -> LDS write chain per stream, one memory round trip after another: 3 for a plain
    // or virtual pass (x_t, x_{t+1}, dy), 5 for a double pass (x_{t-1}, dy_{t-1} as well), against 1 here.  Only the sample order's entries (a
    // unit that stages from the table through `ord`) are a round trip of their own in front of the row loads.  Every request is made by every
    // lane: one with nothing to fetch reads `idle`, 16 bytes of the unit's own descriptor, and holds zeros — the zero rows of b >= nvalid.
    // Not in this form: the same-group builds (they wait for their cell's flag between the rows and dy), and k_step<2, NT, 4, 0, 1>, whose
    // 128 registers the walk fills (the two-halves form costs it 7 spilled VGPRs); requesting the first W / m / v tiles here too spilled
    // in every build with a double walk (profiles/sweep_prologue_ab.log).
    constexpr bool BATCHED = !COH && !(MB == 2 && U == 1 && DEFER);
    if constexpr (BATCHED) {
        const int dt = a.tab.dtype;
        const bool gath = a.gather && feat;      // the candidate's rows were gathered a launch ago (gather_body): rows 0 .. B-1 of its own copy
        const char* tp = feat ? reinterpret_cast<const char*>(d.kind == KIND_S ? a.tab.s[d.tap] : a.tab.v[d.tap]) : nullptr;
        const char *sp = tp, *sc = tp, *sn = tp;     // where the rows of batch t - 1 / t / t + 1 are read from
        if (gath) {
            const char* gb = a.gather + (int64_t)cd.gidx * a.g_cand_stride + gather_tap_off(a.g, d.kind, d.tap, dt == MFAS_DT_F32 ? 4 : 2);
            sp = gb + (int64_t)a.g_par_p * a.g_par_stride; sc = gb + (int64_t)a.g_par_t * a.g_par_stride; sn = gb + (int64_t)a.g_par_n * a.g_par_stride;
        }
        const int32_t* ordp = gath ? nullptr : cand_order(a.order, a.g, cd.gidx);
        const bool on_p = dbl, on_t = upd && feat, on_n = fwd, on_o = upd && !feat;
        const int64_t row_p = stage_table_row(on_p, dt, cc, ordp, a.pos_p, gath ? 0 : a.base_p, a.nvalid_p, Bp, tid);
        const int64_t row_t = stage_table_row(on_t, dt, cc, ordp, st.pos_t, gath ? 0 : st.base_t, st.nvalid_t, Bp, tid);
        const int64_t row_n = stage_table_row(on_n, dt, cc, ordp, st.pos_n, gath ? 0 : st.base_n, st.nvalid_n, Bp, tid);
        // dy of this unit's rows: columns [16*rb0, 16*rb0 + rows_p) of the segment's dy (row stride = the segment's padded rows)
        const int64_t dsrc = (d.kind == KIND_HEAD ? sbo + a.g.sb_dlog : sbo + a.g.sb_dy + (int64_t)d.cell * Bp * a.g.Rp) + d.rb0 * 16;
        const int64_t dsrc_p = sbo + a.sb_dy_prev + (int64_t)d.cell * Bp * a.g.Rp + d.rb0 * 16;
        const int64_t osrc = sbo + a.g.sb_xo + (int64_t)(d.kind == KIND_OUT ? d.cell - 1 : cd.L - 1) * Bp * a.g.Rp + d.k0;      // OUT / HEAD: x_t = `out`
        const void* idle = a.desc + bid;
        const u32x4 q_dy = stage_issue(stage_f32_mine(upd, rows_p, Bp, tid), stage_f32_src(a.stepbuf, dsrc, d.seg_nrb * 16, rows_p, tid), idle);
        const u32x4 q_dyp = stage_issue(stage_f32_mine(dbl, rows_p, Bp, tid), stage_f32_src(a.stepbuf, dsrc_p, d.seg_nrb * 16, rows_p, tid), idle);
        const u32x4 q_p = stage_issue(row_p >= 0, stage_table_src(sp, dt, d.width, d.k0, cc, row_p, tid), idle);
        const u32x4 q_t = stage_issue(on_o ? stage_f32_mine(true, cc, Bp, tid) : row_t >= 0,
                                      on_o ? stage_f32_src(a.stepbuf, osrc, a.g.Rp, cc, tid) : stage_table_src(sc, dt, d.width, d.k0, cc, row_t, tid), idle);
        const u32x4 q_n = stage_issue(row_n >= 0, stage_table_src(sn, dt, d.width, d.k0, cc, row_n, tid), idle);
        stage_f32_commit(upd, dyl, SD, rows_p, Bp, tid, q_dy);
        stage_f32_commit(dbl, dyp, SD, rows_p, Bp, tid, q_dyp);
        stage_table_commit(on_p, xp, ST, dt, cc, Bp, tid, q_p);
        if (on_o) stage_f32_commit(true, xt, ST, cc, Bp, tid, q_t);
        else stage_table_commit(on_t, xt, ST, dt, cc, Bp, tid, q_t);
        stage_table_commit(on_n, xn, SN, dt, cc, Bp, tid, q_n);
        // what a stream has beyond one pass (MB = 2 / 4, a wide chunk)
        if (on_p) stage_table(xp, ST, sp, dt, d.width, d.k0, cc, ordp, a.pos_p, gath ? 0 : a.base_p, a.nvalid_p, Bp, tid, STEP_THREADS, STEP_THREADS);
        if (on_t) stage_table(xt, ST, sc, dt, d.width, d.k0, cc, ordp, st.pos_t, gath ? 0 : st.base_t, st.nvalid_t, Bp, tid, STEP_THREADS, STEP_THREADS);
        if (on_n) stage_table(xn, SN, sn, dt, d.width, d.k0, cc, ordp, st.pos_n, gath ? 0 : st.base_n, st.nvalid_n, Bp, tid, STEP_THREADS, STEP_THREADS);
        if (on_o) stage_f32<false>(xt, ST, a.stepbuf, osrc, a.g.Rp, cc, Bp, tid, STEP_THREADS, STEP_THREADS);
        if (upd) stage_f32<false>(dyl, SD, a.stepbuf, dsrc, d.seg_nrb * 16, rows_p, Bp, tid, STEP_THREADS, STEP_THREADS);
        if (dbl) stage_f32<false>(dyp, SD, a.stepbuf, dsrc_p, d.seg_nrb * 16, rows_p, Bp, tid, STEP_THREADS, STEP_THREADS);
    } else {
    if (!COH && a.gather && feat) {      // the candidate's rows were gathered a launch ago (gather_body): rows 0 .. B-1 of its own copy
        const char* gb = a.gather + (int64_t)cd.gidx * a.g_cand_stride + gather_tap_off(a.g, d.kind, d.tap, a.tab.dtype == MFAS_DT_F32 ? 4 : 2);
        if (dbl) stage_table(xp, ST, gb + (int64_t)a.g_par_p * a.g_par_stride, a.tab.dtype, d.width, d.k0, cc, nullptr, 0, 0, a.nvalid_p, Bp, tid, STEP_THREADS);
        if (upd) stage_table(xt, ST, gb + (int64_t)a.g_par_t * a.g_par_stride, a.tab.dtype, d.width, d.k0, cc, nullptr, 0, 0, st.nvalid_t, Bp, tid, STEP_THREADS);
        if (fwd) stage_table(xn, SN, gb + (int64_t)a.g_par_n * a.g_par_stride, a.tab.dtype, d.width, d.k0, cc, nullptr, 0, 0, st.nvalid_n, Bp, tid, STEP_THREADS);
    } else {
    if (upd && feat) {
        const void* tp = d.kind == KIND_S ? a.tab.s[d.tap] : a.tab.v[d.tap];
        if (dbl) stage_table(xp, ST, tp, a.tab.dtype, d.width, d.k0, cc, cand_order(a.order, a.g, cd.gidx), a.pos_p, a.base_p, a.nvalid_p, Bp, tid, STEP_THREADS);
        stage_table(xt, ST, tp, a.tab.dtype, d.width, d.k0, cc, cand_order(a.order, a.g, cd.gidx), st.pos_t, st.base_t, st.nvalid_t, Bp, tid, STEP_THREADS);
    }
    if (fwd) {
        const void* tp = d.kind == KIND_S ? a.tab.s[d.tap] : a.tab.v[d.tap];
        stage_table(xn, SN, tp, a.tab.dtype, d.width, d.k0, cc, cand_order(a.order, a.g, cd.gidx), st.pos_n, st.base_n, st.nvalid_n, Bp, tid, STEP_THREADS);
    }
    }
    if constexpr (COH) {
        if (upd && a.cellflag) {   // the table rows above are in flight while the chain of this launch gets to this cell's dy
            __shared__ int s_go;
            if (tid == 0) {
                // feature units of cell i need dy_i; OUT_i (the prev-out block of cell i) and HEAD also OVERWRITE weights the chain of
                // this launch still reads in its backward pass (W_out_i^T for d out_{i-1}, Wc^T for d out_{L-1}): they wait until
                // the chain is past that product, i.e. for dy_{i-1} / dy_{L-1}
                const int slot = d.kind == KIND_HEAD ? cd.L - 1 : (d.kind == KIND_OUT ? d.cell - 1 : d.cell);
                const uint32_t* f = a.cellflag + (size_t)cd.gidx * CELLFLAG_STRIDE + slot;
                uint32_t spins = 0;
                int go = 1;
                while (ld_u32_relaxed(f) < a.flag_target) {
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > CELLFLAG_SPIN_LIMIT) { go = 0; atomicMax(&a.flag_status[cd.gidx], 2); break; }
                }
                s_go = go;
#ifdef MFAS_CHAIN_TIMING
                if (a.flag_target == 16u && slot == 0 && d.kind <= KIND_V) atomicMin(reinterpret_cast<uint32_t*>(&a.flag_status[64 + 28]), (uint32_t)wall_clock64());
#endif
            }
            __syncthreads();
            if (!s_go) return;
            SW_UNIT_STAMP(0);
        }
    }
    if (upd) {
        if (!feat) {
            const int xcell = d.kind == KIND_OUT ? d.cell - 1 : cd.L - 1;
            stage_f32<COH>(xt, ST, a.stepbuf, sbo + a.g.sb_xo + (int64_t)xcell * Bp * a.g.Rp + d.k0, a.g.Rp, cc, Bp, tid, STEP_THREADS);
        }
        // dy of this unit's rows: columns [16*rb0, 16*rb0 + rows_p) of the segment's dy (row stride = the segment's padded rows)
        const int64_t dsrc = d.kind == KIND_HEAD ? sbo + a.g.sb_dlog : sbo + a.g.sb_dy + (int64_t)d.cell * Bp * a.g.Rp;
        stage_f32<COH>(dyl, SD, a.stepbuf, dsrc + d.rb0 * 16, d.seg_nrb * 16, rows_p, Bp, tid, STEP_THREADS);
        if (dbl) stage_f32<false>(dyp, SD, a.stepbuf, sbo + a.sb_dy_prev + (int64_t)d.cell * Bp * a.g.Rp + d.rb0 * 16, d.seg_nrb * 16, rows_p, Bp, tid, STEP_THREADS);
    }
    }
    __syncthreads();
    SW_UNIT_STAMP(1);

    float* Wp = a.plane + d.w_off;
    float* Mp = Wp + a.plane_stride;
    float* Vp = Mp + a.plane_stride;
    const AdamC ac = adam_consts(a.ac, upd ? st.ss : 0.f, upd ? st.bc2s : 1.f);
    // alpha scaling of the gradient of S / V columns (aux_models.py:103-111): sigma(alpha_t) as used by this
    // step's forward, published by k_chain (alpha itself has already been stepped); 1.0 when alphas are off
    float gsc = 1.0f;
    if (a.g.alphas && feat && upd) gsc = ldc1<COH>(a.stepbuf + sbo + a.g.sb_gsc + d.cell * 2 + d.kind);

    const int rb0 = split_k ? 0 : wave, rbs = split_k ? 1 : STEP_NW;
    const int kb0 = split_k ? wave : 0, kbs = split_k ? STEP_NW : 1;
    // partial slot of this chunk: [seg_nrb][MB][256] in MFMA D layout; this unit owns row blocks rb0 .. rb0 + nrb
    const int64_t part = sbo + a.g.sb_part + (((int64_t)(cd.part_cell_off[d.cell] + d.part_idx) * d.seg_nrb * MB) << 8) +
                         (((int64_t)d.rb0 * MB) << 8);

    for (int rb = rb0; rb < nrb; rb += rbs) {
        float dyf[MB * 4];      // (the double walk reads dy from LDS tile by tile and leaves this alone)
        f32x4 yacc[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) yacc[mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float* Tt = d.wt_off >= 0 ? a.wt + d.wt_off + ((int64_t)(d.k0 >> 4) * d.seg_nrb + d.rb0) * 256 : nullptr;
        bool plain_walk = true;
        if constexpr (DEFER) {
            if (dbl) {
                plain_walk = false;
                tile_run<MB, NT, (U > 1 ? U / 2 : 1), false, true>(Wp, Mp, Vp, rb, nkb, kb0, kbs, xt, ST, xn, SN, dyf, gsc, ac, upd, fwd, yacc, Tt, d.seg_nrb,
                                                                    lane, (a.g.B + 3) >> 2, true, xp, dyp, dyl, SD, a.ss_p, a.bc2s_p);
                if (split_k && fwd && rb == nrb - 1) __syncthreads();     // xp / dyp lie over the slabs this row block is about to write
            }
        }
        if (plain_walk) {
#pragma unroll
            for (int j = 0; j < MB * 4; ++j) dyf[j] = upd ? dyl[(4 * j + lg) * SD + rb * 16 + l15] : 0.f;
            tile_run<MB, NT, U, COH>(Wp, Mp, Vp, rb, nkb, kb0, kbs, xt, ST, xn, SN, dyf, gsc, ac, upd, fwd, yacc, Tt, d.seg_nrb, lane,
                                     (a.g.B + 3) >> 2, mode != LAUNCH_VIRTUAL);
        }
        if (fwd) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                if (split_k)
                    *reinterpret_cast<f32x4*>(wred + (((rb * STEP_NW + wave) * MB + mb) << 8) + lane * 4) = yacc[mb];
                else if (red) stc4<true>(a.stepbuf, part + ((rb * MB + mb) << 8) + lane * 4, yacc[mb]);
                else   // partial slot in MFMA D layout [chunk][rb][mb][lane][4]
                    stc4<COH>(a.stepbuf, part + ((rb * MB + mb) << 8) + lane * 4, yacc[mb]);
            }
        }
    }
    SW_UNIT_STAMP(2);
    if (!fwd) { SW_END_STAMP(); return; }
    if (split_k) {
        __syncthreads();
        // deterministic cross-wave reduction (fixed order 0..7)
        for (int e = tid; e < nrb * MB * 64; e += STEP_THREADS) {
            const int slot = e >> 6, ln = e & 63;
            const int srb = slot / MB, smb = slot - srb * MB;      // slot = rb * MB + mb of the unit's slab; wred is [rb][wave][mb]
            f32x4 s = *reinterpret_cast<const f32x4*>(wred + (((srb * STEP_NW) * MB + smb) << 8) + ln * 4);
#pragma unroll
            for (int w = 1; w < STEP_NW; ++w)
                s += *reinterpret_cast<const f32x4*>(wred + (((srb * STEP_NW + w) * MB + smb) << 8) + ln * 4);
            if (red) stc4<true>(a.stepbuf, part + (slot << 8) + ln * 4, s);
            else stc4<COH>(a.stepbuf, part + (slot << 8) + ln * 4, s);
        }
    }
    if (!red) { SW_END_STAMP(); return; }
    // ---- reduce-in-sweep: arrive on the cell's counter; the last arriver sums the cell's slabs (write-through stores + every
    // wave's drain + barrier + relaxed agent-scope counter on the producer side, sc1 loads on the reader's: G16 R1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    SW_UNIT_STAMP(3);
    int* flagw = reinterpret_cast<int*>(lds);      // (the staging tiles are dead by now)
    const int ns_c = cd.nch_s[d.cell], nch_c = ns_c + cd.nch_v[d.cell];
    if (tid == 0) {
        uint32_t* cnt = a.red_cnt + d.cand * MFAS_MAX_CELLS + d.cell;
        const uint32_t old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == (uint32_t)(nch_c - 1);
        if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        flagw[0] = last;
    }
    __syncthreads();
    SW_UNIT_STAMP(4);
    if (!flagw[0]) { SW_END_STAMP(); return; }
    {
        const int snrb = d.seg_nrb;
        const int per_cell = snrb * MB * 64;            // float4 items of the cell's [nrb][MB][256] slab
        const int64_t part0 = sbo + a.g.sb_part + (((int64_t)cd.part_cell_off[d.cell] * snrb * MB) << 8);
        const int64_t yf0 = sbo + a.g.sb_yf + (int64_t)d.cell * per_cell * 4;
        const int64_t vplane = (int64_t)MFAS_MAX_CELLS * snrb * MB * 256;
        for (int it = tid; it < per_cell; it += STEP_THREADS) {
            f32x4 accS = {0.f, 0.f, 0.f, 0.f}, accV = {0.f, 0.f, 0.f, 0.f};
            constexpr int PB = 8;
            for (int ch0 = 0; ch0 < nch_c; ch0 += PB) {
                f32x4 p8[PB];
#pragma unroll
                for (int u = 0; u < PB; ++u)
                    if (ch0 + u < nch_c) p8[u] = ldc4<true>(a.stepbuf, part0 + (((int64_t)(ch0 + u) * snrb * MB) << 8) + it * 4);
#pragma unroll
                for (int u = 0; u < PB; ++u)
                    if (ch0 + u < nch_c) {
                        if (ch0 + u < ns_c) accS += p8[u]; else accV += p8[u];
                    }
            }
            if (a.g.alphas) {
                *reinterpret_cast<f32x4*>(a.stepbuf + yf0 + it * 4) = accS;
                *reinterpret_cast<f32x4*>(a.stepbuf + yf0 + vplane + it * 4) = accV;
            } else {
                *reinterpret_cast<f32x4*>(a.stepbuf + yf0 + it * 4) = accS + accV;
            }
        }
    }
    SW_END_STAMP();
}

// ------------------------------------------------------------------------------------------------
// sweep_tap_body — the same fused dW + Adam + next-step forward for SMALL R (1, 2 or 4 row blocks): a column chunk of
// ONE feature tap is staged once and shared by up to 8/nrb segments (candidates x cells) that read this tap; every wave
// owns one (segment, row block), streams its contiguous tiles and writes its forward partial directly — no cross-wave
// reduction, and the feature staging (1/3 of the traffic at R=16) is amortised over the segments.
// ------------------------------------------------------------------------------------------------
template <int MB, bool NT, int U>
__device__ __forceinline__ void sweep_tap_body(const SweepArgs& a, const int bid, float* lds) {
    const TapDesc& d = a.tdesc[bid];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    constexpr int Bp = MB * 16;
    const int cc = d.cc, rows_p = d.rows_p, nrb = rows_p >> 4, nkb = cc >> 4;
    const int ST = cc + 16, SN = cc + 4;
    float* xt = lds;
    float* xn = xt + Bp * ST;
    const bool upd = a.do_update != 0;
    const bool fwd = a.do_forward != 0;
    if (!upd && !fwd) return;
    const void* tp = d.kind == KIND_S ? a.tab.s[d.tap] : a.tab.v[d.tap];
    if (upd) stage_table(xt, ST, tp, a.tab.dtype, d.width, d.k0, cc, a.order, a.pos_t, a.base_t, a.nvalid_t, Bp, tid, STEP_THREADS);
    if (fwd) stage_table(xn, SN, tp, a.tab.dtype, d.width, d.k0, cc, a.order, a.pos_n, a.base_n, a.nvalid_n, Bp, tid, STEP_THREADS);
    __syncthreads();
    const int item = wave / nrb, rb = wave - item * nrb;
    if (item >= d.nitems) return;
    const CandDev& cd = a.cands[d.cand[item]];
    float* sb = a.stepbuf + cd.step_off;
    const int cell = d.cell[item];
    float dyf[MB * 4];
#pragma unroll
    for (int j = 0; j < MB * 4; ++j) dyf[j] = 0.f;
    if (upd) {
        const float* dsrc = sb + a.g.sb_dy + (int64_t)cell * Bp * a.g.Rp;
#pragma unroll
        for (int j = 0; j < MB * 4; ++j) dyf[j] = dsrc[(4 * j + lg) * rows_p + rb * 16 + l15];
    }
    float gsc = 1.0f;
    if (a.g.alphas && upd) gsc = sb[a.g.sb_gsc + cell * 2 + d.kind];
    float* Wp = a.plane + d.w_off[item];
    float* Mp = Wp + a.plane_stride;
    float* Vp = Mp + a.plane_stride;
    const AdamC ac = adam_consts(a.ac, a.ac.ss, a.ac.bc2s);
    f32x4 yacc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) yacc[mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    tile_run<MB, NT, U>(Wp, Mp, Vp, rb, nkb, 0, 1, xt, ST, xn, SN, dyf, gsc, ac, upd, fwd, yacc, nullptr, nrb, lane, (a.g.B + 3) >> 2);
    if (fwd) {
        float* part = sb + a.g.sb_part + (((int64_t)(cd.part_cell_off[cell] + d.part_idx[item]) * nrb * MB) << 8);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
            *reinterpret_cast<f32x4*>(part + ((rb * MB + mb) << 8) + lane * 4) = yacc[mb];
    }
}
