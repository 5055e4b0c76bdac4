// tapgrad.hip.h — the gradients of the feature taps from the train-mode backward (mfas_population_backward_taps): the work list, a pure
// host function over the plan's own descriptors, and k_tap_grad.  (part of the single translation unit mfas_hip.hip)
// The first half is plain C++17 like plan.hip.h / launches.hip.h — no HIP call, g++ compiles it alone (tests/tapgrad_header.py); the
// kernel and its launch follow under __HIPCC__.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "records.hip.h"
#include "hosterr.hip.h"
#include "plan.hip.h"

// ------------------------------------------------------------------------------------------------
// The work list.  After single_batch's backward chain dy_i of every cell lies in the candidate's step buffers, and what a tap's gradient
// needs of W is the tap's columns of every cell that selects it: d tap = sum_i scale_i * dy_i * W_i[:, tap columns].  One unit = one
// workgroup = up to TAPGRAD_KB consecutive 16-column blocks of ONE tap inside one layout chunk, with every cell of the candidate that
// selects the tap, cells ascending.  Where the tiles are comes from the descriptors single_batch hands to the sweep — pl.descs from
// desc_start[k], the group's units from wide_start[k] on a wide plan — never from a second statement of the plane layout: a unit that
// a plan cut into row-block pieces (rb0; sub_kb0 / sub_nkb) is joined in ascending rb0, and the join REFUSES pieces that do not
// continue each other (first row block, row blocks of the segment, one tile stride).
// ------------------------------------------------------------------------------------------------
#define TAPGRAD_KB 8          // 16-column blocks per unit: one per wave

struct TapGradDesc {          // one workgroup of k_tap_grad
    int32_t kind, tap;        // modality (KIND_S / KIND_V), tap slot
    int32_t kb0, nkb;         // first 16-column block of the unit inside the tap, its blocks (<= TAPGRAD_KB)
    int32_t width, nitems;    // true tap width = leading dimension of the output; cells that select the tap (0: the tap's gradient is zero)
    int32_t nrb, _pad;        // row blocks of a segment (Rp / 16)
    int32_t cell[MFAS_MAX_CELLS];
    int32_t rb_stride[MFAS_MAX_CELLS];   // floats from a tile to the tile of the next row block, same k-block
    int64_t w_off[MFAS_MAX_CELLS];       // plane offset of the tile (row block 0, k-block kb0) of each item
    float* out;               // DEVICE (nrows, width) float32 of this tap: filled in by the call, not by the work list
};

// the tile (row block 0, 16-column block kb of the tap) of cell `cell`, joined from the descriptors' pieces.  returns 0: the cell does
// not select the tap; 1: found; < 0: the pieces do not join (fail() has the text)
static int tap_tile_of(const SegDesc* descs, int n, int kind, int tap, int cell, int kb, int64_t* w_off, int32_t* rb_stride, int32_t* nrb) {
    std::vector<const SegDesc*> pieces;
    for (int j = 0; j < n; ++j) {
        const SegDesc& d = descs[j];
        if (d.kind != kind || d.tap != tap || d.cell != cell) continue;
        const int kbl = kb - d.k0 / 16;       // k-block inside the layout chunk
        if (kbl < 0 || kbl >= d.cc / 16) continue;
        if (d.sub_nkb > 0 && (kbl < d.sub_kb0 || kbl >= d.sub_kb0 + d.sub_nkb)) continue;
        pieces.push_back(&d);
    }
    if (pieces.empty()) return 0;
    std::stable_sort(pieces.begin(), pieces.end(), [](const SegDesc* x, const SegDesc* y) { return x->rb0 < y->rb0; });
    const SegDesc& p0 = *pieces[0];
    const int32_t stride = (p0.cc / 16) * 256;
    int next = 0;
    for (const SegDesc* p : pieces) {
        if (p->rb0 != next || p->cc != p0.cc || p->k0 != p0.k0 || p->seg_nrb != p0.seg_nrb || p->w_off != p0.w_off + (int64_t)p->rb0 * stride)
            return fail(MFAS_EINVAL, "internal: the row-block pieces of cell " + std::to_string(cell) + ", " + (kind == KIND_S ? "s" : "v") +
                                     std::to_string(tap) + " do not join (row block " + std::to_string(p->rb0) + ", expected " + std::to_string(next) + ")");
        next += p->rows_p / 16;
    }
    if (next != p0.seg_nrb) return fail(MFAS_EINVAL, "internal: the row-block pieces of cell " + std::to_string(cell) + " are incomplete");
    *w_off = p0.w_off + (int64_t)(kb - p0.k0 / 16) * 256; *rb_stride = stride; *nrb = p0.seg_nrb;
    return 1;
}

// The units of candidate k for the requested taps (want[kind][slot]), S slots first, slots and 16-column blocks ascending.  reads: the
// plan's descriptors, the declared tap widths.  A requested slot of width 0 is refused, naming the slot.
static int tap_grad_units(const LayoutPlan& pl, const mfas_hyper& hp, int k, const bool want[2][MFAS_MAX_TAPS], std::vector<TapGradDesc>& out) {
    out.clear();
    if (k < 0 || k + 1 >= (int)pl.desc_start.size()) return fail(MFAS_EINVAL, "bad argument");
    const SegDesc* descs = pl.wide ? pl.groups[0].descs.data() + pl.wide_start[k] : pl.descs.data() + pl.desc_start[k];
    const int n = pl.wide ? pl.wide_start[k + 1] - pl.wide_start[k] : pl.desc_start[k + 1] - pl.desc_start[k];
    for (int kind = KIND_S; kind <= KIND_V; ++kind)
        for (int tap = 0; tap < MFAS_MAX_TAPS; ++tap) {
            if (!want[kind][tap]) continue;
            const int width = kind == KIND_S ? hp.s_sizes[tap] : hp.v_sizes[tap];
            if (width < 1)
                return fail(MFAS_EINVAL, std::string("tap gradient requested for ") + (kind == KIND_S ? "s" : "v") + std::to_string(tap) + ", a slot of width 0");
            for (int kb = 0; kb < (width + 15) / 16; ++kb) {
                TapGradDesc b;
                memset(&b, 0, sizeof(b));
                b.kind = kind; b.tap = tap; b.kb0 = kb; b.nkb = 1; b.width = width; b.nrb = pl.g.nrb;
                for (int cell = 0; cell < MFAS_MAX_CELLS; ++cell) {
                    int32_t nrb = 0;
                    const int rc = tap_tile_of(descs, n, kind, tap, cell, kb, &b.w_off[b.nitems], &b.rb_stride[b.nitems], &nrb);
                    if (rc < 0) return MFAS_EINVAL;
                    if (rc == 0) continue;
                    if (nrb != pl.g.nrb) return fail(MFAS_EINVAL, "internal: a feature segment's row blocks differ from the geometry's");
                    b.cell[b.nitems++] = cell;
                }
                // the block continues the last unit when every item's tile is the next tile of the same layout chunk
                bool joins = !out.empty() && out.back().kind == kind && out.back().tap == tap && out.back().nkb < TAPGRAD_KB &&
                             out.back().kb0 + out.back().nkb == kb && out.back().nitems == b.nitems;
                for (int it = 0; joins && it < b.nitems; ++it) {
                    const TapGradDesc& u = out.back();
                    joins = u.cell[it] == b.cell[it] && u.rb_stride[it] == b.rb_stride[it] && u.w_off[it] + (int64_t)u.nkb * 256 == b.w_off[it];
                }
                if (joins) out.back().nkb++;
                else out.push_back(b);
            }
        }
    return MFAS_OK;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------------
// k_tap_grad — out[b][f] = sum over the unit's items (cells ascending) of scale_i * sum_r dy_i[b][r] * W_i[r][16 kb + f], for one unit:
// wave w owns 16-column block kb0 + w and keeps the accumulators of all Bp / 16 batch tiles (NT >= Bp / 16 is the build: <= 8 x 4 VGPRs).
// Per item and row block rb: the wave loads its 1 KiB tile (16 B per lane, coalesced; every W tile is read ONCE), the workgroup stages
// dy_i[:, 16 rb .. 16 rb + 16) — Bp x 16 floats, columns >= R as zeros — in LDS, and the tile goes through a per-wave padded LDS patch:
// a stored tile keeps W[16 rb + (l & 15)][16 kb + 4 (l >> 4) + q] in lane l, element q, but r is the contraction index, which
// v_mfma_f32_16x16x4_f32 wants in l >> 4.  MFMA step s contracts r = 16 rb + 4 (l >> 4) + s: the A operand of the four steps is ONE
// 16-byte LDS read of dy (row 16 mt + (l & 15), columns 4 (l >> 4) ..), the B operand is patch[4 (l >> 4) + s][l & 15]; both strides (20
// floats) make those reads conflict-free.  Staging areas and patches are double-buffered: one barrier per row block.
// Each cell's product is summed from zero, scaled by what the chain stored at sb_gsc + 2 i + kind (alphas; else 1) with an explicit
// multiply, and added to the running sum with an explicit add: the order is fixed and the bits do not depend on the run or on which
// other taps were requested.  Rows >= nrows and columns >= width are never written; a unit without items writes zeros.  No atomics,
// no workgroup reads what another writes.  Not in the kernel tables, not in the launch record (like k_vote and k_pool).
// ------------------------------------------------------------------------------------------------
#define TAPGRAD_SD 20         // LDS row stride of the staged dy block (floats)
#define TAPGRAD_SW 20         // LDS row stride of a wave's transposition patch

struct TapGradArgs {
    const float* plane;       // W plane
    const float* stepbuf;     // the candidate's step buffers (step_off applied)
    const TapGradDesc* desc;
    int64_t sb_dy, sb_gsc;
    int32_t Bp, Rp, R, nrows, alphas;
};

template <int NT>
__global__ void __launch_bounds__(STEP_THREADS) k_tap_grad(const TapGradArgs a) {
    __shared__ __attribute__((aligned(16))) float s_dy[2][NT * 16 * TAPGRAD_SD];
    __shared__ __attribute__((aligned(16))) float s_wt[2][STEP_NW][16 * TAPGRAD_SW];
    const TapGradDesc& d = a.desc[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int Bp = a.Bp, Rp = a.Rp, MB = Bp >> 4, nrb = d.nrb, nitems = d.nitems;
    const bool mine = wave < d.nkb;
    const int sb_b = tid >> 2, sb_c = (tid & 3) << 2;      // this thread's 16 bytes of a staged dy block: row, first column
    const bool stager = sb_b < Bp;
    f32x4 tot[NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) tot[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int par = 0;
    for (int it = 0; it < nitems; ++it) {
        const int cell = d.cell[it];
        const int64_t rbs = d.rb_stride[it];
        const float* wt = a.plane + d.w_off[it] + wave * 256 + lane * 4;
        const float* dyc = a.stepbuf + a.sb_dy + (int64_t)cell * Bp * Rp + (int64_t)sb_b * Rp + sb_c;
        f32x4 acc[NT];
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int rb = 0; rb < nrb; ++rb, par ^= 1) {
            f32x4 w = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
            if (mine) w = *reinterpret_cast<const f32x4*>(wt + rb * rbs);
            if (stager) dv = *reinterpret_cast<const f32x4*>(dyc + rb * 16);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (rb * 16 + sb_c + q >= a.R) dv[q] = 0.f;
            if (stager) *reinterpret_cast<f32x4*>(&s_dy[par][sb_b * TAPGRAD_SD + sb_c]) = dv;
            if (mine) *reinterpret_cast<f32x4*>(&s_wt[par][wave][l15 * TAPGRAD_SW + 4 * lg]) = w;
            __syncthreads();
            if (mine) {
                float bop[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) bop[s] = s_wt[par][wave][(4 * lg + s) * TAPGRAD_SW + l15];
#pragma unroll
                for (int mt = 0; mt < NT; ++mt)
                    if (mt < MB) {
                        const f32x4 av = *reinterpret_cast<const f32x4*>(&s_dy[par][(16 * mt + l15) * TAPGRAD_SD + 4 * lg]);
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc[mt] = MFMA16(av[s], bop[s], acc[mt]);
                    }
            }
        }
        const float sc = a.alphas ? a.stepbuf[a.sb_gsc + 2 * cell + d.kind] : 1.0f;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) tot[mt] = tot[mt] + sc * acc[mt];
    }
    if (!mine) return;
    // MFMA D layout: lane l, element q holds row 4 (l >> 4) + q, column l & 15
    const int f = 16 * (d.kb0 + wave) + l15;
    if (f >= d.width) return;
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int b = 16 * mt + 4 * lg + q;
            if (mt < MB && b < a.nrows) d.out[(int64_t)b * d.width + f] = tot[mt][q];
        }
}

// the launch of one call: the work list of candidate k for the non-NULL pointers, uploaded before anything of the call is launched
struct TapGradCall {
    std::vector<TapGradDesc> units;
    DevBuf<TapGradDesc> d_units;
};

// check + work list + upload; nothing is launched.  ds / dv: HOST [MFAS_MAX_TAPS] of DEVICE pointers or NULL (either array may be NULL)
static int tap_grad_prepare(const LayoutPlan& pl, const mfas_hyper& hp, int k, float* const* ds, float* const* dv, TapGradCall& c) {
    bool want[2][MFAS_MAX_TAPS];
    for (int j = 0; j < MFAS_MAX_TAPS; ++j) { want[KIND_S][j] = ds && ds[j]; want[KIND_V][j] = dv && dv[j]; }
    if (int rc = tap_grad_units(pl, hp, k, want, c.units)) return rc;
    for (TapGradDesc& u : c.units) u.out = u.kind == KIND_S ? ds[u.tap] : dv[u.tap];
    HIPCHK(c.d_units.upload(c.units));
    return MFAS_OK;
}

// one launch over the units, on `stream`, behind the chain that left dy and the scales (errors: hipGetLastError)
static void tap_grad_launch(const LayoutPlan& pl, const float* plane, const float* stepbuf, int k, int nrows, const TapGradCall& c, hipStream_t stream) {
    if (c.units.empty()) return;
    const Geo& g = pl.g;
    TapGradArgs a;
    a.plane = plane; a.stepbuf = stepbuf + pl.cands[k].step_off; a.desc = c.d_units.get();
    a.sb_dy = g.sb_dy; a.sb_gsc = g.sb_gsc; a.Bp = g.Bp; a.Rp = g.Rp; a.R = g.R; a.nrows = nrows; a.alphas = g.alphas;
    const unsigned grid = (unsigned)c.units.size();
    const int mb = g.Bp / 16;
    if (mb <= 1) hipLaunchKernelGGL(k_tap_grad<1>, dim3(grid), dim3(STEP_THREADS), 0, stream, a);
    else if (mb == 2) hipLaunchKernelGGL(k_tap_grad<2>, dim3(grid), dim3(STEP_THREADS), 0, stream, a);
    else if (mb <= 4) hipLaunchKernelGGL(k_tap_grad<4>, dim3(grid), dim3(STEP_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(k_tap_grad<8>, dim3(grid), dim3(STEP_THREADS), 0, stream, a);
}
#endif
