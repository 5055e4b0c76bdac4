// records.hip.h — what the host and the kernels SHARE, stated once: the records the planner (plan.hip.h) fills and the kernels read
// (SegDesc, TapDesc, CandDev, DevStats, Geo), the sizes both sides must agree on, and the LDS formulas the planner budgets with where a
// kernel still walks its LDS itself (the layouts both sides read are lds.hip.h).  Plain C++17 (no HIP include, no device code): the
// device headers include it, and so do the pure host headers plan.hip.h and builds.hip.h, which g++ compiles alone
// (tests/plan_header.py, tests/builds_header.py).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/mfas_hip.h"      // (by its place in the tree: a program that holds a pure header needs no include path but csrc)

#ifdef __HIPCC__
#define MFAS_HD __host__ __device__
#else
#define MFAS_HD
#endif

#define KIND_S 0
#define KIND_V 1
#define KIND_OUT 2
#define KIND_HEAD 3

// ------------------------------------------------------------------------------------------------
// Device-side descriptors
// ------------------------------------------------------------------------------------------------
struct SegDesc {          // one workgroup of k_sweep / k_pack
    int32_t cand, kind, cell, tap;
    int32_t k0, cc;       // first column inside the segment, chunk columns (multiple of 16)
    int32_t rows_p, width;  // padded rows; FEAT: table row width (elements)
    int64_t w_off;        // float offset (within a plane) of this chunk: tiles [rb][kb][256]
    int64_t wt_off;       // OUT/HEAD: float offset in the transposed arena, else -1
    int32_t part_idx;     // FEAT: chunk index within the cell's partial list
    int32_t rows, cols;   // true rows (R or C) / true columns of the whole segment
    int64_t src_off;      // flat-parameter offset of the matrix this segment belongs to
    int32_t src_ld, src_col0;
    uint32_t init_seed;   // hash seed of that matrix (device init)
    float init_bound;
    int32_t rb0, seg_nrb; // row-split units: first row block of this unit inside the segment, row blocks of the whole segment
                          // (rows_p = rows of THIS unit; w_off already points at row block rb0 of the chunk)
    int32_t sub_kb0, sub_nkb; // wide units (wide.hip.h): first k-block of the unit inside this layout chunk, its k-blocks (<= 8); 0 elsewhere
                          // (the struct, and every kernel's descriptor indexing, stays at 104 bytes)
};
static_assert(sizeof(SegDesc) == 104, "SegDesc layout");

#define TAP_MAX_ITEMS 8
struct TapDesc {          // tap-major workgroup (R < 128): one feature chunk shared by up to 8 segments of that tap
    int32_t kind, tap, k0, cc;      // modality (KIND_S / KIND_V), tap index, first column, columns
    int32_t rows_p, width, nitems, _pad;
    int32_t cand[TAP_MAX_ITEMS], cell[TAP_MAX_ITEMS], part_idx[TAP_MAX_ITEMS];
    int64_t w_off[TAP_MAX_ITEMS];   // plane offset of each item's chunk: tiles [rb][kb][256]
};

struct CandDev {
    int32_t L;
    int32_t conf[MFAS_MAX_CELLS][3];
    int64_t seg_off[MFAS_MAX_CELLS][3];   // plane offset of S / V / OUT segment of cell i (-1: none)
    int32_t seg_cc[MFAS_MAX_CELLS][3];    // chunk columns of that segment
    int32_t seg_cols[MFAS_MAX_CELLS][3];  // padded columns
    int64_t head_off;
    int64_t outT_off[MFAS_MAX_CELLS];     // transposed arena offset of cell i's OUT segment
    int64_t headT_off;
    int64_t vec_off;                      // plane offset of the vector block
    int32_t nch_s[MFAS_MAX_CELLS], nch_v[MFAS_MAX_CELLS];
    int32_t part_cell_off[MFAS_MAX_CELLS];  // first partial-slot index of cell i
    int64_t step_off;                     // float offset of this candidate's step buffers
    uint32_t drop_seed;
    int32_t gidx;                         // index of this candidate in the population (stats / status slot)
    // flat (reference state_dict order) offsets of this candidate's parameters
    int64_t f_alpha, f_W[MFAS_MAX_CELLS], f_b[MFAS_MAX_CELLS], f_bn[MFAS_MAX_CELLS], f_Wc, f_bc;
    int32_t K_in[MFAS_MAX_CELLS];   // in_features of cell i
    int32_t _pad2[4];
};

struct DevStats {
    double train_loss, dev_loss;
    long long train_corr, dev_corr;
};

struct Geo {             // geometry shared by all candidates of a population
    int32_t R, C, Rp, Cp, nrb, ncb, B, Bp, MB;
    int32_t bn, alphas, multitask, use_drop;
    float drop_scale, bn_eps, bn_mom;
    uint32_t drop_thr;
    // per-candidate step-buffer sub-offsets (floats)
    int64_t sb_part, sb_dy, sb_xo, sb_dlog, sb_sav, sb_yf, sb_gsc, sb_size;
    int32_t vec_cell_stride;   // 5*Rp + 16
    int32_t vec_head;          // offset of head bias inside the vector block
    int32_t sw[MFAS_MAX_TAPS], vw[MFAS_MAX_TAPS];   // table row strides of the taps (width padded to 16)
    int32_t loss_mode;         // 0 softmax CE + accuracy, 1 weighted BCE + F1-samples
    float f1_th;
    int64_t order_stride;      // elements between two candidates' sample-order tables (0: one order shared by the population)
};

// vector block of a candidate (inside every plane): per cell [b | gamma | beta | rm | rv | alpha(16)], then bc[Cp]
#define VEC_B 0
#define VEC_G 1
#define VEC_BE 2
#define VEC_RM 3
#define VEC_RV 4

// ------------------------------------------------------------------------------------------------
// Sizes the planner's budgets and the kernels' buffers agree on (each kernel's header says what it does with its own)
// ------------------------------------------------------------------------------------------------
#define STEP_NW 8
#define STEP_THREADS (STEP_NW * 64)

// Per-(candidate, cell) "dy is out" flags of the same-group fused launch (k_step_same): [candidate][8] uint32, slot i < 4: dy_i of
// cell i (published after backward cell i, i.e. when the chain no longer reads W_out_{i+1}^T / Wc^T either); the value is the
// global step index + 1 (monotonic over a train() call)
#define CELLFLAG_STRIDE 8

#define PERSIST_LDS_WORDS 32            // LDS words the loop itself uses (behind the bodies' LDS)
#define PERSIST_NTR 4                   // resident units, f32 staging: tiles per wave (cc <= 512 columns)
#define PERSIST_NTR16 8                 // resident units, 16-bit staging: cc <= 1024 columns

#define LEAN_OWN_TILES 7   // slots 0..2: OUT_1..OUT_3, slots 3..6: head class blocks 0..3
#define LEAN_SCR 1024      // floats of chain_lean's cross-wave exchange scratch (its parts by name: lds.hip.h, LeanScr)
// chain_lean's own-tile area (LeanLds<MB>::own_floats / stage_floats): resident [W|M|V|T][7 tiles][256], otherwise [W|T] staged at entry
MFAS_HD constexpr int lean_own_floats() { return 4 * LEAN_OWN_TILES * 256; }
MFAS_HD constexpr int lean_stage_floats() { return 2 * LEAN_OWN_TILES * 256; }

#define WIDE_SLICE 64     // batch rows a sweep unit stages at a time
#define WIDE_KB 8         // k-blocks (of 16 columns) per sweep unit: the dW tiles one wave keeps in registers
#define WIDE_RBG STEP_NW  // row blocks per sweep unit: one per wave
#define WIDE_TROWS 32     // batch rows the chain stages at a time (two 16-row tiles)

// LDS floats of k_chain_wide (plan.hip.h budgets them; k_sweep_wide has its layout in lds.hip.h)
MFAS_HD constexpr size_t wide_chain_lds_floats(int Rp, int Cp, int Bp) {
    return (size_t)WIDE_TROWS * ((Rp > Cp ? Rp : Cp) + 4) + (size_t)WIDE_TROWS * (Cp + 4) + (size_t)MFAS_MAX_CELLS * Rp + 2 * (size_t)Bp + 16 + STEP_NW;
}

#define EVAL_CE 128   // staged feature columns per pass

#define XCH_SLOTS 7
#define XCH_CAND_FLOATS (2 * XCH_SLOTS * 8 * 256)

// LDS floats of chain_split<NS> (host: launch size)
template <int NS> MFAS_HD constexpr size_t chain_split_lds_floats(int Rp, int Cp) {
    return (size_t)2 * 16 * (Rp + 4) + (size_t)16 * (Cp + 4) + (size_t)MFAS_MAX_CELLS * (8 / NS) * 16 + 48 + 16 +
           (size_t)MFAS_MAX_CELLS * (8 / NS) * 256 + (size_t)(MFAS_MAX_CELLS * 5 * (8 / NS) * 16 + Cp) + (size_t)(8 / NS) * 8 * 256 +
           (size_t)2 * MFAS_MAX_CELLS * (8 / NS) * 256 + (size_t)(8 / NS) * 256;
}
