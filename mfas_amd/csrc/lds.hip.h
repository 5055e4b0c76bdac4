// lds.hip.h — the LDS layout of a kernel that takes its LDS as one `extern __shared__` block, stated ONCE: a function per kernel body
// that walks the body's areas in order from `base` and returns them (where each begins, its floats) with their `total`.  A kernel calls
// it with base = its LDS pointer and takes its pointers and row strides from the struct (`m.xt.at`, `m.ST`); the planner calls it with
// base = 0, which makes every `at` a float offset, and asks for `total * 4` bytes — there is no second statement of the layout
// (surrogate.hip.h's surr_lds is the same idea, for the surrogate kernels).  An area a kernel lays over another one is declared here as
// that area, never derived in the kernel.
// Here: k_sweep_wide, and the names of chain_lean's scratch parts and of k_president's loop words.  The other bodies
// still walk their LDS themselves against a formula in plan.hip.h / records.hip.h: the same treatment moved their register allocation
// (DESIGN.md §8).  (MFAS_LAYOUT, not MFAS_HD: on the device the functions are inlined by force, as every device function here is.)
// Plain C++17 like records.hip.h (no HIP call): tests/test_lds_cpu.py prints every area through a g++ program and checks order,
// disjointness, aliases, 16-byte alignment and the totals against the plan dump.
#pragma once
#include "records.hip.h"

#ifdef __HIPCC__
#define MFAS_LAYOUT __host__ __device__ __forceinline__
#else
#define MFAS_LAYOUT inline
#endif

template <class P> struct LdsArea {                       // P: float* (a kernel) or int32_t (float offsets)
    P at;
    int32_t len;                                          // floats
    MFAS_LAYOUT P end() const { return at + len; }
};
template <class P> struct LdsWalk {                       // areas in the order they are taken
    P base, at;
    MFAS_LAYOUT explicit LdsWalk(P b) : base(b), at(b) {}
    MFAS_LAYOUT LdsArea<P> take(int32_t len) { const LdsArea<P> a{at, len}; at = at + len; return a; }
    MFAS_LAYOUT int32_t total() const { return (int32_t)(at - base); }
};

// ------------------------------------------------------------------------------------------------
// k_sweep_wide: a WIDE_SLICE batch slice of a unit's columns and rows
// ------------------------------------------------------------------------------------------------
template <class P> struct WideSweepLds {
    int32_t ST;          // cols + 16, x_t's row stride: conflict-free ds_read_b32 column reads
    int32_t SN;          // cols + 4, x_{t+1}'s: 16-byte aligned rows for ds_read_b128
    int32_t SD;          // rows + 16, dy's
    LdsArea<P> xt, xn, dy;      // [WIDE_SLICE][ST], [WIDE_SLICE][SN], [WIDE_SLICE][SD]
    int32_t total;
};
template <class P> MFAS_LAYOUT WideSweepLds<P> wide_sweep_lds(P base, int cols, int rows) {
    WideSweepLds<P> m;
    LdsWalk<P> w(base);
    m.ST = cols + 16; m.SN = cols + 4; m.SD = rows + 16;
    m.xt = w.take(WIDE_SLICE * m.ST);
    m.xn = w.take(WIDE_SLICE * m.SN);
    m.dy = w.take(WIDE_SLICE * m.SD);
    m.total = w.total();
    return m;
}

// ------------------------------------------------------------------------------------------------
// chain_lean's cross-wave exchange scratch (LeanLds<MB>::scr, LEAN_SCR floats), its parts by name: float offsets into it
// ------------------------------------------------------------------------------------------------
struct LeanScr {
    static constexpr int bn_fwd = 0;    // [parity][sum | squares][tile][16] forward BatchNorm exchange (256)
    static constexpr int gv2 = 256;     // [cell][dgamma | dbeta][16] (128)
    static constexpr int bnf = 384;     // [forward sum | forward squares | backward][parity][tile wave] pair-exchange sequence numbers (uint32; 16 zeroed)
    static constexpr int bnv = 400;     // [cell][16] the cells' batch variance for the running statistics (chain_lean_tail) (64)
    static constexpr int bn_bwd = 512;  // [parity][..] backward BatchNorm exchange: not the forward's region, no barrier separates them (256)
    static constexpr int bst = 768;     // [tile wave][cell][mean | rstd][16] (256)
};
static_assert(LeanScr::bn_fwd + 256 <= LeanScr::gv2 && LeanScr::gv2 + 128 <= LeanScr::bnf && LeanScr::bnf + 16 <= LeanScr::bnv &&
              LeanScr::bnv + 64 <= LeanScr::bn_bwd && LeanScr::bn_bwd + 256 <= LeanScr::bst && LeanScr::bst + 256 <= LEAN_SCR, "chain_lean's scratch");

// ------------------------------------------------------------------------------------------------
// k_president's own words: PERSIST_LDS_WORDS behind the bodies' LDS (the kernel's lds_word argument), by name
// ------------------------------------------------------------------------------------------------
struct PresWords {
    static constexpr int wait = 0;    // a chain workgroup: wg_wait_ge's verdict
    static constexpr int pick = 0;    // a unit workgroup: the unit it serves next
    static constexpr int roll = 1;    // persist_roll_call's verdict
    static constexpr int arrive = 4;  // MB > 1: arrival counter of a unit's waves
    static constexpr int next = 8;    // [NU] next step of the workgroup's u-th unit
    static constexpr int stats = 16;  // LeanRes: the epoch's running statistics of a chain workgroup (6 words, 8-byte aligned)
};
static_assert(PresWords::stats + 6 <= PERSIST_LDS_WORDS, "the loop's words");
