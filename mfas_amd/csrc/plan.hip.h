// plan.hip.h — host side only: the environment switches (Tuning), the input checks and the LAYOUT PLAN — everything that is decided
// about a population before anything is allocated.  plan_layout() is a pure function: no HIP call, no allocation on the device, the
// CU count is an argument.  mfas_population_create lays the population out from its result, mfas_population_plan answers from it,
// persist_fallback asks it again without the resident schedule.
// plan_layout_as is a sequence of stages, each a function that says what it reads and writes: choose_chunk (plan_chunk; wide; the
// resident plan that does not stand) -> layout_candidates (layout_candidate, make_seg: records, descriptors, plane / arena offsets) ->
// lds_budgets -> dev_pass_and_streaming -> choose_schedule (enum Sched: the ONE statement of which of wide / resident / same-group / one
// group / two groups runs) + schedule_flags -> balanced_split -> group_work_list (tap_major_units, wide_units, same_group_units,
// row_block_unit) -> unit_dependent_flags (red_in_sweep, defer) -> resident_units_and_roles -> layout_step_buffers (once, after defer).
// Plain C++17, the fourth host header of this kind after devmem.hip.h, builds.hip.h and launches.hip.h: it includes what it uses and
// g++ compiles it alone.  What it shares with the kernels — the records it fills (SegDesc, TapDesc, CandDev, Geo), the sizes and the
// LDS formulas its budgets name — is records.hip.h; fail() is hosterr.hip.h's.  tests/test_plan_cpu.py pins the complete result for
// some 700 inputs through a g++ program (tests/plan_header.py, tests/plan_dump.h), also under the address and undefined sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>
#include "records.hip.h"
#include "lds.hip.h"
#include "hosterr.hip.h"
#include "builds.hip.h"      // PlanFacts
// ================================================================================================
// Tuning — EVERY environment switch of the library, parsed in ONE place (tuning_from_env) when a population is created or planned
// and kept in the population: nothing else in this translation unit calls getenv, so a variable that changes after create() cannot
// change the schedule of a population that was laid out (and parity-tested) without it.  An empty environment gives the defaults
// below = the configuration the test suites run; INTEGRATION.md lists the switches, mfas_tuning_describe() prints the parsed set
// (tests/test_host_cpu.py::test_switches_default_when_unset_and_retired_ones_are_ignored).  They are A/B and debugging aids, not API.
// ================================================================================================
struct Tuning {
    int persist = -1;               // MFAS_PERSIST            0: never take the resident schedule (k_president); unset / 1: where it fits
    int no_lean_chain = 0;          // MFAS_NO_LEAN_CHAIN      general chain_body also at R <= 16
    int groups = 0;                 // MFAS_GROUPS=1|2         force one / two candidate groups (0: by population size)
    int same_group = -1;            // MFAS_SAME_GROUP         0: never k_step_same, 2: whatever the size (-1: by state bytes)
    int no_tap_major = 0;           // MFAS_NO_TAP_MAJOR       per-segment sweep units also at R < 128
    int force_tap_major = 0;        // MFAS_FORCE_TAP_MAJOR    tap-major units even with < 192 workgroups
    int no_red_in_sweep = 0;        // MFAS_NO_RED_IN_SWEEP    the chain reduces the partial slabs itself
    double occ_bytes = -1.0;        // MFAS_OCC_BYTES          MB == 2: crossover between the 2- and 4-waves-per-SIMD sweep builds
    int no_xcd_placement = 0;       // MFAS_NO_XCD_PLACEMENT   resident launch: block b runs role b
    int n_xcd = 0;                  // MFAS_XCDS=n             XCDs the placement assumes (0: 8 — MI355X in SPX mode)
    int persist_trace = 0;          // MFAS_PERSIST_TRACE      allocate the step-phase timestamp buffer
    int nt = -1;                    // MFAS_NT=0|1             force cached / nontemporal W/m/v streaming (-1: by plane size)
    int eval_no_x16 = 0;            // MFAS_EVAL_NO_X16        dev pass: f32 row tiles also over bf16 tables
    int eval_no_msplit = 0;         // MFAS_EVAL_NO_MSPLIT     dev pass at R <= 32: one wave per row block
    int eval_no_b3 = 0;             // MFAS_EVAL_NO_B3         dev pass at R = 72..128: f32 feature products
    int eval_no_wl = 0;             // MFAS_EVAL_NO_WL         dev pass at R <= 16: every wait for the LDS weight tiles is vmcnt(0) (rows one chunk deep)
    int no_gather = 0;              // MFAS_NO_GATHER          feature units stage rows through the order table
    int gather_verbose = 0;         // MFAS_GATHER_VERBOSE
    int no_plain_chain = 0;         // MFAS_NO_PLAIN_CHAIN     resident chain: the general (BN / alphas / multitask capable) instantiation
    int persist_verbose = 0;        // MFAS_PERSIST_VERBOSE=1|2
    int prof_every = 16;            // MFAS_PROF_EVERY=n       HIP events around every n-th sweep launch when profiling is on
    int chain_split = -1;           // MFAS_CHAIN_SPLIT        0 or 1: the one-CU chain_body; unset / other values: the planner decides (4 CUs or 1)
    // test hooks: parsed only by the -DMFAS_TEST_HOOKS build variant (__graft_entry__.build_variant("hooks", ...)); the product library
    // never reads these variables
    int test_not_resident = -1;     // MFAS_PERSIST_TEST_NOT_RESIDENT=e   every roll call from epoch e on "fails"
    int test_lose_step = -1;        // MFAS_PERSIST_TEST_LOSE_STEP=t      candidate 0's chain never publishes step t
};

static Tuning tuning_from_env() {
    Tuning t;
    auto flag = [](const char* n) { return getenv(n) ? 1 : 0; };
    auto num = [](const char* n, int dflt) { const char* e = getenv(n); return e ? atoi(e) : dflt; };
    t.persist = getenv("MFAS_PERSIST") ? (atoi(getenv("MFAS_PERSIST")) != 0 ? 1 : 0) : -1;
    t.no_lean_chain = flag("MFAS_NO_LEAN_CHAIN");
    t.groups = num("MFAS_GROUPS", 0);
    t.same_group = num("MFAS_SAME_GROUP", -1);
    t.no_tap_major = flag("MFAS_NO_TAP_MAJOR");
    t.force_tap_major = flag("MFAS_FORCE_TAP_MAJOR");
    t.no_red_in_sweep = flag("MFAS_NO_RED_IN_SWEEP");
    if (const char* e = getenv("MFAS_OCC_BYTES")) t.occ_bytes = atof(e);
    t.no_xcd_placement = flag("MFAS_NO_XCD_PLACEMENT");
    t.n_xcd = num("MFAS_XCDS", 0);
    t.persist_trace = flag("MFAS_PERSIST_TRACE");
    t.nt = getenv("MFAS_NT") ? (atoi(getenv("MFAS_NT")) != 0 ? 1 : 0) : -1;
    t.eval_no_x16 = flag("MFAS_EVAL_NO_X16");
    t.eval_no_msplit = flag("MFAS_EVAL_NO_MSPLIT");
    t.eval_no_b3 = flag("MFAS_EVAL_NO_B3");
    t.eval_no_wl = flag("MFAS_EVAL_NO_WL");
    t.no_gather = flag("MFAS_NO_GATHER");
    t.gather_verbose = flag("MFAS_GATHER_VERBOSE");
    t.no_plain_chain = flag("MFAS_NO_PLAIN_CHAIN");
    t.persist_verbose = num("MFAS_PERSIST_VERBOSE", 0);
    t.prof_every = std::max(1, num("MFAS_PROF_EVERY", 16));
    t.chain_split = num("MFAS_CHAIN_SPLIT", -1);
#ifdef MFAS_TEST_HOOKS
    t.test_not_resident = num("MFAS_PERSIST_TEST_NOT_RESIDENT", -1);
    t.test_lose_step = num("MFAS_PERSIST_TEST_LOSE_STEP", -1);
#endif
    return t;
}

// "name=value ..." of the switches as parsed from the CURRENT environment, in declaration order (hooks=1 marks the test-hook variant)
extern "C" int mfas_tuning_describe(char* buf, int32_t cap) {
    if (!buf || cap <= 0) return MFAS_EINVAL;
    const Tuning t = tuning_from_env();
    char tmp[1024];
    snprintf(tmp, sizeof(tmp),
             "persist=%d no_lean_chain=%d groups=%d same_group=%d "
             "no_tap_major=%d force_tap_major=%d no_red_in_sweep=%d occ_bytes=%g no_xcd_placement=%d n_xcd=%d persist_trace=%d nt=%d eval_no_x16=%d "
             "eval_no_msplit=%d eval_no_b3=%d eval_no_wl=%d no_gather=%d gather_verbose=%d no_plain_chain=%d persist_verbose=%d prof_every=%d "
             "chain_split=%d test_not_resident=%d test_lose_step=%d hooks=%d",
             t.persist, t.no_lean_chain, t.groups, t.same_group,
             t.no_tap_major, t.force_tap_major, t.no_red_in_sweep, t.occ_bytes, t.no_xcd_placement, t.n_xcd, t.persist_trace, t.nt, t.eval_no_x16,
             t.eval_no_msplit, t.eval_no_b3, t.eval_no_wl, t.no_gather, t.gather_verbose, t.no_plain_chain, t.persist_verbose, t.prof_every,
             t.chain_split, t.test_not_resident, t.test_lose_step,
#ifdef MFAS_TEST_HOOKS
             1
#else
             0
#endif
    );
    snprintf(buf, (size_t)cap, "%s", tmp);
    return MFAS_OK;
}

static inline int ceil16(int x) { return (x + 15) & ~15; }

static int pick_chunk(int cols_p, int target) {
    int best = 16;
    for (int c = 16; c <= cols_p && c <= target; c += 16)
        if (cols_p % c == 0) best = c;
    return best;
}

// Everything mfas_population_create refuses about (hp, confs, n_cells, K): shared with mfas_population_plan, so that the query never
// reports a layout for inputs create() would reject.
inline int validate_inputs(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells, int32_t K) {
    if (!hp || !confs || !n_cells || K <= 0) return fail(MFAS_EINVAL, "null argument or K <= 0");
    if (hp->R < 1 || hp->R > 512 || hp->C < 1 || hp->C > 256) return fail(MFAS_EINVAL, "R must be in [1,512], C in [1,256]");
    if (hp->B < 2 || hp->B > 128) return fail(MFAS_EINVAL, "batchsize must be in [2,128]");
    if (!(hp->drpt > 1e-10) && !hp->bn && !hp->allow_plain_cell)   // ntu_searchable.py:274-284: `op` never assigned
        return fail(MFAS_EINVAL, "illegal cell variant: drpt < 1e-10 without batchnorm (reference: UnboundLocalError)");
    if (hp->drpt >= 1.0) return fail(MFAS_EINVAL, "drpt must be < 1");
    if (hp->loss_mode == 1 && hp->multitask) return fail(MFAS_EINVAL, "multitask applies to the single-label head only");
    for (int j = 0; j < MFAS_MAX_TAPS; ++j)
        if (hp->s_sizes[j] < 0 || hp->v_sizes[j] < 0 || hp->s_sizes[j] > (1 << 20) || hp->v_sizes[j] > (1 << 20))
            return fail(MFAS_EINVAL, "tap widths must be in [0, 2^20]");
    for (int k = 0; k < K; ++k) {
        const int L = n_cells[k];
        if (L < 1 || L > MFAS_MAX_CELLS) return fail(MFAS_EINVAL, "n_cells must be in [1,4]");
        for (int i = 0; i < L; ++i) {
            const int32_t* c = confs + (k * 4 + i) * 3;
            if (c[0] < 0 || c[0] >= MFAS_MAX_TAPS || c[1] < 0 || c[1] >= MFAS_MAX_TAPS || c[2] < 0 || c[2] > 2 ||
                hp->s_sizes[c[0]] < 1 || hp->v_sizes[c[1]] < 1)
                return fail(MFAS_EINVAL, "configuration entry out of range (tap index / unused tap slot / non-linearity)");
        }
    }
    return MFAS_OK;
}

// What the batch-resident kernels (chain_body / chain_lean / sweep_body: the whole padded batch in LDS, MB <= 4 as a template
// parameter, softmax with <= 8 classes per lane) cannot take whatever the LDS says: such a geometry trains on the wide path
// (wide.hip.h), like one whose step does not fit the LDS (plan_layout).
static bool batch_resident_refuses(const mfas_hyper* hp) {
    const int bp = ((hp->B + 15) / 16 == 3 ? 4 : (hp->B + 15) / 16) * 16, lpr = std::min(16, 512 / bp);
    return hp->B > 64 || ((hp->C + 15) & ~15) > 8 * lpr;
}

// The S and V taps cell i of candidate k selects: true and stored (padded to 16) columns.  The one place a configuration is turned into
// widths: plan_chunk's unit count and column total and the candidate layout read it.  (validate_inputs has bounded n_cells and the tap
// indices before any plan is asked for: they are not masked or clamped again here.)
struct CellWidths { int s, v, sp, vp; };
static CellWidths cell_widths(const mfas_hyper* hp, const int32_t* confs, int k, int i) {
    const int32_t* c = confs + (k * 4 + i) * 3;
    const int s = hp->s_sizes[c[0]], v = hp->v_sizes[c[1]];
    return {s, v, ceil16(s), ceil16(v)};
}

static Geo make_geo(const mfas_hyper* hp) {      // (the step-buffer offsets sb_* depend on the widest candidate: plan_layout fills them in)
    Geo g;
    memset(&g, 0, sizeof(g));
    g.R = hp->R; g.C = hp->C; g.Rp = ceil16(hp->R); g.Cp = ceil16(hp->C);
    g.nrb = g.Rp / 16; g.ncb = g.Cp / 16; g.B = hp->B;
    g.MB = (hp->B + 15) / 16; if (g.MB == 3) g.MB = 4;
    g.Bp = g.MB * 16;
    g.bn = hp->bn != 0; g.alphas = hp->alphas != 0; g.multitask = hp->multitask != 0;
    g.use_drop = hp->drpt > 1e-10;
    g.drop_scale = g.use_drop ? (float)(1.0 / (1.0 - hp->drpt)) : 1.0f;
    g.drop_thr = g.use_drop ? (uint32_t)floor(hp->drpt * 16777216.0) : 0u;
    g.bn_eps = (float)hp->bn_eps; g.bn_mom = (float)hp->bn_momentum;
    g.vec_cell_stride = 5 * g.Rp + 16;
    g.vec_head = MFAS_MAX_CELLS * g.vec_cell_stride;
    for (int j = 0; j < MFAS_MAX_TAPS; ++j) { g.sw[j] = ceil16(hp->s_sizes[j]); g.vw[j] = ceil16(hp->v_sizes[j]); }
    g.loss_mode = hp->loss_mode == 1 ? 1 : 0;
    g.f1_th = (float)hp->f1_threshold;
    return g;
}

// ------------------------------------------------------------------------------------------------
// LDS needs, each formula once (bytes)
// ------------------------------------------------------------------------------------------------
// one staged batch of a resident unit: raw 16-bit rows when the caller promised 16-bit taps, f32 rows otherwise
static size_t res_batch_lds(const mfas_hyper* hp, const Geo& g, int cc) {
    return hp->tap_bits == 16 ? (size_t)g.Bp * (cc + 8) * 2 : (size_t)g.Bp * (cc + 4) * 4;
}
// a resident workgroup: nu units x 2 staged batches + the cross-wave reduction slabs + the loop's own words
static size_t res_unit_lds(const mfas_hyper* hp, const Geo& g, int cc, int nu) {
    return (size_t)nu * 2 * res_batch_lds(hp, g, cc) + (size_t)STEP_NW * g.MB * 256 * 4 + 4 * PERSIST_LDS_WORDS + 64;
}
// a streaming sweep unit (sweep_body): x_t, x_{t+1} and dy (+ the k-split reduction slabs: forward only)
static size_t sweep_unit_lds(const Geo& g, const SegDesc& d) {
    const int nrb = d.rows_p / 16;
    size_t fl = (size_t)g.Bp * (d.cc + 16) + (size_t)g.Bp * (d.cc + 4) + (size_t)g.Bp * (d.rows_p + 16);
    if (nrb < STEP_NW && d.kind <= KIND_V) fl += (size_t)STEP_NW * nrb * g.MB * 256;
    return fl * 4;
}
// the same feature unit in a double pass (deferred stores): + the replayed step's rows and dy, which a k-split unit lays over the
// reduction slabs of its LAST row block (sweep_body)
static size_t sweep_unit_lds_double(const Geo& g, const SegDesc& d) {
    const int nrb = d.rows_p / 16;
    const size_t replay = (size_t)g.Bp * (d.cc + 16) + (size_t)g.Bp * (d.rows_p + 16), slab = (size_t)STEP_NW * g.MB * 256;
    size_t fl = (size_t)g.Bp * (d.cc + 16) + (size_t)g.Bp * (d.cc + 4) + (size_t)g.Bp * (d.rows_p + 16);
    fl += nrb < STEP_NW ? (size_t)(nrb - 1) * slab + std::max(slab, replay) : replay;
    return fl * 4;
}
// the wide path (wide.hip.h): a sweep unit's batch slice of x_t, x_{t+1} and dy; the chain's rows in flight, logits and statistics
static size_t wide_unit_lds(const SegDesc& d) {
    return (size_t)wide_sweep_lds(0, std::min(16 * WIDE_KB, d.cc), std::min(16 * WIDE_RBG, d.rows_p)).total * 4;
}
static size_t wide_chain_lds(const Geo& g) { return wide_chain_lds_floats(g.Rp, g.Cp, g.Bp) * 4; }
// a candidate's vector block, three planes
static size_t vec_lds(const Geo& g) { return (size_t)3 * (MFAS_MAX_CELLS * g.vec_cell_stride + g.Cp) * 4; }
// chain_lean: out_i / dy_i of all cells, logits, misc, reduced sums, vector block, saved activations
static size_t lean_chain_lds(const Geo& g) {
    return ((size_t)2 * MFAS_MAX_CELLS * g.Bp * 20 + (size_t)g.Bp * (g.Cp + 4) + MFAS_MAX_CELLS * 16 + 3 * g.Bp + 16
            + (size_t)(g.alphas ? 2 : 1) * MFAS_MAX_CELLS * g.MB * 256 + vec_lds(g) / 4 + LEAN_SCR + 8 + lean_stage_floats() + (size_t)g.Bp * 64) * 4;
}

// ------------------------------------------------------------------------------------------------
// Column chunk: which chunk the feature segments are cut into and whether the population takes the RESIDENT persistent
// schedule (k_president: every chain and every feature unit resident, W/m/v in registers).
// ------------------------------------------------------------------------------------------------
struct ChunkPlan {
    bool want_persist = false;
    int target = 0, nu = 1;          // feature-column chunk, units per resident workgroup
    bool plan_res = false;           // the chunk was chosen for the resident schedule
    int nfeat = 0, max_fcc = 0;      // feature units and the widest of them at that chunk
    bool res_ok = false, res_wide = false, lean_ok = false;
    int nres_wg = 0;
    bool resident = false;           // the resident persistent schedule runs
};

struct PlanIn {                      // plan_layout's arguments + which of the two kernel families is planned for
    const mfas_hyper* hp;
    const int32_t* confs;
    const int32_t* n_cells;
    const uint32_t* drop_seeds;
    int K, chunk_cols, n_cus;
    bool allow_persist;
    const Tuning& tu;
    bool wide;
};

// feature units of the population when its S / V segments are cut into chunks of <= cc_target columns, and the widest of them
static int64_t feature_units(const PlanIn& in, int cc_target, int* max_cc) {
    int64_t n = 0;
    int mx = 0;
    for (int k = 0; k < in.K; ++k)
        for (int i = 0; i < in.n_cells[k]; ++i) {
            const CellWidths w = cell_widths(in.hp, in.confs, k, i);
            const int cs = pick_chunk(w.sp, cc_target), cv = pick_chunk(w.vp, cc_target);
            n += w.sp / cs + w.vp / cv;
            mx = std::max(mx, std::max(cs, cv));
        }
    if (max_cc) *max_cc = mx;
    return n;
}

// `units` resident units of cc columns, nu per workgroup: tiles per wave, LDS, and a CU for every chain and every unit workgroup
static bool res_units_fit(const PlanIn& in, const Geo& g, int cc, int nu, int64_t units) {
    return (cc <= 128 * PERSIST_NTR || (in.hp->tap_bits == 16 && nu == 1 && cc <= 128 * PERSIST_NTR16)) &&
           res_unit_lds(in.hp, g, cc, nu) <= 160 * 1024 && in.K + (units + nu - 1) / nu <= in.n_cus;
}

// The launch-per-phase chunk: a workgroup should stream >= ~64 tiles (amortises staging / reduction and keeps the number of partial-sum
// chunks the chain has to reduce small), the launch should still have a few hundred workgroups, and x_t / x_{t+1} for the chunk must
// fit the LDS budget.
static int streaming_chunk(const PlanIn& in, const Geo& g) {
    double tot_cols = 0;
    for (int k = 0; k < in.K; ++k)
        for (int i = 0; i < in.n_cells[k]; ++i) { const CellWidths w = cell_widths(in.hp, in.confs, k, i); tot_cols += w.sp + w.vp; }
    int lds_max = 64;                                   // largest power of two with Bp*(2cc+20)*4 <= 72 KiB
    while ((size_t)g.Bp * (8 * lds_max + 20) * 4 <= 72 * 1024 && lds_max < 1024) lds_max <<= 1;   // test the doubled size
    int target = 64;
    while (target * g.nrb < 64 * 16 && target < lds_max) target <<= 1;      // >= 64 tiles per workgroup
    while (target > 64 && tot_cols / target < 320.0) target >>= 1;           // ... but keep >= ~320 workgroups
    // R >= 128, measured on MI355X: 64-column chunks (finer, better-balanced workgroups) win once
    // the chain is hidden under the other group's sweep (K >= 20); below that fewer partial chunks matter more
    // (round 2: with reduce-in-sweep the number of partial slabs no longer loads the chain; 256-column chunks stay best up
    // to ~28 candidates, 64 beyond — profiles/r02_popsweep_r128.log)
    if (g.nrb >= 8) target = std::min(target, in.K >= 28 ? 64 : 256);
    return target;
}

static ChunkPlan plan_chunk(const PlanIn& in, const Geo& g, bool allow_persist) {
    const Tuning& tu = in.tu;
    ChunkPlan lp;
    // Persistent step loop (persist.hip.h): with one row block (R <= 16) the feature units become RESIDENT (one workgroup per
    // unit, or two units per workgroup; W/m/v in registers): the column chunk is then the smallest of 128 / 256 / 512 / 1024
    // columns with which every chain and every unit workgroup gets a CU of its own.
    // Default (measured, profiles/r02_popsweep_*.log, r03_popsweep.log): ON where the resident form fits (x1.6-2.1 over the
    // launch-per-phase schedule at 4..28 candidates per GPU).  Nothing else is persistent: the streaming form of round 2 (larger R,
    // or units that do not fit; x0.8-0.9 of launch-per-phase) was removed in round 3.  MFAS_PERSIST=0 turns the schedule off.
    lp.want_persist = allow_persist && tu.persist != 0;
    // (the chain form must not depend on the sweep's chunk size: since round 2 the lean chain sums bias gradients and BN
    // statistics in its own — element-parallel — order, so lean and general chains agree to rounding, not bit for bit)
    lp.lean_ok = g.nrb == 1 && g.ncb <= 4 && g.MB <= 2 && lean_chain_lds(g) <= 78 * 1024 && !tu.no_lean_chain;
    // (resident units exist only together with the resident lean chain — k_president; a population without both runs launch-per-phase)
    lp.plan_res = lp.want_persist && g.nrb == 1 && g.MB <= 2 && lp.lean_ok;
    lp.target = in.chunk_cols;
    lp.nu = 1;
    if (lp.plan_res && lp.target <= 0) {
        // smallest units first (fewest tiles per wave on the critical path); two units per workgroup before 1024-column units
        // (measured: 16 candidates, 1024-column units: 34.8 us per step)
        // (two 256-column units per workgroup before one 512-column unit: 9..15 candidates 15.7-16.2 vs 18.0-18.7 us per step)
        // (round 5: 128-column units are out — twice the partial slabs through the chain's one CU for half the tiles per wave:
        //  3 / 4 candidates 23.9 / 23.7 us per step against 18.8 / 18.8 with 256-column units, profiles/r05_popsweep_units.log)
        const int opts[5][2] = {{256, 1}, {256, 2}, {512, 1}, {512, 2}, {1024, 1}};
        int pick = -1;
        for (int o = 0; o < 5 && pick < 0; ++o)
            if (res_units_fit(in, g, opts[o][0], opts[o][1], feature_units(in, opts[o][0], nullptr))) pick = o;
        if (pick >= 0) { lp.target = opts[pick][0]; lp.nu = opts[pick][1]; }
        else lp.plan_res = false;
    } else if (lp.plan_res) {
        const int64_t units = feature_units(in, lp.target, nullptr);
        if (res_units_fit(in, g, lp.target, 1, units)) lp.nu = 1;
        else if (res_units_fit(in, g, lp.target, 2, units)) lp.nu = 2;
        else lp.plan_res = false;
    }
    if (lp.target <= 0) lp.target = streaming_chunk(in, g);
    lp.target = std::max(16, (lp.target / 16) * 16);
    lp.nfeat = (int)feature_units(in, lp.target, &lp.max_fcc);
    lp.res_ok = lp.plan_res && res_units_fit(in, g, lp.max_fcc, lp.nu, lp.nfeat);
    lp.res_wide = lp.res_ok && lp.max_fcc > 128 * PERSIST_NTR;      // 16-bit staging only
    lp.nres_wg = lp.res_ok ? (lp.nfeat + lp.nu - 1) / lp.nu : 0;
    // persistent step loop: small populations (one workgroup per CU must hold every chain + a useful number of sweep workgroups)
    lp.resident = lp.want_persist && lp.res_ok && in.K <= in.n_cus / 4 && g.MB != 4 && in.K + lp.nres_wg <= in.n_cus;
    return lp;
}

// ------------------------------------------------------------------------------------------------
// Layout plan: the complete, immutable description of a population — geometry, per-candidate records and descriptors, the schedule,
// every LDS budget and the work lists of every launch — as a pure function of the geometry, the configurations, the CU count and the
// switches.  mfas_population keeps it as one member; nothing in it changes after create.
// ------------------------------------------------------------------------------------------------
struct GroupPlan {                   // a contiguous candidate range with its own sweep work list
    int c0 = 0, nc = 0;
    double alg_state = 0, alg_feat = 0;
    std::vector<SegDesc> descs;      // per-segment units, largest first (same-group launch: in the order the chain releases them)
    std::vector<TapDesc> taps;       // tap-major units (small R); empty: every feature unit is in descs
};

struct LayoutPlan {
    Geo g;
    int chunk = 0;                   // feature-column chunk the segments were cut with
    std::vector<CandDev> cands;
    std::vector<SegDesc> descs;
    std::vector<int> desc_start;     // K+1
    std::vector<int64_t> nparams;
    std::vector<int64_t> cand_plane_base, cand_plane_size;
    int64_t plane_stride = 0, wt_size = 0, step_total = 0;
    double bytes_per_launch = 0.0;   // algorithmic bytes of one update + forward sweep of the whole population (f32 tables)
    // schedule
    bool persist = false;            // persistent step loop (persist.hip.h): one launch per epoch, per-candidate dependencies
    bool res_chain = false;          // resident lean chain: owns OUT / HEAD + vector block on chip; persistent units = feature units only
    bool res_wide = false;           // resident units of more than 512 columns (16-bit staging): f32 tables cannot be trained
    int nres = 0;                    // resident feature units (W/m/v in registers)
    int res_nu = 1;                  // resident units per workgroup (2: a workgroup serves units of two candidates)
    int nres_wg = 0;                 // resident workgroups = ceil(nres / res_nu)
    int res_buf_words = 0;           // LDS words of one staged batch of a resident unit
    bool wide = false;               // the wide path (wide.hip.h: k_chain_wide + k_sweep_wide, launch per phase, batch walked in tiles): exactly
                                     // the geometries the batch-resident kernels refuse; no resident / same-group / chain_split / A-B schedule
    std::vector<int> wide_start;     // [K+1] first wide unit of every candidate in groups[0].descs (candidate-major)
    bool lean_chain = false;         // chain_lean (R <= 16, C <= 64, B <= 32) in standalone and fused launches
    bool same_group = false;         // one launch per step: chain blocks + sweep blocks of the same candidates, per-cell dy flags (k_step_same)
    int chain_split = 0;             // CUs per candidate chain in the same-group launch (0 / 1: chain_body on one CU; 4: chain_split<4>)
    bool red_in_sweep = false;       // reduce-in-sweep arrival counters [K][4] (small populations, general chain)
    bool nontemporal = false;
    bool defer = false;              // feature segments store W / m / v every second step (launches.hip.h, mark_deferred)
    int64_t sb_dy_alt = 0;           // deferring plans: the second dy area of a candidate's step buffers (Geo::sb_dy is the first)
    double occ_bytes = 0;           // MB == 2: group state bytes/launch above which the sweep (not the chain) bounds a fused launch
    int mbe = 4, nrbw = 1;           // dev pass: batch tiles per workgroup, row blocks per wave
    bool yf_in_lds = false, vec_in_lds = false;
    size_t lds_step = 0, lds_chain = 0, lds_eval = 0;
    bool fits_lds = false;           // the geometry fits the 160 KiB LDS (R / batchsize not too large)
    size_t lds_split = 0;            // dynamic LDS of the chain_split launches
    size_t lds_president = 0;        // resident form (k_president)
    // work lists
    std::vector<GroupPlan> groups;   // 1 or 2
    std::vector<SegDesc> pdescs;     // resident schedule's unit list: the feature units
    std::vector<int32_t> need;       // [K] resident units per candidate
    std::vector<int32_t> role;       // [K + nres_wg] role of every workgroup of the resident launch (XCD-aware placement); empty: block b runs role b
};

// ---- the stages of plan_layout_as, in the order they run: each reads the inputs (PlanIn) and what earlier stages wrote into the plan
// Stage 1, the column chunk.  reads: the inputs, Geo.  returns: the chunk and, for the batch-resident kernels, whether the resident
// schedule stands (plan_chunk).
static ChunkPlan choose_chunk(const PlanIn& in, const Geo& g) {
    ChunkPlan lp;
    if (in.wide) {   // feature chunks of <= 8 k-blocks: one wide unit keeps a chunk's dW tiles of its row block in registers
        lp.target = in.chunk_cols > 0 ? std::min(16 * WIDE_KB, in.chunk_cols) : 16 * WIDE_KB;
        lp.target = std::max(16, (lp.target / 16) * 16);
        return lp;
    }
    lp = plan_chunk(in, g, in.allow_persist);
    if (lp.res_ok && !lp.resident)    // units were chosen for the resident schedule, which does not stand: the launch-per-phase chunking
        lp = plan_chunk(in, g, false);
    return lp;
}

// The descriptor of a whole weight matrix segment — a cell's S, V or OUT columns (rows = R) or the head (rows = C) — with everything its
// chunks share; the caller cuts it: tap, k0, cc, w_off, wt_off, part_idx.
static SegDesc make_seg(int cand, int kind, int cell, int rows, int rows_p, int cols, int width, int64_t src_off, int src_ld, int src_col0,
                        uint32_t init_seed, int fan_in) {
    SegDesc d;
    memset(&d, 0, sizeof(d));
    d.cand = cand; d.kind = kind; d.cell = cell;
    d.rows = rows; d.rows_p = rows_p; d.cols = cols; d.width = width;
    d.src_off = src_off; d.src_ld = src_ld; d.src_col0 = src_col0;
    d.init_seed = init_seed; d.init_bound = (float)(1.0 / sqrt((double)fan_in));
    d.rb0 = 0; d.seg_nrb = rows_p / 16;
    return d;
}

struct LayoutCursor {                // where the next candidate goes
    int64_t plane = 0, wt = 0;       // floats into a W / m / v plane, into the transposed arena
    double alg_bytes = 0, alg_feat = 0;
};

// One candidate at the cursor: its record (flat-parameter offsets in state_dict order, plane and arena offsets, chunk counts) and its
// descriptors — per cell the S and V chunks of `pl.chunk` columns and, from the second cell on, OUT; then the head.
// reads: the inputs, Geo, pl.chunk.  writes: pl.cands[k], pl.nparams[k], appends to pl.descs, moves the cursor.  returns: the
// candidate's partial slots (one per feature chunk).
static int layout_candidate(const PlanIn& in, int k, LayoutCursor& cur, LayoutPlan& pl) {
    const mfas_hyper* hp = in.hp;
    const Geo& g = pl.g;
    CandDev& c = pl.cands[k];
    memset(&c, 0, sizeof(c));
    const int L = c.L = in.n_cells[k];
    c.drop_seed = in.drop_seeds ? in.drop_seeds[k] : (uint32_t)k;
    c.gidx = k;
    c.vec_off = cur.plane;
    cur.plane += (g.vec_head + g.Cp + 63) & ~63;
    int64_t f = 0;
    c.f_alpha = f; f += L;
    int pslot = 0;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < 3; ++j) { c.conf[i][j] = in.confs[(k * 4 + i) * 3 + j]; c.seg_off[i][j] = -1; }
        const CellWidths w = cell_widths(hp, in.confs, k, i);
        const int Kin = c.K_in[i] = w.s + w.v + (i > 0 ? hp->R : 0);
        c.f_W[i] = f; f += (int64_t)hp->R * Kin;
        c.f_b[i] = f; f += hp->R;
        c.f_bn[i] = f; if (hp->bn) f += 4 * (int64_t)hp->R;
        c.part_cell_off[i] = pslot;
        const int widths[3] = {w.sp, w.vp, g.Rp};        // stored (padded) columns = table row stride
        const int true_w[3] = {w.s, w.v, hp->R};         // reference columns
        const int col0[3] = {0, w.s, w.s + w.v};
        for (int j = 0; j < (i == 0 ? 2 : 3); ++j) {     // (the first cell has no OUT segment)
            const int cols_p = widths[j], cc = j < 2 ? pick_chunk(cols_p, pl.chunk) : cols_p, nch = cols_p / cc;
            c.seg_off[i][j] = cur.plane; c.seg_cc[i][j] = cc; c.seg_cols[i][j] = cols_p;
            if (j == 0) c.nch_s[i] = nch;
            if (j == 1) c.nch_v[i] = nch;
            if (j == 2) c.outT_off[i] = cur.wt;
            SegDesc d = make_seg(k, j, i, hp->R, g.Rp, true_w[j], cols_p, c.f_W[i], Kin, col0[j], 2 * i, Kin);
            d.tap = j < 2 ? c.conf[i][j] : 0; d.cc = cc; d.wt_off = j == 2 ? cur.wt : -1;
            for (int ch = 0; ch < nch; ++ch) {
                d.k0 = ch * cc; d.w_off = cur.plane + (int64_t)ch * g.Rp * cc;
                d.part_idx = j == 0 ? ch : (j == 1 ? c.nch_s[i] + ch : 0);      // one partial slab per chunk
                pl.descs.push_back(d);
            }
            if (j < 2) pslot += nch;
            cur.plane += (int64_t)g.Rp * cols_p;
            if (j == 2) cur.wt += (int64_t)g.Rp * g.Rp;
            cur.alg_bytes += 24.0 * hp->R * true_w[j];
            if (j < 2) cur.alg_feat += (double)hp->B * true_w[j];   // x elements (dtype size applied at train time)
        }
    }
    c.f_Wc = f; f += (int64_t)hp->C * hp->R;
    c.f_bc = f; f += hp->C;
    pl.nparams[k] = f;
    c.head_off = cur.plane;
    c.headT_off = cur.wt;
    SegDesc d = make_seg(k, KIND_HEAD, L - 1, hp->C, g.Cp, hp->R, g.Rp, c.f_Wc, hp->R, 0, 10, hp->R);
    d.cc = g.Rp; d.w_off = cur.plane; d.wt_off = cur.wt;
    pl.descs.push_back(d);
    cur.plane += (int64_t)g.Cp * g.Rp;
    cur.wt += (int64_t)g.Cp * g.Rp;
    cur.alg_bytes += 24.0 * hp->C * hp->R;
    cur.plane = (cur.plane + 63) & ~63LL;
    return pslot;
}

// Stage 2, the candidate layout.  reads: the inputs, Geo, pl.chunk.  writes: cands (all but step_off), descs, desc_start, nparams,
// cand_plane_base / _size, plane_stride, wt_size, bytes_per_launch.  returns: the partial slots of the widest candidate.
static int layout_candidates(const PlanIn& in, LayoutPlan& pl) {
    const int K = in.K;
    pl.cands.resize(K);
    pl.desc_start.assign(K + 1, 0);
    pl.nparams.resize(K);
    pl.cand_plane_base.resize(K);
    pl.cand_plane_size.resize(K);
    LayoutCursor cur;
    int max_slots = 0;
    for (int k = 0; k < K; ++k) {
        pl.desc_start[k] = (int)pl.descs.size();
        pl.cand_plane_base[k] = cur.plane;
        max_slots = std::max(max_slots, layout_candidate(in, k, cur, pl));
        pl.cand_plane_size[k] = cur.plane - pl.cand_plane_base[k];
    }
    pl.desc_start[K] = (int)pl.descs.size();
    pl.plane_stride = cur.plane;
    pl.wt_size = cur.wt;
    pl.bytes_per_launch = cur.alg_bytes + 4.0 * cur.alg_feat;
    return max_slots;
}

// Stage 3, the LDS budgets of the training kernels.  reads: Geo, descs, the chunk plan.  writes: lds_step, lds_chain, lds_president,
// yf_in_lds, vec_in_lds, lean_chain and — taken over from the chunk plan — persist, res_chain, res_wide, nres, res_nu, nres_wg,
// res_buf_words.  (The wide plan has none of the resident facts: they keep their defaults.)
static void lds_budgets(const PlanIn& in, const ChunkPlan& lp, LayoutPlan& pl) {
    const Geo& g = pl.g;
    if (in.wide) {
        for (const SegDesc& d : pl.descs) pl.lds_step = std::max(pl.lds_step, wide_unit_lds(d));
        pl.lds_chain = wide_chain_lds(g);
        return;
    }
    // resident feature units (persistent schedule) do not go through sweep_body: their LDS need is separate
    pl.persist = lp.resident;
    pl.res_chain = lp.res_ok;
    pl.res_wide = lp.res_wide;
    pl.nres = lp.res_ok ? lp.nfeat : 0;
    pl.res_nu = lp.nu;
    pl.nres_wg = lp.nres_wg;
    pl.res_buf_words = (int)(res_batch_lds(in.hp, g, lp.max_fcc) / 4);
    size_t ls = 0;
    for (const SegDesc& d : pl.descs)
        if (!(lp.res_ok && d.kind <= KIND_V)) ls = std::max(ls, sweep_unit_lds(g, d));
    // chain: ping-pong activations + logits + misc (+ reduced feature sums when they fit next to the sweep's need)
    const size_t base = ((size_t)2 * g.Bp * (g.Rp + 4) + (size_t)g.Bp * (g.Cp + 4) + MFAS_MAX_CELLS * g.Rp + 3 * g.Bp + 16) * 4;
    const size_t yf = (size_t)(g.alphas ? 2 : 1) * MFAS_MAX_CELLS * g.nrb * g.MB * 256 * 4;
    pl.yf_in_lds = base + yf <= std::max<size_t>(ls, 64 * 1024);
    pl.lds_step = std::max(ls, base + (pl.yf_in_lds ? yf : 0));
    const size_t vec = vec_lds(g);
    pl.vec_in_lds = base + (pl.yf_in_lds ? yf : 0) + vec <= 150 * 1024;
    pl.lds_chain = base + (pl.yf_in_lds ? yf : 0) + (pl.vec_in_lds ? vec : 0);
    pl.lean_chain = lp.lean_ok;
    if (pl.lean_chain) { pl.lds_chain = lean_chain_lds(g); pl.lds_step = std::max(pl.lds_step, pl.lds_chain); }
    const size_t lds_rchain = pl.res_chain ? pl.lds_chain + 16 + 4 * (size_t)(lean_own_floats() - lean_stage_floats()) : 0;
    pl.lds_president = ((std::max(lds_rchain, res_unit_lds(in.hp, g, lp.max_fcc, lp.nu)) + 15) & ~(size_t)15) + 4 * PERSIST_LDS_WORDS;
}

// Stage 4, the dev pass and what streams.  reads: Geo, lds_step, lds_chain, plane_stride.  writes: nrbw, mbe, lds_eval, fits_lds, occ_bytes,
// nontemporal.
static void dev_pass_and_streaming(const PlanIn& in, LayoutPlan& pl) {
    const Geo& g = pl.g;
    // dev-pass row blocks per wave: k_eval is built for 1, 2, 4 and 8 (eval.hip.h clamps / skips row blocks >= nrb), so 3 and
    // 5..7 (R = 257..448) take the next build up
    pl.nrbw = (g.nrb + 3) / 4;
    if (pl.nrbw == 3) pl.nrbw = 4;
    else if (pl.nrbw > 4 && pl.nrbw < 8) pl.nrbw = 8;
    for (pl.mbe = 4; pl.mbe >= 1; pl.mbe >>= 1) {
        const int ME = pl.mbe * 16;
        pl.lds_eval = ((size_t)ME * std::max(EVAL_CE + 8, g.Cp + 4) + (size_t)ME * (g.Rp + 8)) * 4;   // strides: eval.hip.h
        if (pl.lds_eval <= 80 * 1024) break;
    }
    // (create refuses what does not fit; the plan query still answers)
    pl.fits_lds = !(pl.mbe < 1 || pl.nrbw > 8 || pl.lds_step > 150 * 1024 || (in.wide && pl.lds_chain > 150 * 1024));
    // measured crossover (MI355X, B=20): R=16 between 165 and 330 MB of group state per launch, R=128 between 300 and 600 MB
    // (the spilling chain of the occupancy build takes ~40 / ~125 us there)
    pl.occ_bytes = g.nrb >= 8 ? 450e6 : 250e6;
    if (in.tu.occ_bytes >= 0) pl.occ_bytes = in.tu.occ_bytes;
    // W/m/v beyond what the 256 MiB Infinity Cache can keep between steps are streamed nontemporally
    pl.nontemporal = (double)pl.plane_stride * 12.0 > 200.0 * 1024 * 1024;
    if (in.tu.nt >= 0) pl.nontemporal = in.tu.nt != 0;
}

// Which of its five schedules a population trains under.  They exclude each other, and the LayoutPlan flags the consumers read
// (wide, persist, same_group, groups.size(), chain_split, red_in_sweep, defer, tap-major units) all follow from this one choice.
enum class Sched {
    Wide,        // wide.hip.h, launch per phase, one group: exactly the geometries the batch-resident kernels refuse
    Resident,    // k_president: one launch per epoch
    SameGroup,   // k_step_same: one launch per step, chain and sweep blocks of the same candidates
    OneGroup,    // launch per phase: chain, then sweep
    TwoGroups,   // launch per phase, fused: the chain of one group runs under the sweep of the other
};
static bool launch_per_phase(Sched s) { return s == Sched::OneGroup || s == Sched::TwoGroups; }

// Stage 5, the schedule.  reads: the inputs, Geo, descs, persist, lean_chain.
static Sched choose_schedule(const PlanIn& in, const LayoutPlan& pl) {
    const Tuning& tu = in.tu;
    const int K = in.K;
    if (in.wide) return Sched::Wide;
    if (pl.persist) return Sched::Resident;
    // same-group fused launch (k_step_same): general chain, launch-per-phase.  MFAS_SAME_GROUP = 0: never, 2: whatever the size (A/B runs);
    // MFAS_GROUPS=2 (tests: the two-group fused schedule) goes before it.
    // measured (MI355X, conf 4, B=16): pays while the population's W/m/v stream is <= ~260 MB per step — R=128: 1 / 3 / 6 / 8 / 12
    // candidates 56 / 65 / 76 / 81 / 91 -> 50 / 54 / 63 / 70 / 88 us per step (16: equal); R=64: 6 / 12 / 16: 52 / 61 / 64 -> 45 / 55 / 61
    // (24: 74 -> 79); R=32: 6 / 12 / 32: 45 / 54 / 68 -> 36 / 41 / 60 (64: 85 -> 90)
    double state_bytes = 0;
    for (const SegDesc& d : pl.descs) state_bytes += 24.0 * d.cc * d.rows_p;
    if (!pl.lean_chain && pl.g.MB <= 2 && (state_bytes <= 260e6 || tu.same_group == 2) && tu.same_group != 0 && tu.groups < 2) return Sched::SameGroup;
    // Two groups (the chain of one runs under the sweep of the other).  Measured on MI355X (cand/s, unfused vs fused):
    // general chain, R=128: 16 candidates 104 vs 96, 20: 103 vs 110, 32: 119 vs 142 -> fused from 20;
    // lean chain, R=16 (18 us, cheap enough to run as its own launch over all CUs): 32: 348 vs 307, 40: 361 vs 364,
    // 50: 430 vs 475, 100: 582 vs 677, 200: 566 vs 600, 256: 630 vs 619, 512: 685 vs 641 -> fused only for 40 <= K < 224.
    // round 2, general chain with reduce-in-sweep (chain 48 -> 38 us at R=128): fused from 8 candidates
    // (R=128 cand/s unfused+reduce vs fused+reduce: 12 candidates 18.1 vs 20.2, 16: 21.0 vs 23.6, 24: 22.9 (old default) vs 26.6)
    bool two = pl.lean_chain ? (K >= 40 && K < 224) : K >= 8;
    if (tu.groups > 0) two = tu.groups >= 2 && K >= 2;
    return two ? Sched::TwoGroups : Sched::OneGroup;
}

// What follows from the schedule before the work lists are built.  writes: same_group, chain_split, lds_split.
static int schedule_flags(const PlanIn& in, Sched s, LayoutPlan& pl) {
    const Geo& g = pl.g;
    pl.same_group = s == Sched::SameGroup;
    // the chain of one candidate over 4 CUs (chain.hip.h, chain_split): eight row blocks, one batch tile, <= 4 class blocks, no alphas
    // — in the same-group launch, and in the two-group launches while the chain bounds them (< 28 candidates: sweep(8 candidates) = 36 us
    // against a 47 us chain; beyond, the chain hides under the other group's sweep and 4 x 64 chain workgroups would only take CUs from it)
    pl.chain_split = ((s == Sched::SameGroup || (s == Sched::TwoGroups && in.K < 28)) && !pl.lean_chain && g.MB == 1 && g.nrb == 8 && g.ncb <= 4 &&
                      !g.alphas && in.tu.chain_split != 0 && in.tu.chain_split != 1) ? 4 : 0;
    if (pl.chain_split) {
        pl.lds_split = std::max(pl.lds_step, chain_split_lds_floats<4>(g.Rp, g.Cp) * 4);
        if ((size_t)in.K * XCH_CAND_FLOATS >= (1ull << 30)) return fail(MFAS_EINVAL, "internal: exchange area beyond the 32-bit buffer offsets");
    }
    return MFAS_OK;
}

// Stage 6, the balanced group split of the two-group schedule: contiguous halves balanced by work (descriptor columns).
// reads: descs, desc_start.  returns: the first candidate of the second group.
static int balanced_split(const LayoutPlan& pl, int K) {
    double tot = 0, run = 0;
    for (const SegDesc& d : pl.descs) tot += (double)d.cc * d.rows_p;
    int split = 1;
    for (int k = 0; k < K - 1; ++k) {
        for (int j = pl.desc_start[k]; j < pl.desc_start[k + 1]; ++j) run += (double)pl.descs[j].cc * pl.descs[j].rows_p;
        split = k + 1;
        if (run >= tot / 2) break;
    }
    return split;
}

// Row blocks r0 .. r0 + nrows - 1 of a descriptor as a unit of their own (SegDesc::rb0 / seg_nrb; w_off points at row block r0 of the chunk)
static SegDesc row_block_unit(const SegDesc& d, int r0, int nrows) {
    SegDesc u = d;
    u.rb0 = r0; u.rows_p = 16 * nrows; u.seg_nrb = d.rows_p / 16;
    u.w_off = d.w_off + (int64_t)r0 * (d.cc / 16) * 256;
    return u;
}

// Small R (1, 2 or 4 row blocks): the feature segments of `all` regrouped tap-major (sweep_tap_body), up to STEP_NW / nrb segments of one
// tap chunk per workgroup, largest first; the other segments go to `rest`.
static std::vector<TapDesc> tap_major_units(const std::vector<SegDesc>& all, int per_wg, std::vector<SegDesc>& rest) {
    std::vector<TapDesc> taps;
    std::vector<const SegDesc*> feat;
    for (const SegDesc& d : all) { if (d.kind <= KIND_V) feat.push_back(&d); else rest.push_back(d); }
    std::stable_sort(feat.begin(), feat.end(), [](const SegDesc* x, const SegDesc* y) {
        if (x->kind != y->kind) return x->kind < y->kind;
        if (x->tap != y->tap) return x->tap < y->tap;
        if (x->cc != y->cc) return x->cc < y->cc;
        return x->k0 < y->k0;
    });
    for (size_t i0 = 0; i0 < feat.size();) {
        TapDesc t;
        memset(&t, 0, sizeof(t));
        const SegDesc* f0 = feat[i0];
        t.kind = f0->kind; t.tap = f0->tap; t.k0 = f0->k0; t.cc = f0->cc; t.rows_p = f0->rows_p; t.width = f0->width;
        while (i0 < feat.size() && t.nitems < per_wg && feat[i0]->kind == t.kind && feat[i0]->tap == t.tap &&
               feat[i0]->k0 == t.k0 && feat[i0]->cc == t.cc) {
            t.cand[t.nitems] = feat[i0]->cand; t.cell[t.nitems] = feat[i0]->cell;
            t.part_idx[t.nitems] = feat[i0]->part_idx; t.w_off[t.nitems] = feat[i0]->w_off;
            ++t.nitems; ++i0;
        }
        taps.push_back(t);
    }
    std::stable_sort(taps.begin(), taps.end(), [](const TapDesc& x, const TapDesc& y) { return x.nitems * x.cc > y.nitems * y.cc; });
    return taps;
}

// wide units: <= 8 row blocks (one per wave) x <= 8 k-blocks of a layout chunk, candidate-major (train-mode single batches
// launch one candidate's range).  The plane layout is the batch-resident one — OUT / HEAD stay ONE chunk of Rp columns, which the
// chain, the dev pass and the packers index — so their units name a k-block range inside it (SegDesc::sub_kb0 / sub_nkb).
// writes: pl.wide_start.
static std::vector<SegDesc> wide_units(int K, LayoutPlan& pl) {
    std::vector<SegDesc> fine;
    pl.wide_start.assign(K + 1, 0);
    for (int k = 0; k < K; ++k) {
        pl.wide_start[k] = (int)fine.size();
        for (int j = pl.desc_start[k]; j < pl.desc_start[k + 1]; ++j) {
            const SegDesc& d = pl.descs[j];
            const int nrb_d = d.rows_p / 16, nkb_d = d.cc / 16;
            for (int r0 = 0; r0 < nrb_d; r0 += WIDE_RBG)
                for (int q0 = 0; q0 < nkb_d; q0 += WIDE_KB) {
                    SegDesc u = row_block_unit(d, r0, std::min(WIDE_RBG, nrb_d - r0));
                    u.sub_kb0 = q0; u.sub_nkb = std::min(WIDE_KB, nkb_d - q0);
                    fine.push_back(u);
                }
        }
    }
    pl.wide_start[K] = (int)fine.size();
    return fine;
}

// The same-group launch's units.  OUT / HEAD units one ROW BLOCK each (round 6): as ONE workgroup per 128 x 128 segment every wave walked
// its row block's eight tiles in four dependent load -> Adam -> store rounds of ~2.5 us behind the dy it waits for — OUT_1, released by the
// LAST dy of the step, ended 12.7 us after the chain where the cell-0 feature units end after 6.2 (profiles/r06_chain_split_r128.log).
// Row-split units (one tile per wave: the k-split walk) update the same tiles with the same arithmetic.  Then the order the chain releases
// the units in.
static std::vector<SegDesc> same_group_units(const std::vector<SegDesc>& sorted) {
    std::vector<SegDesc> fine;
    for (const SegDesc& d : sorted) {
        const int nrb_d = d.rows_p / 16;
        if (d.kind <= KIND_V || nrb_d <= 1) { fine.push_back(d); continue; }
        for (int r0 = 0; r0 < nrb_d; ++r0) fine.push_back(row_block_unit(d, r0, 1));
    }
    std::stable_sort(fine.begin(), fine.end(), [](const SegDesc& x, const SegDesc& y) {
        // (the slot each unit waits for: feature units of cell i -> i, OUT_i -> i - 1, HEAD -> the last cell; highest slot first)
        auto slot = [](const SegDesc& d) { return d.kind == KIND_HEAD ? MFAS_MAX_CELLS : (d.kind == KIND_OUT ? d.cell - 1 : d.cell); };
        return slot(x) > slot(y);
    });
    return fine;
}

// Stage 7, one group's work list: candidates c0 .. c0 + nc - 1.  reads: the inputs, the schedule, Geo, descs, desc_start.
// returns: the group with its per-segment units (largest first; wide: candidate-major; same-group: release order) and tap-major units.
static GroupPlan group_work_list(const PlanIn& in, Sched s, int c0, int nc, LayoutPlan& pl) {
    const Geo& g = pl.g;
    GroupPlan gr;
    gr.c0 = c0; gr.nc = nc;
    std::vector<SegDesc> all(pl.descs.begin() + pl.desc_start[c0], pl.descs.begin() + pl.desc_start[c0 + nc]);
    for (const SegDesc& d : all) {
        gr.alg_state += 24.0 * d.rows * std::max(0, std::min(d.cc, d.cols - d.k0));
        if (d.kind <= KIND_V) gr.alg_feat += (double)in.hp->B * d.cc;
    }
    if (s == Sched::Wide) { gr.descs = wide_units(in.K, pl); return gr; }
    // (tap-major workgroups stage a batch's rows ONCE for several candidates: not with per-candidate sample orders)
    if (launch_per_phase(s) && (g.nrb == 1 || g.nrb == 2 || g.nrb == 4) && !in.tu.no_tap_major && !in.hp->order_per_candidate) {
        gr.taps = tap_major_units(all, STEP_NW / g.nrb, gr.descs);
        if (gr.taps.size() < 192 && !in.tu.force_tap_major) gr.taps.clear();      // too few workgroups to fill 256 CUs: per-segment path
    }
    if (gr.taps.empty()) gr.descs = std::move(all);
    std::stable_sort(gr.descs.begin(), gr.descs.end(), [](const SegDesc& x, const SegDesc& y) {
        return (int64_t)x.cc * x.rows_p > (int64_t)y.cc * y.rows_p; });
    if (s == Sched::SameGroup) gr.descs = same_group_units(gr.descs);
    return gr;
}

// What follows from the schedule once the units are known.  reads: the schedule, groups, lds_step.  writes: red_in_sweep, defer.
static void unit_dependent_flags(const PlanIn& in, Sched s, LayoutPlan& pl) {
    bool tap_units = false, double_pass_fits = true;
    for (const GroupPlan& gr : pl.groups) {
        tap_units = tap_units || !gr.taps.empty();
        for (const SegDesc& d : gr.descs)
            if (d.kind <= KIND_V && sweep_unit_lds_double(pl.g, d) > pl.lds_step) double_pass_fits = false;
    }
    // reduce-in-sweep: the chain is on the critical path, general chain, per-segment units only (tap-major workgroups serve several candidates)
    // (beyond ~28 candidates the co-scheduled chain is hidden anyway and the extra write-through traffic costs: 29.0 vs 26.7 cand/s at 32)
    // (not with chain_split: the reducing unit's drain + arrival + summing pass behind the LAST dy of the step ends the launch 3.5 us later,
    //  while the chain's four parts sum their own row blocks of the slabs at entry, every load in flight at once; measured, K = 1: 41.3 with
    //  the reduction in the sweep, 38.4 without, 43.0 with a hybrid — cells >= 1 in the sweep, cell 0 in the chain — profiles/r06_chain_split_r128.log)
    pl.red_in_sweep = (launch_per_phase(s) || s == Sched::SameGroup) && in.K < 28 && !pl.lean_chain && !in.tu.no_red_in_sweep &&
                      !(pl.chain_split && s == Sched::SameGroup) && !tap_units;
    // deferred stores (launches.hip.h, mark_deferred): the two-group launch-per-phase schedule with the general chain, no alphas (the
    // replayed step would need its gradient scale too) and per-segment feature units only, where every feature unit's double pass — a plain
    // unit's three staged tiles + the replayed step's rows and dy — fits the LDS the plan already asks for (lds_step is NOT raised for it)
    pl.defer = s == Sched::TwoGroups && !pl.lean_chain && !pl.g.alphas && !tap_units && double_pass_fits;
}

// Stage 8, the resident schedule's unit list and XCD role table.  reads: descs, nres_wg, res_nu.  writes: pdescs, need, role.
static void resident_units_and_roles(const PlanIn& in, LayoutPlan& pl) {
    const int K = in.K;
    std::vector<int> res_cand;      // candidate of every resident unit, in unit order
    // unit list of the resident schedule: the feature units (the resident lean chain updates OUT / HEAD itself)
    pl.need.assign(K, 0);
    for (const SegDesc& d : pl.descs)
        if (d.kind <= KIND_V) { pl.pdescs.push_back(d); res_cand.push_back(d.cand); pl.need[d.cand]++; }
    if (in.tu.no_xcd_placement) return;
    // XCD-aware placement (round 5): consecutive workgroups of a launch are dealt round-robin to the 8 XCDs (block b -> XCD b % 8,
    // MI355X_MICROARCH.md), each with its own L2.  A candidate's chain and the workgroups that hold its units exchange 60 KB of
    // slabs and 8 KB of dy per step: deal the roles so that they share an XCD wherever its 32 slots allow (greedy, candidate by
    // candidate; two-unit workgroups are grouped by their FIRST unit's candidate, and the chain of a candidate that only ever
    // comes second goes where most of its units are).  Placement only: the exchanges do not depend on it.
    // (NX: 8 XCDs on MI355X in SPX mode, block b -> XCD b % 8; MFAS_XCDS=n for another partition mode.  A wrong NX costs
    //  only the co-location.  prim / sec below mirror sweep_resident's unit mapping — unit u of workgroup w is unit w + u * nwg,
    //  persist.hip.h `const int ui = wg + u * nwg` — and must change with it.)
    const int nwg = pl.nres_wg, G = K + nwg, NX = in.tu.n_xcd > 0 ? std::min(in.tu.n_xcd, 64) : 8;
    std::vector<std::vector<int>> slots(NX);
    for (int b = G - 1; b >= 0; --b) slots[b % NX].push_back(b);       // (pop_back hands out the lowest block of an XCD first)
    std::vector<int32_t> role(G, -1);
    std::vector<int> chain_xcd(K, -1);
    std::vector<char> wg_done(nwg, 0);
    auto take = [&](int x, int item) { role[slots[x].back()] = item; slots[x].pop_back(); };
    auto roomiest = [&]() { int bx = 0; for (int x = 1; x < NX; ++x) if (slots[x].size() > slots[bx].size()) bx = x; return bx; };
    std::vector<int> prim(nwg), sec(nwg, -1);
    for (int w = 0; w < nwg; ++w) {
        prim[w] = res_cand[w];
        if (pl.res_nu == 2 && w + nwg < (int)res_cand.size()) sec[w] = res_cand[w + nwg];
    }
    for (int c = 0; c < K; ++c) {                   // candidates that come first in some workgroup: chain + those workgroups
        bool any = false;
        for (int w = 0; w < nwg; ++w) any = any || prim[w] == c;
        if (!any) continue;
        const int x = roomiest();
        if (!slots[x].empty()) { take(x, c); chain_xcd[c] = x; }
        for (int w = 0; w < nwg; ++w)
            if (prim[w] == c && !wg_done[w] && !slots[x].empty()) { take(x, K + w); wg_done[w] = 1; }
    }
    std::vector<int> wg_xcd(nwg, -1);
    for (int b = 0; b < G; ++b) if (role[b] >= K) wg_xcd[role[b] - K] = b % NX;
    for (int c = 0; c < K; ++c) {                   // chains not placed yet: where most of the candidate's units are
        if (chain_xcd[c] >= 0) continue;
        std::vector<int> votes(NX, 0);
        for (int w = 0; w < nwg; ++w) if ((prim[w] == c || sec[w] == c) && wg_xcd[w] >= 0) votes[wg_xcd[w]]++;
        int bx = -1;
        for (int x = 0; x < NX; ++x) if (!slots[x].empty() && (bx < 0 || votes[x] > votes[bx])) bx = x;
        if (bx >= 0) { take(bx, c); chain_xcd[c] = bx; }
    }
    for (int w = 0; w < nwg; ++w)                   // whatever did not fit its XCD
        if (!wg_done[w]) { const int x = roomiest(); take(x, K + w); wg_done[w] = 1; }
    bool ok = true;
    for (int b = 0; b < G; ++b) ok = ok && role[b] >= 0;
    if (ok) pl.role = role;
}

// Stage 9, the step buffers (same geometry for every candidate: sized for the largest).  A deferring plan's replayed step needs its dy to
// outlive the group's next chain: a second dy area at the END of every candidate's block (no other sub-offset depends on it); the host
// alternates Geo::sb_dy between the two in the per-launch arguments (train.hip.h).
// reads: Geo, defer.  writes: Geo::sb_*, sb_dy_alt, cands[k].step_off, step_total.
static void layout_step_buffers(int K, int max_slots, LayoutPlan& pl) {
    Geo& g = pl.g;
    const int64_t br = (int64_t)g.Bp * g.Rp;
    int64_t o = 0;
    g.sb_part = o; o += (int64_t)max_slots * br;
    g.sb_dy = o; o += MFAS_MAX_CELLS * br;
    g.sb_xo = o; o += MFAS_MAX_CELLS * br;
    g.sb_dlog = o; o += (int64_t)g.Bp * g.Cp;
    g.sb_sav = o; o += 3 * MFAS_MAX_CELLS * br;
    g.sb_yf = o; o += 2 * MFAS_MAX_CELLS * br;
    g.sb_gsc = o; o += 16;
    o = (o + 63) & ~63LL;
    if (pl.defer) { pl.sb_dy_alt = o; o = (o + MFAS_MAX_CELLS * br + 63) & ~63LL; }
    g.sb_size = o;
    for (int k = 0; k < K; ++k) pl.cands[k].step_off = (int64_t)k * g.sb_size;
    pl.step_total = (int64_t)K * g.sb_size;
}

// One plan for one kernel family (wide or batch-resident): the stages in order.
static int plan_layout_as(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells, const uint32_t* drop_seeds, int K, int chunk_cols,
                          int n_cus, bool allow_persist, const Tuning& tu, const bool wide, LayoutPlan& pl) {
    const PlanIn in{hp, confs, n_cells, drop_seeds, K, chunk_cols, n_cus, allow_persist, tu, wide};
    pl = LayoutPlan();
    pl.wide = wide;
    pl.g = make_geo(hp);
    const ChunkPlan lp = choose_chunk(in, pl.g);
    pl.chunk = lp.target;
    const int max_slots = layout_candidates(in, pl);
    lds_budgets(in, lp, pl);
    dev_pass_and_streaming(in, pl);
    const Sched s = choose_schedule(in, pl);
    if (int rc = schedule_flags(in, s, pl)) return rc;
    const int split = s == Sched::TwoGroups ? balanced_split(pl, K) : K;
    pl.groups.push_back(group_work_list(in, s, 0, split, pl));
    if (split < K) pl.groups.push_back(group_work_list(in, s, split, K - split, pl));
    unit_dependent_flags(in, s, pl);
    if (s == Sched::Resident) resident_units_and_roles(in, pl);
    layout_step_buffers(K, max_slots, pl);
    return MFAS_OK;
}

// The plan of a population: the batch-resident schedules wherever they hold the geometry — decided exactly as before the wide path
// existed, so every such population keeps its layout, kernels and bits — and the wide path exactly where they do not: B > 64, more
// classes than the batch-resident softmax takes, or a step that does not fit the LDS.
inline int plan_layout(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells, const uint32_t* drop_seeds, int K, int chunk_cols,
                       int n_cus, bool allow_persist, const Tuning& tu, LayoutPlan& pl) {
    if (!batch_resident_refuses(hp)) {
        if (int rc = plan_layout_as(hp, confs, n_cells, drop_seeds, K, chunk_cols, n_cus, allow_persist, tu, false, pl)) return rc;
        if (pl.fits_lds) return MFAS_OK;
    }
    return plan_layout_as(hp, confs, n_cells, drop_seeds, K, chunk_cols, n_cus, allow_persist, tu, true, pl);
}

// what the choice of a launch's build reads from the plan (builds.hip.h)
inline PlanFacts plan_facts(const LayoutPlan& pl) {
    PlanFacts f;
    f.wide = pl.wide; f.MB = pl.g.MB; f.lean_chain = pl.lean_chain; f.same_group = pl.same_group; f.chain_split = pl.chain_split;
    f.ngroups = (int)pl.groups.size(); f.nontemporal = pl.nontemporal; f.persist = pl.persist; f.res_wide = pl.res_wide; f.res_nu = pl.res_nu;
    f.mbe = pl.mbe; f.nrbw = pl.nrbw; f.nrb = pl.g.nrb;
    return f;
}
