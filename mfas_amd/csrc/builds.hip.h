// builds.hip.h — which kernel build a launch takes, as data (host only; plain C++17: no HIP include, no engine type but the shared
// sizes of records.hip.h).
// A build is named by a BuildKey: the kernel family and the template arguments of the instantiation.  The choice functions below turn
// the few plan facts a choice reads (PlanFacts, filled from the LayoutPlan by plan_facts in plan.hip.h) and the launch's own inputs
// into a key; the kernel tables of mfas_hip.hip turn a key into the function pointer.  plan_keys lists every key a population with
// these facts can ever launch: create sets the dynamic-LDS limit of exactly those builds.  The row lists at the end are the tables'
// rows: mfas_hip.hip expands them into instantiations, table_keys() into their keys, so both are one list.
// tests/test_builds_cpu.py compiles this header with g++ alone and judges it over the whole domain.
#pragma once
#include <string>
#include <vector>
#include "records.hip.h"

enum BuildFamily { F_STEP, F_STEP_SAME, F_SWEEP_WIDE, F_CHAIN, F_CHAIN_WIDE, F_PRESIDENT, F_EVAL, F_NONE };

struct BuildKey {
    int family = F_NONE, narg = 0, arg[5] = {0, 0, 0, 0, 0};
    bool operator==(const BuildKey& o) const {
        if (family != o.family || narg != o.narg) return false;
        for (int i = 0; i < 5; ++i) if (arg[i] != o.arg[i]) return false;
        return true;
    }
    // "k_step<1,1,4,0,1>", "k_chain_wide": the spelling of the launch record (describe() is its only user: no launch makes a string)
    std::string name() const {
        static const char* const families[] = {"k_step", "k_step_same", "k_sweep_wide", "k_chain", "k_chain_wide", "k_president", "k_eval", "none"};
        std::string s = families[family];
        for (int i = 0; i < narg; ++i) s += (i ? "," : "<") + std::to_string(arg[i]);
        if (narg) s += ">";
        return s;
    }
};

// what the choice reads from a LayoutPlan
struct PlanFacts {
    bool wide = false;                  // the wide path: k_chain_wide + k_sweep_wide
    int MB = 1;                         // batch tiles (1, 2, 4)
    bool lean_chain = false, same_group = false;
    int chain_split = 0;                // 0, or the CUs per candidate chain (4)
    int ngroups = 1;                    // candidate groups of the launch list (1, 2)
    bool nontemporal = false;
    bool persist = false, res_wide = false;     // the resident schedule; its units are wider than 512 columns
    int res_nu = 1;                     // resident units per workgroup
    int mbe = 4, nrbw = 1, nrb = 1;     // dev pass: batch tiles per workgroup, row blocks per wave; the geometry's row blocks
};

inline BuildKey step_key_of(int MB, bool nt, int wpe, bool lean, int ns) { return {F_STEP, 5, {MB, nt, wpe, lean, ns}}; }
inline BuildKey same_key_of(int MB, bool nt, int ns) { return {F_STEP_SAME, 3, {MB, nt, ns, 0, 0}}; }
inline BuildKey sweep_wide_key_of(bool nt) { return {F_SWEEP_WIDE, 1, {nt, 0, 0, 0, 0}}; }
inline BuildKey chain_key_of(int MB, bool lean) { return {F_CHAIN, 2, {MB, lean, 0, 0, 0}}; }
inline BuildKey chain_wide_key_of() { return {F_CHAIN_WIDE, 0, {0, 0, 0, 0, 0}}; }
inline BuildKey president_key_of(int MB, int ntr, bool x16, int nu, int plain) { return {F_PRESIDENT, 5, {MB, ntr, x16, nu, plain}}; }
inline BuildKey eval_key_of(int mbe, int nrbw, int msp, bool xb, bool b3) { return {F_EVAL, 5, {mbe, nrbw, msp, xb, b3}}; }

// The build that carries a launch with a sweep in it.  nch: candidates of its chain (0: none); same: chain(g, t) and sweep(g, t) in ONE
// launch behind per-cell flags; over_occ: the state bytes of the sweep's group exceed the plan's occ_bytes.  With chain_split the chain
// blocks of a launch that has a chain are chain_split parts.
inline BuildKey step_key(const PlanFacts& f, unsigned nch, bool same, bool over_occ) {
    const bool split = f.chain_split && nch > 0;
    if (f.wide) return sweep_wide_key_of(f.nontemporal);      // launch per phase only: the sweep of the one group, after its chain's launch
    if (same) return same_key_of(f.MB, f.nontemporal, split ? f.chain_split : 1);
    if (split) return step_key_of(f.MB, f.nontemporal, 4, false, f.chain_split);
    // MB == 2: the two-workgroups-per-CU build unless a co-scheduled chain would bound the launch (see SweepU)
    // (lean chain: the 128-VGPR build spills 8 registers of the element-parallel chain to scratch and is still the faster
    //  one — R=16, B=20, 50 / 128 / 512 candidates: 47.2 / 99.2 / 418 us per step against 50.5 / 117.4 / 447 for the 2-workgroup build)
    const bool occ = nch == 0 || over_occ;
    return step_key_of(f.MB, f.nontemporal, f.MB == 1 || (f.MB == 2 && (occ || f.lean_chain)) ? 4 : 2, f.lean_chain, 1);
}

// a launch without a sweep: the latency-tuned standalone chain (wide populations: theirs)
inline BuildKey chain_key(const PlanFacts& f) { return f.wide ? chain_wide_key_of() : chain_key_of(f.MB, f.lean_chain); }

// The resident loop's chain: the search default — no BatchNorm, no alphas, single-task softmax CE — runs the chain compiled for exactly
// that (1), `--batchnorm` alone the chain compiled for exactly THAT (2), everything else the general one (0)
inline int president_plain(bool alphas, bool multitask, int loss_mode, bool bn, bool no_plain_chain) {
    const bool simple = !alphas && !multitask && loss_mode == 0 && !no_plain_chain;
    return simple ? (bn ? 2 : 1) : 0;
}

// one build per unit form: f32 staging (one or two units per workgroup), 16-bit staging (the same, or one WIDE unit of up to 1024
// columns).  x16: the train table is not f32
inline BuildKey president_key(const PlanFacts& f, bool x16, int plain) {
    if (x16 && f.res_wide) return president_key_of(f.MB, PERSIST_NTR16, true, 1, plain);
    return president_key_of(f.MB, PERSIST_NTR, x16, f.res_nu != 2 ? 1 : 2, plain);
}

// The dev pass.  One or two row blocks (R <= 32): the m-blocks of a row tile are split over the four waves, and the rows of a bf16 table
// stay 16-bit in LDS; two row blocks per wave (R = 72 .. 128) over a bf16 table: exact bf16 x 3 feature products on the bf16 matrix
// pipe; else the plain build.  no_*: the MFAS_EVAL_NO_* switches
inline BuildKey eval_key(const PlanFacts& f, int dtype, bool no_x16, bool no_msplit, bool no_b3) {
    const bool bf16 = dtype == MFAS_DT_BF16;
    if (f.nrbw == 1 && (f.nrb == 1 || f.nrb == 2) && !no_msplit) return eval_key_of(f.mbe, 1, f.nrb, bf16 && !no_x16, false);
    if (bf16 && f.nrbw == 2 && !no_b3) return eval_key_of(f.mbe, 2, 0, false, true);
    return eval_key_of(f.mbe, f.nrbw, 0, false, false);
}

// One batch through one candidate (forward_train / backward): the cached sweep with no chain next to it at the occupancy its batch
// tiles were tuned for, and the plan's standalone chain
inline BuildKey single_batch_step_key(const PlanFacts& f) {
    return f.wide ? sweep_wide_key_of(false) : step_key_of(f.MB, false, f.MB == 1 ? 4 : 2, false, 1);
}
inline BuildKey single_batch_chain_key(const PlanFacts& f) { return chain_key(f); }

// Every build a population with these facts can launch, each once: its train calls (the resident launch over both staging widths and
// the three chains, or the launch list of launches.hip.h: a prologue without a chain, then the same-group launch, or chain and sweep
// in turn, or two groups' sweep + chain under either occupancy verdict), the dev pass over the three table dtypes and every switch
// setting, and single_batch.
inline std::vector<BuildKey> plan_keys(const PlanFacts& f) {
    std::vector<BuildKey> out;
    auto add = [&out](const BuildKey& k) {
        for (const BuildKey& o : out) if (o == k) return;
        out.push_back(k);
    };
    if (f.persist) {
        for (int x16 = 0; x16 < 2; ++x16)
            for (int plain = 0; plain < 3; ++plain) add(president_key(f, x16 != 0, plain));
    } else {
        add(step_key(f, 0, false, false));
        if (f.same_group) add(step_key(f, 1, true, false));
        else if (f.ngroups == 1) add(chain_key(f));
        else {
            add(chain_key(f));
            for (int over = 0; over < 2; ++over) add(step_key(f, 1, false, over != 0));
        }
    }
    for (int dtype = 0; dtype < 3; ++dtype)
        for (int sw = 0; sw < 8; ++sw) add(eval_key(f, dtype, sw & 1, sw & 2, sw & 4));
    add(single_batch_step_key(f));
    add(single_batch_chain_key(f));
    return out;
}

// ------------------------------------------------------------------------------------------------
// The rows of the kernel tables: every instantiation that is built, as its template arguments.  ROW is the user's: mfas_hip.hip's makes
// the Build (pointer and key, both from one *_of template), table_keys()'s the key alone.
// ------------------------------------------------------------------------------------------------
// k_step<MB, NT, WPE, LEAN, NS>, k_step_same<MB, NT, NS>, k_sweep_wide<NT>: each cached and nontemporal
#define BUILDS_STEP_NT(ROW, M, W, F, S) ROW(M, 0, W, F, S) ROW(M, 1, W, F, S)
#define BUILDS_STEP_ROWS(ROW) BUILDS_STEP_NT(ROW, 1, 4, 0, 4) BUILDS_STEP_NT(ROW, 1, 4, 0, 1) BUILDS_STEP_NT(ROW, 2, 2, 0, 1) BUILDS_STEP_NT(ROW, 2, 4, 0, 1) \
    BUILDS_STEP_NT(ROW, 4, 2, 0, 1) BUILDS_STEP_NT(ROW, 1, 4, 1, 1) BUILDS_STEP_NT(ROW, 2, 4, 1, 1)
#define BUILDS_SAME_NT(ROW, M, S) ROW(M, 0, S) ROW(M, 1, S)
#define BUILDS_SAME_ROWS(ROW) BUILDS_SAME_NT(ROW, 1, 1) BUILDS_SAME_NT(ROW, 2, 1) BUILDS_SAME_NT(ROW, 1, 4)
#define BUILDS_SWEEP_WIDE_ROWS(ROW) ROW(0) ROW(1)
// k_chain<MB, LEAN>
#define BUILDS_CHAIN_ROWS(ROW) ROW(1, 0) ROW(2, 0) ROW(4, 0) ROW(1, 1) ROW(2, 1)
// k_president<MB, NTR, X16, NU, PLAIN>: every (MB, PLAIN) in the five unit forms
#define BUILDS_PRESIDENT_FORMS(ROW, M, P) ROW(M, 4, 0, 1, P) ROW(M, 4, 0, 2, P) ROW(M, 4, 1, 1, P) ROW(M, 4, 1, 2, P) ROW(M, 8, 1, 1, P)
#define BUILDS_PRESIDENT_ROWS(ROW) BUILDS_PRESIDENT_FORMS(ROW, 1, 0) BUILDS_PRESIDENT_FORMS(ROW, 2, 0) BUILDS_PRESIDENT_FORMS(ROW, 1, 1) \
    BUILDS_PRESIDENT_FORMS(ROW, 2, 1) BUILDS_PRESIDENT_FORMS(ROW, 1, 2) BUILDS_PRESIDENT_FORMS(ROW, 2, 2)
// k_eval<MBE, NRBW, MSP, XB, B3>: the m-blocks split over the waves (f32 and 16-bit rows), bf16 x 3, plain.  Only what an accepted
// geometry can launch is built.  The tile is 64 rows (MBE = 4) unless (64 * (max(136, Cp + 4) + Rp + 8)) * 4 exceeds 80 KiB, i.e.
// Rp + max(136, Cp + 4) > 312, and 32 rows (MBE = 2) unless Rp + max(136, Cp + 4) > 632; C <= 256, so max(136, Cp + 4) <= 260.  So:
//   the split builds (one or two row blocks, Rp <= 32): 32 + 260 = 292 is not over 312 — the tile is always 64 rows, MBE = 4 only;
//   MBE = 1 (a 16-row tile) needs Rp + 260 > 632, Rp > 372 — only with eight row blocks per wave: (1, 8) and no other MBE = 1 row;
//   (4, 8): eight row blocks per wave is Rp >= 272, and 272 + 136 = 408 is over 312 — the tile is never 64 rows.
// (eval_build of a key that is not built gives nullptr: launch_eval answers hipErrorInvalidValue)
#define BUILDS_EVAL_SPLIT(ROW, M, S) ROW(M, 1, S, 0, 0) ROW(M, 1, S, 1, 0)
#define BUILDS_EVAL_ROWS(ROW) BUILDS_EVAL_SPLIT(ROW, 4, 1) BUILDS_EVAL_SPLIT(ROW, 4, 2) ROW(4, 2, 0, 0, 1) ROW(2, 2, 0, 0, 1) \
    ROW(4, 1, 0, 0, 0) ROW(4, 2, 0, 0, 0) ROW(4, 4, 0, 0, 0) ROW(2, 1, 0, 0, 0) ROW(2, 2, 0, 0, 0) ROW(2, 4, 0, 0, 0) ROW(2, 8, 0, 0, 0) \
    ROW(1, 8, 0, 0, 0)

inline std::vector<BuildKey> table_keys() {
    std::vector<BuildKey> out;
#define STEP_(...) out.push_back(step_key_of(__VA_ARGS__));
#define SAME_(...) out.push_back(same_key_of(__VA_ARGS__));
#define WIDE_(...) out.push_back(sweep_wide_key_of(__VA_ARGS__));
#define CHAIN_(...) out.push_back(chain_key_of(__VA_ARGS__));
#define PRES_(...) out.push_back(president_key_of(__VA_ARGS__));
#define EVAL_(...) out.push_back(eval_key_of(__VA_ARGS__));
    BUILDS_STEP_ROWS(STEP_) BUILDS_SAME_ROWS(SAME_) BUILDS_SWEEP_WIDE_ROWS(WIDE_) BUILDS_CHAIN_ROWS(CHAIN_)
    out.push_back(chain_wide_key_of());
    BUILDS_PRESIDENT_ROWS(PRES_) BUILDS_EVAL_ROWS(EVAL_)
#undef STEP_
#undef SAME_
#undef WIDE_
#undef CHAIN_
#undef PRES_
#undef EVAL_
    return out;
}
