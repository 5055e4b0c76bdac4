// mfas_hip.hip — MI355X (gfx950 / CDNA4) inner candidate-training engine for MFAS.
//
// What it replaces (reference = jperezrua/mfas, pure PyTorch):
//   train_sampled_models                models/search/ntu_searchable.py:23-102
//   train_ntu_track_acc                 models/search/train_searchable/ntu.py:14-89
//   Searchable_Skeleton_Image_Net.forward (+ autograd + torch.optim.Adam)   ntu_searchable.py:206-286
//
// Design: the whole population trains in lockstep.  Per train step three kernels run for
// ALL candidates at once:
//   k_chain  (1 workgroup / candidate): the serial R-wide part — reduce feature partial sums, cell chain
//            (prev-out GEMM on f32 MFMA, activation, BN batch stats, dropout), head, CE loss, and the
//            backward chain producing dy_i for every cell;
//   k_sweep  (1 workgroup / (candidate, weight chunk)): the HBM-bound part — for every weight tile:
//            dW = x_t^T dy (f32 MFMA) -> Adam(+L2) update of W/m/v in registers -> store -> immediately
//            use the new W for the NEXT step's forward partial sums (f32 MFMA).  24 B/param/step = the
//            algorithmic minimum with state in HBM.
// Source layout (ONE translation unit; this file includes the rest): records.hip.h (what host and device share, plain C++: the records
// the planner fills and the kernels read — SegDesc, TapDesc, CandDev, DevStats, Geo — the sizes both agree on and the LDS formulas both
// use), hosterr.hip.h (fail() and the last error text), common.hip.h (device helpers, LDS staging, HIPCHK), sweep.hip.h
// (tile_run, sweep_body, sweep_tap_body), chain.hip.h (chain_body, chain_lean, softmax / BCE rows), wide.hip.h (k_chain_wide / k_sweep_wide:
// the batch walked in tiles), eval.hip.h (k_eval), pack.hip.h (k_pack, k_vec, k_pool, k_stream_probe), surrogate.hip.h (the search
// controller's LSTM surrogate: k_surr_grad / k_surr_adam / k_surr_forward and their stateless C ABI); host only: devmem.hip.h (DevBuf: the
// one owner of device memory — a population's buffers and every call's scratch free themselves; nothing else allocates or frees), plan.hip.h (the switches,
// validate_inputs, plan_layout: layout, schedule, LDS budgets and work lists decided before anything is allocated — the fourth header,
// after devmem / builds / launches, that is plain C++17 and that g++ compiles alone: tests/plan_header.py), launches.hip.h (the
// launches of an epoch as data), builds.hip.h (which build a launch takes, as data: the choice functions, the builds a plan can launch, the
// tables' row lists), state.hip.h (state in and out, the candidate carry, move, the fallback), train.hip.h (the train call); vote.hip.h (k_vote and the host side of
// mfas_population_evaluate: members through k_eval, then the vote), tally.hip.h (k_tally: the per-class tallies of
// mfas_population_evaluate_report).  Here:
// k_step / k_chain, the kernel tables (key -> instantiation: the only place one is named), create / destroy, the C ABI.
// Dev evaluation is row-parallel (k_eval).  Weights live in a 16x16 tile-major layout that is exactly the
// MFMA 16x16x4 f32 operand layout, so every W/m/v access is one coalesced 16 B/lane load.
//
// MFMA used: v_mfma_f32_16x16x4_f32 (exact f32 fma chain).  Layout (lane l):
//   A[i = l&15][k = l>>4],  B[k = l>>4][j = l&15],  D[i = 4*(l>>4)+reg][j = l&15].
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
// No implicit FMA contraction anywhere in this translation unit (see __graft_entry__.build): every schedule (k_chain / k_step /
// k_president instantiations) must round identically.  MFMA instructions are unaffected.
#pragma clang fp contract(off)
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <cmath>
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include <thread>
#include <chrono>
#include <dlfcn.h>

#include "mfas_hip.h"

#include "common.hip.h"
#include "sweep.hip.h"
#include "chain.hip.h"

// ------------------------------------------------------------------------------------------------
// k_step — ONE launch per half-step: blocks [0, nchain) run the chain of one candidate group while the other
// blocks run the sweep of the OTHER group (candidates are independent).  The latency-bound chain hides under
// the HBM-bound sweep; kernel boundaries carry every dependency (chain(t) -> sweep(t) -> chain(t+1) of a group).
// ------------------------------------------------------------------------------------------------
struct StepArgs {
    SweepArgs sa;
    ChainArgs ca;
    int32_t nchain, _pad;
    GatherArgs ga;          // nblocks gather workgroups (one per chain candidate) right after the chain blocks
};

// NS > 1 (its own instantiation: the headline k_step<1, true, 4, false> carries none of it): the chain blocks are chain_split parts,
// block b = part * (nchain / NS) + candidate (k_step_same below).
template <int MB, bool NT, int WPE, bool LEAN, int NS = 1>
__global__ void __launch_bounds__(STEP_THREADS, WPE) k_step(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int bid = (int)blockIdx.x;
    if (bid < a.nchain) {
        if constexpr (NS > 1) {
            const int Kp = a.nchain / NS, part = bid / Kp, c = bid - part * Kp;
            if (c < a.ca.ncand) chain_split<NS>(a.ca, chain_step_of(a.ca), c, part, lds);
        } else
        if constexpr (LEAN) { chain_lean<MB, 0, (WPE >= 4 ? 8 : 16)>(a.ca, chain_step_of(a.ca), bid, lds, lean_pre<MB>(a.ca, bid)); chain_lean_tail<MB, 0>(a.ca, chain_step_of(a.ca), bid, lds); }
        else chain_body<MB, false>(a.ca, chain_step_of(a.ca), bid, lds);
    }
    else if (bid < a.nchain + a.ga.nblocks) gather_body(a.ga, a.ga.cands[bid - a.nchain], a.sa.g, a.sa.tab, a.sa.order, (int)threadIdx.x);
    else if (bid < a.nchain + a.ga.nblocks + a.sa.ntap) sweep_tap_body<MB, NT, SweepU<MB, WPE>::v>(a.sa, bid - a.nchain - a.ga.nblocks, lds);
    else sweep_body<MB, NT, SweepU<MB, WPE>::v, false, !LEAN>(a.sa, sweep_step_of(a.sa), bid - a.nchain - a.ga.nblocks - a.sa.ntap, lds);      // (a lean-chain plan defers no stores)
}

// Same-group fused launch (small populations with the general chain, R >= 128): chain blocks AND sweep blocks of the SAME
// candidates in one launch; a sweep unit waits for its cell's dy (per-cell flags published by the chain as the backward pass
// reaches the cell) instead of for a kernel boundary, so the sweeps of cells L-1 .. 1 overlap the rest of the backward pass.
// The work list is ordered last cell first; chain blocks have the lowest block indices (dispatched first).
// NS > 1 (MB = 1, eight row blocks): every candidate's chain runs on NS workgroups (chain_split): chain block b = part * Kp + candidate
// with Kp = the candidate count rounded up to 8 — block b lands on XCD b % 8, so a candidate's parts share an XCD and its L2.
template <int MB, bool NT, int NS = 1>
__global__ void __launch_bounds__(STEP_THREADS, 4) k_step_same(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int bid = (int)blockIdx.x;
    if (bid < a.nchain) {
        if constexpr (NS > 1) {
            const int Kp = a.nchain / NS, part = bid / Kp, c = bid - part * Kp;
            if (c < a.ca.ncand) chain_split<NS>(a.ca, chain_step_of(a.ca), c, part, lds);
        } else chain_body<MB, false, true>(a.ca, chain_step_of(a.ca), bid, lds);
    } else sweep_body<MB, NT, SweepU<MB, 4>::v, true>(a.sa, sweep_step_of(a.sa), bid - a.nchain, lds);
}

// Standalone chain launch (small populations: chain and sweep run back to back, so the chain's latency is on the
// critical path): full register budget, next-product weight tiles prefetched into registers.
template <int MB, bool LEAN>
__global__ void __launch_bounds__(STEP_THREADS, 2) k_chain(const ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if constexpr (LEAN) { chain_lean<MB>(a, chain_step_of(a), (int)blockIdx.x, lds, lean_pre<MB>(a, (int)blockIdx.x)); chain_lean_tail<MB, 0>(a, chain_step_of(a), (int)blockIdx.x, lds); }
    else chain_body<MB, true>(a, chain_step_of(a), (int)blockIdx.x, lds);
}

#include "wide.hip.h"
#include "persist.hip.h"
#include "eval.hip.h"
#include "pack.hip.h"
#include "surrogate.hip.h"

#include "devmem.hip.h"
#include "builds.hip.h"
#include "plan.hip.h"

// ================================================================================================
// Host side: C ABI
// ================================================================================================
// The launch record: the distinct kernel builds the last train call of a population launched, each with its template arguments and a
// launch count (mfas_population_launch_record).  An entry is made where the launch is made, from the Build the launch takes its function
// pointer from (the kernel tables below), so the record cannot name another instantiation than the one that ran.
struct LaunchRecord {
    struct Entry { BuildKey key; const void* fn; int64_t n; };
    std::vector<Entry> entries;     // a handful: one per build, found by its function pointer
    void clear() { entries.clear(); }
    void count(const BuildKey& key, const void* fn) {
        for (Entry& e : entries) if (e.fn == fn) { ++e.n; return; }
        entries.push_back(Entry{key, fn, 1});
    }
    // "k_step<1,1,4,0,1>:7 k_chain<1,0>:8 ...", sorted by name
    std::string describe() const {
        std::vector<std::string> items;
        for (const Entry& e : entries) items.push_back(e.key.name() + ":" + std::to_string(e.n));
        std::sort(items.begin(), items.end());
        std::string out;
        for (const std::string& s : items) out += (out.empty() ? "" : " ") + s;
        return out;
    }
};

// The profiling event pairs of a population.  Move-only, and a move EXCHANGES: whichever record, or temporary of a swap, ends up
// holding an event destroys it, once.
struct EventPairs {
    std::vector<hipEvent_t> v;
    EventPairs() = default;
    EventPairs(EventPairs&& o) noexcept { v.swap(o.v); }
    EventPairs& operator=(EventPairs&& o) noexcept {
        v.swap(o.v);
        return *this;
    }
    ~EventPairs() {
        for (hipEvent_t e : v) hipEventDestroy(e);
    }
    // one more pair; false, and nothing added, when an event cannot be created
    bool add_pair() {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) != hipSuccess) return false;
        if (hipEventCreate(&e1) != hipSuccess) {
            hipEventDestroy(e0);
            return false;
        }
        v.push_back(e0);
        v.push_back(e1);
        return true;
    }
};

struct mfas_population {
    mfas_hyper hp;
    Tuning tune;                    // the environment switches as they stood when the population was created
    int K = 0, device = 0, n_cus = 0;
    int chunk_cols_req = 0;         // chunk_cols the caller asked for at creation (the fallback layout is built with the same request)
    hipStream_t stream = nullptr;
    LayoutPlan plan;                // layout, schedule, LDS budgets, work lists (plan.hip.h): decided before anything was allocated, never changed
    // device memory: every buffer owns itself (devmem.hip.h) — nothing here is freed by hand, a grow-only buffer's capacity is its size()
    DevBuf<float> plane, wt, stepbuf;
    DevBuf<float> best;             // snapshot_best: copy of plane 0 (keep_best, state.hip.h)
    DevBuf<CandDev> d_cands;
    DevBuf<SegDesc> d_descs;
    struct GroupDev { DevBuf<SegDesc> d_descs; DevBuf<TapDesc> d_taps; };
    std::vector<GroupDev> groups;   // device copies of plan.groups[i].descs / .taps
    DevBuf<DevStats> d_stats;       // [K][epochs] of the largest schedule so far (grow-only)
    DevBuf<int32_t> d_status;
    DevBuf<uint32_t> d_seeds;
    DevBuf<long long> d_corr;
    DevBuf<float> d_posw;           // loss_mode 1: per-class positive weights (default 1)
    // profiling of the dominant kernel
    bool profiling = false;
    int prof_every = 16;            // HIP events bracket every prof_every-th sweep launch (event records are not free)
    EventPairs ev;
    int64_t prof_launches = 0;
    double prof_ms = 0.0, bytes_per_launch = 0.0, prof_bytes = 0.0;
    LaunchRecord launched;          // the builds the last train call launched (cleared when a call has passed its checks)
    double best_threshold = 0.0;   // snapshot_best: a dev metric must exceed this to count (init_f1, mmimdb.py:18; 0 for NTU)
    // Progress record (mfas_population_train_from): what train_ntu_track_acc keeps on its stack for one call (best_acc,
    // train_searchable/ntu.py:18,82-83) and where in its schedule every candidate stands, kept between calls.  Per candidate: a moved
    // candidate (mfas_population_move) brings its own.
    struct Progress {
        std::vector<int64_t> done, nb;      // epochs of the schedule that are complete; that schedule's batches per epoch
        std::vector<double> best_metric;    // best dev metric so far (starts at best_threshold)
        std::vector<int32_t> keeps_best;    // the schedule runs with snapshot_best: plane `best` holds this candidate's best epoch
        void reset(int K, double threshold) { done.assign(K, 0); nb.assign(K, 0); best_metric.assign(K, threshold); keeps_best.assign(K, 0); }
    } prog;
    DevBuf<float> d_move;           // mfas_population_move: one candidate in flat state_dict order (grow-only scratch of the destination)
    DevBuf<uint32_t> d_red_cnt;     // reduce-in-sweep arrival counters [K][4] (small populations, general chain)
    DevBuf<char> d_gather;          // gathered rows [K][2 parities][taps][Bp][width] (two-group schedule, per-candidate orders; sweep.hip.h; grow-only)
    DevBuf<uint32_t> d_cellflag;    // [K][CELLFLAG_STRIDE]
    DevBuf<float> d_xch;            // chain_split's exchange area [K][XCH_CAND_FLOATS]
    // persistent step loop (persist.hip.h)
    DevBuf<SegDesc> d_pdescs;       // plan.pdescs
    int fell_back = 0;              // the resident schedule was given up for launch-per-phase inside a train() call (roll call never complete)
    DevBuf<uint32_t> d_sync;        // [K] flags | [K] counters | abort word (zeroed before every launch)
    DevBuf<int32_t> d_need, d_role; // plan.need, plan.role
    DevBuf<float> d_scal;           // device copy of the step scalars (grow-only)
    DevBuf<unsigned long long> d_trace;
    DevBuf<char> d_vote;            // mfas_population_evaluate's arena (grow-only; vote.hip.h): nothing a train call reads

    mfas_population() = default;
    mfas_population(mfas_population&&) = default;               // (persist_fallback swaps two records; the temporary of that swap
    mfas_population& operator=(mfas_population&&) = default;    //  waits for the — drained — stream too when it leaves)
    // what the stream still runs may read the buffers: wait for it, then the members free themselves
    ~mfas_population() {
        hipSetDevice(device);
        hipStreamSynchronize(stream);
    }
};

// roctx ranges around a train() call and each of its epochs (rocprofv3 --marker-trace shows them next to the kernels).  The
// marker library is looked up at run time: no link-time dependency, plain no-ops where it is absent (or MFAS_NO_ROCTX is set).
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        if (getenv("MFAS_NO_ROCTX")) return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_LOCAL);
        if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_LAZY | RTLD_LOCAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
Roctx& roctx() { static Roctx r; return r; }
struct RangeGuard {      // pops on every return path
    bool on;
    explicit RangeGuard(const std::string& name) : on(roctx().push != nullptr) { if (on) roctx().push(name.c_str()); }
    ~RangeGuard() { if (on) roctx().pop(); }
};
}
extern "C" int mfas_range_push(const char* name) { if (name && roctx().push) roctx().push(name); return MFAS_OK; }
extern "C" int mfas_range_pop(void) { if (roctx().pop) roctx().pop(); return MFAS_OK; }

extern "C" const char* mfas_last_error(void) { return g_err.c_str(); }
extern "C" int mfas_version(void) { return 200; }
#ifndef MFAS_SRC_DIGEST
#define MFAS_SRC_DIGEST "unknown"
#endif
// sha256 (first 16 hex digits) of the sources this library was built from, baked in by __graft_entry__.build()
extern "C" const char* mfas_source_digest(void) { return "mfas-src-digest:" MFAS_SRC_DIGEST; }

template <typename KT>
static hipError_t set_lds(KT kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// ------------------------------------------------------------------------------------------------
// Kernel tables: every instantiation of a family is named HERE and nowhere else, one row per entry of the family's row list in
// builds.hip.h.  A row is a Build: the instantiation's pointer AND its key, both written by ONE function template per family (*_of below)
// from the same template parameters — the name the launch record keeps is the name of the instantiation that is launched.  A launch
// chooses a key (builds.hip.h) and looks its row up; create sets the dynamic-LDS limit of the rows of plan_keys (set_lds_all), the keys a
// population with that plan can choose.  A key that is not built gives nullptr.
// ------------------------------------------------------------------------------------------------
typedef void (*StepKernel)(const StepArgs);
typedef void (*ChainKernel)(const ChainArgs);
typedef void (*PresidentKernel)(const PersistArgs, const int);
typedef hipError_t (*EvalLaunch)(mfas_population*, const EvalArgs&, int, hipStream_t);      // (launch_eval_t: the dev pass sets its LDS limit per launch)

template <typename KT>
struct Build { BuildKey key; KT fn = nullptr; };
typedef Build<StepKernel> StepBuild;
typedef Build<ChainKernel> ChainBuild;
typedef Build<PresidentKernel> PresidentBuild;
typedef Build<EvalLaunch> EvalBuild;

template <int MBE, int NRBW, int MSP, bool XB, bool B3>
static hipError_t launch_eval_t(mfas_population* p, const EvalArgs& a, int ncand, hipStream_t st);

template <int MB, bool NT, int WPE, bool LEAN, int NS> static StepBuild step_of() { return {step_key_of(MB, NT, WPE, LEAN, NS), k_step<MB, NT, WPE, LEAN, NS>}; }
template <int MB, bool NT, int NS> static StepBuild same_of() { return {same_key_of(MB, NT, NS), k_step_same<MB, NT, NS>}; }
template <bool NT> static StepBuild wide_sweep_of() { return {sweep_wide_key_of(NT), k_sweep_wide<NT>}; }
template <int MB, bool LEAN> static ChainBuild chain_of() { return {chain_key_of(MB, LEAN), k_chain<MB, LEAN>}; }
template <int MB, int NTR, bool X16, int NU, int PLAIN> static PresidentBuild president_of() { return {president_key_of(MB, NTR, X16, NU, PLAIN), k_president<MB, NTR, X16, NU, PLAIN>}; }
template <int MBE, int NRBW, int MSP, bool XB, bool B3> static EvalBuild eval_of() { return {eval_key_of(MBE, NRBW, MSP, XB, B3), launch_eval_t<MBE, NRBW, MSP, XB, B3>}; }

template <typename KT, size_t N>
static Build<KT> find_build(const Build<KT> (&rows)[N], const BuildKey& key) {
    for (const Build<KT>& r : rows) if (r.key == key) return r;
    return Build<KT>();
}

// the launches with a sweep in them: k_step, k_step_same, k_sweep_wide (wide.hip.h)
static StepBuild step_build(const BuildKey& key) {
#define STEP_(...) step_of<__VA_ARGS__>(),
#define SAME_(...) same_of<__VA_ARGS__>(),
#define WIDE_(...) wide_sweep_of<__VA_ARGS__>(),
    static const StepBuild rows[] = {BUILDS_SAME_ROWS(SAME_) BUILDS_STEP_ROWS(STEP_) BUILDS_SWEEP_WIDE_ROWS(WIDE_)};
#undef STEP_
#undef SAME_
#undef WIDE_
    return find_build(rows, key);
}

// the standalone chain, and the wide path's
static ChainBuild chain_build(const BuildKey& key) {
#define CHAIN_(...) chain_of<__VA_ARGS__>(),
    static const ChainBuild rows[] = {BUILDS_CHAIN_ROWS(CHAIN_) {chain_wide_key_of(), k_chain_wide}};
#undef CHAIN_
    return find_build(rows, key);
}

static PresidentBuild president_build(const BuildKey& key) {
#define PRES_(...) president_of<__VA_ARGS__>(),
    static const PresidentBuild rows[] = {BUILDS_PRESIDENT_ROWS(PRES_)};
#undef PRES_
    return find_build(rows, key);
}

static EvalBuild eval_build(const BuildKey& key) {
#define EVAL_(...) eval_of<__VA_ARGS__>(),
    static const EvalBuild rows[] = {BUILDS_EVAL_ROWS(EVAL_)};
#undef EVAL_
    return find_build(rows, key);
}

template <typename... A>
static void launch(void (*kernel)(A...), unsigned grid, size_t lds, hipStream_t stream, A... args) {
    void* argv[] = {const_cast<void*>(static_cast<const void*>(&args))...};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3(grid), dim3(STEP_THREADS), argv, lds, stream);    // (errors: hipGetLastError)
}

// a launch of a train call: counted in the population's launch record, then made
template <typename... A>
static void launch_build(mfas_population* p, const Build<void (*)(A...)>& b, unsigned grid, size_t lds, hipStream_t stream, A... args) {
    if (b.fn) p->launched.count(b.key, reinterpret_cast<const void*>(b.fn));
    launch(b.fn, grid, lds, stream, args...);
}

// the dynamic-LDS limit of every build a population with this plan can launch (the dev pass sets its own per launch: launch_eval_t)
static hipError_t set_lds_all(const LayoutPlan& pl) {
    hipError_t e = hipSuccess;
    auto set = [&e](auto kernel, size_t bytes) { if (kernel && e == hipSuccess) e = set_lds(kernel, bytes); };
    for (const BuildKey& key : plan_keys(plan_facts(pl)))
        switch (key.family) {
            case F_STEP: set(step_build(key).fn, key.arg[4] > 1 ? pl.lds_split : pl.lds_step); break;
            case F_STEP_SAME: set(step_build(key).fn, key.arg[2] > 1 ? pl.lds_split : pl.lds_step); break;
            case F_SWEEP_WIDE: set(step_build(key).fn, pl.lds_step); break;
            case F_CHAIN: case F_CHAIN_WIDE: set(chain_build(key).fn, pl.lds_chain); break;
            case F_PRESIDENT: set(president_build(key).fn, pl.lds_president); break;
            default: break;
        }
    return e;
}

static int device_cus(int device) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
    return ncu;
}

// validate -> plan (pure: plan.hip.h) -> allocate / upload / set the LDS limits from the plan; a failure on the way just leaves: the record owns its buffers
static int create_impl(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells,
                       const uint32_t* drop_seeds, int32_t K, int32_t device, void* hip_stream,
                       int32_t chunk_cols, mfas_population** out, const bool allow_persist, const Tuning* inherit = nullptr) {
    if (!out) return fail(MFAS_EINVAL, "null argument or K <= 0");
    if (int vrc = validate_inputs(hp, confs, n_cells, K)) return vrc;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(MFAS_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    std::unique_ptr<mfas_population> p(new (std::nothrow) mfas_population());
    if (!p) return fail(MFAS_ENOMEM, "host alloc");
    p->hp = *hp;
    p->tune = inherit ? *inherit : tuning_from_env();      // (persist_fallback rebuilds a population under the switches it was created with)
    p->K = K;
    p->device = device;
    p->stream = reinterpret_cast<hipStream_t>(hip_stream);
    p->chunk_cols_req = chunk_cols;
    p->n_cus = device_cus(device);
    p->prog.reset(K, 0.0);
    if (int prc = plan_layout(hp, confs, n_cells, drop_seeds, K, chunk_cols, p->n_cus, allow_persist, p->tune, p->plan)) return prc;
    const LayoutPlan& pl = p->plan;
    if (!pl.fits_lds) return fail(MFAS_EINVAL, "geometry does not fit the 160 KiB LDS (R / batchsize too large)");
    p->bytes_per_launch = pl.bytes_per_launch;

#define CREATE_CHK(x)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? MFAS_ENOMEM : MFAS_EHIP,                       \
                        std::string(#x) + ": " + hipGetErrorString(e_));                           \
    } while (0)
    const size_t wt_floats = (size_t)std::max<int64_t>(pl.wt_size, 64), nstatus = (size_t)K + 256, nred = (size_t)K * MFAS_MAX_CELLS;
    CREATE_CHK(p->plane.alloc(3 * (size_t)pl.plane_stride));
    CREATE_CHK(p->wt.alloc(wt_floats));
    CREATE_CHK(p->stepbuf.alloc((size_t)pl.step_total));
    CREATE_CHK(p->d_status.alloc(nstatus));   // + debug timestamp slots (MFAS_CHAIN_TIMING builds)
    CREATE_CHK(hipMemset(p->d_status.get(), 0, sizeof(int32_t) * nstatus));
    CREATE_CHK(p->d_seeds.alloc(K));
    CREATE_CHK(p->d_corr.alloc(1));
    CREATE_CHK(p->d_posw.upload(std::vector<float>(pl.g.Cp, 1.0f)));
    CREATE_CHK(p->d_cands.upload(pl.cands));
    CREATE_CHK(p->d_descs.upload(pl.descs));
    p->groups.resize(pl.groups.size());
    for (size_t gi = 0; gi < pl.groups.size(); ++gi) {
        CREATE_CHK(p->groups[gi].d_descs.upload(pl.groups[gi].descs));
        CREATE_CHK(p->groups[gi].d_taps.upload(pl.groups[gi].taps));
    }
    if (pl.red_in_sweep) {
        CREATE_CHK(p->d_red_cnt.alloc(nred));
        CREATE_CHK(hipMemset(p->d_red_cnt.get(), 0, sizeof(uint32_t) * nred));
    }
    if (pl.same_group) CREATE_CHK(p->d_cellflag.alloc((size_t)K * CELLFLAG_STRIDE));
    if (pl.chain_split) CREATE_CHK(p->d_xch.alloc((size_t)K * XCH_CAND_FLOATS));
    CREATE_CHK(hipMemsetAsync(p->plane.get(), 0, sizeof(float) * 3 * (size_t)pl.plane_stride, p->stream));
    CREATE_CHK(hipMemsetAsync(p->wt.get(), 0, sizeof(float) * wt_floats, p->stream));
    CREATE_CHK(hipMemsetAsync(p->stepbuf.get(), 0, sizeof(float) * (size_t)pl.step_total, p->stream));
    CREATE_CHK(set_lds_all(pl));
    if (pl.persist) {
        CREATE_CHK(p->d_pdescs.upload(pl.pdescs));
        CREATE_CHK(p->d_need.upload(pl.need));
        CREATE_CHK(p->d_role.upload(pl.role));
        CREATE_CHK(p->d_sync.alloc((size_t)K * PERSIST_SYNC_STRIDE + 64));
        if (p->tune.persist_trace) {
            CREATE_CHK(p->d_trace.alloc(256));
            CREATE_CHK(hipMemset(p->d_trace.get(), 0, sizeof(unsigned long long) * 256));
        }
    }
    CREATE_CHK(hipStreamSynchronize(p->stream));
#undef CREATE_CHK
    *out = p.release();
    return MFAS_OK;
}

extern "C" int mfas_population_create(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells,
                                      const uint32_t* drop_seeds, int32_t K, int32_t device, void* hip_stream,
                                      int32_t chunk_cols, mfas_population** out) {
    return create_impl(hp, confs, n_cells, drop_seeds, K, device, hip_stream, chunk_cols, out, true);
}

// The layout / schedule decision of mfas_population_create for these configurations WITHOUT creating anything (no allocation, no
// launch): the host's capacity planning (how many candidates one resident round can hold) asks this instead of building and
// destroying populations.
extern "C" int mfas_population_plan(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells, int32_t K, int32_t device,
                                    int32_t chunk_cols, int32_t info[8]) {
    if (!info) return fail(MFAS_EINVAL, "null argument or K <= 0");
    if (int vrc = validate_inputs(hp, confs, n_cells, K)) return vrc;
    const int ncu = device_cus(device);
    LayoutPlan pl;
    if (int prc = plan_layout(hp, confs, n_cells, nullptr, K, chunk_cols, ncu, true, tuning_from_env(), pl)) return prc;
    info[0] = pl.persist ? 1 : 0; info[1] = pl.nres; info[2] = pl.nres_wg; info[3] = pl.res_nu;
    info[4] = pl.chunk; info[5] = (pl.lean_chain ? 1 : 0) | (pl.wide ? 2 : 0); info[6] = ncu; info[7] = K;
    return MFAS_OK;
}

extern "C" void mfas_population_destroy(mfas_population* p) { if (p) delete p; }      // (~mfas_population waits for the stream)

extern "C" int64_t mfas_population_param_count(const mfas_population* p, int32_t k) {
    if (!p || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad candidate index");
    return p->plan.nparams[k];
}

static int check_table(const mfas_population* p, const mfas_table* t, bool need_logits) {
    if (!t || t->N <= 0) return fail(MFAS_EINVAL, "table: null or empty");
    if (p->plan.g.loss_mode == 0 && !t->label) return fail(MFAS_EINVAL, "table: labels missing");
    if (p->plan.g.loss_mode == 1 && !t->multilabel) return fail(MFAS_EINVAL, "table: multi-hot targets missing (loss_mode 1)");
    if (t->dtype < 0 || t->dtype > 2) return fail(MFAS_EINVAL, "table: bad dtype");
    for (int j = 0; j < MFAS_MAX_TAPS; ++j)      // (a width-0 tap is an unused slot: no configuration may select it, so no pointer is needed)
        if ((!t->s[j] && p->plan.g.sw[j] > 0) || (!t->v[j] && p->plan.g.vw[j] > 0)) return fail(MFAS_EINVAL, "table: null tap pointer");
    if (need_logits && (!t->vlogit || !t->slogit)) return fail(MFAS_EINVAL, "multitask needs vlogit/slogit");
    return MFAS_OK;
}

template <int MBE, int NRBW, int MSP, bool XB, bool B3>
static hipError_t launch_eval_t(mfas_population* p, const EvalArgs& a, int ncand, hipStream_t st) {
    const int ME = MBE * 16;
    // (16-bit row tile: half the width, more workgroups per CU)
    size_t lds = (XB || B3) ? ((size_t)ME * std::max((EVAL_CE + 8) / 2, p->plan.g.Cp + 4) + (size_t)ME * (p->plan.g.Rp + 8)) * 4 : p->plan.lds_eval;
    if (XB && MSP == 1 && NRBW == 1 && MBE == 4) lds += (size_t)2 * (EVAL_CE / 16) * 256 * 4;      // the workgroup's weight tiles, double-buffered (eval.hip.h, WL)
    hipError_t e = set_lds(k_eval<MBE, NRBW, MSP, XB, B3>, lds);
    if (e != hipSuccess) return e;
    const unsigned nblk = (unsigned)((a.nrows + ME - 1) / ME);
    EvalArgs b = a;
    b.nblk = (int32_t)nblk;
    b.ncand = ncand;
    b.wl_safe = p->tune.eval_no_wl;
    hipLaunchKernelGGL((k_eval<MBE, NRBW, MSP, XB, B3>), B3 ? dim3(nblk * (unsigned)ncand) : dim3(nblk, ncand), dim3(256), lds, st, b);
    return hipGetLastError();
}

static hipError_t launch_eval(mfas_population* p, const EvalArgs& a, int ncand, hipStream_t st) {
    const Tuning& tu = p->tune;
    const EvalLaunch fn = eval_build(eval_key(plan_facts(p->plan), a.tab.dtype, tu.eval_no_x16, tu.eval_no_msplit, tu.eval_no_b3)).fn;
    return fn ? fn(p, a, ncand, st) : hipErrorInvalidValue;
}

// The rest of the host side — host-only headers, included like plan.hip.h — and the C ABI over it
#include "launches.hip.h"
#include "state.hip.h"
#include "tapgrad.hip.h"
#include "train.hip.h"
#include "vote.hip.h"
#include "tally.hip.h"

extern "C" int mfas_population_set_params(mfas_population* p, int32_t k, const float* flat) {
    if (!p || !flat || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    put_plane(p, k, p->plane.get(), 0, PK_SET, true, flat, p->stream);
    HIPCHK(hipGetLastError());
    return MFAS_OK;
}

extern "C" int mfas_population_get_params(mfas_population* p, int32_t k, int32_t plane, float* flat) {
    if (!p || !flat || k < 0 || k >= p->K || plane < 0 || plane > 3) return fail(MFAS_EINVAL, "bad argument");
    if (plane == 3 && !(p->best && p->prog.keeps_best[k]))
        return fail(MFAS_EINVAL, "plane 3: candidate " + std::to_string(k) + " keeps no best-epoch parameters (no snapshot_best schedule in progress)");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(get_plane(p, k, plane == 3 ? p->best.get() : p->plane.get(), plane == 3 ? 0 : plane, flat, p->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MFAS_OK;
}

extern "C" int mfas_population_init(mfas_population* p, const uint32_t* seeds) {
    if (!p || !seeds) return fail(MFAS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(p->d_seeds.get(), seeds, sizeof(uint32_t) * p->K, hipMemcpyHostToDevice, p->stream));
    run_pack(p, pack_args(p, PK_INIT, 0, nullptr), -1, true, p->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));   // seeds is a host buffer
    return MFAS_OK;
}

extern "C" int mfas_population_set_state(mfas_population* p, int32_t k, int32_t plane, const float* flat) {
    if (!p || !flat || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad argument");
    if (plane < 1 || plane > 3)
        return fail(MFAS_EINVAL, "set_state: plane " + std::to_string(plane) + " (1 = exp_avg, 2 = exp_avg_sq, 3 = kept best; plane 0 is mfas_population_set_params)");
    HIPCHK(hipSetDevice(p->device));
    if (plane == 3) {
        HIPCHK(keep_best(p, BEST_LIVE_IF_NEW, p->stream));
        put_plane(p, k, p->best.get(), 0, PK_PUT, false, flat, p->stream);
        p->prog.keeps_best[k] = 1;
    } else put_plane(p, k, p->plane.get(), plane, PK_PUT, false, flat, p->stream);
    HIPCHK(hipGetLastError());
    return MFAS_OK;
}

extern "C" int mfas_population_get_progress(mfas_population* p, int32_t k, int64_t* epochs_done, int64_t* nb, double* best_metric,
                                            int32_t* status) {
    if (!p || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad argument");
    if (epochs_done) *epochs_done = p->prog.done[k];
    if (nb) *nb = p->prog.nb[k];
    if (best_metric) *best_metric = p->prog.best_metric[k];
    if (status) {
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipMemcpyAsync(status, p->d_status.get() + k, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
    }
    return MFAS_OK;
}

extern "C" int mfas_population_set_progress(mfas_population* p, int32_t k, const int64_t* epochs_done, const int64_t* nb,
                                            const double* best_metric, const int32_t* status) {
    if (!p || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad argument");
    if ((epochs_done && *epochs_done < 0) || (nb && *nb < 0)) return fail(MFAS_EINVAL, "set_progress: negative epoch or batch count");
    if (status) {
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipMemcpyAsync(p->d_status.get() + k, status, sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));      // status is a host word
    }
    if (epochs_done) { p->prog.done[k] = *epochs_done; if (*epochs_done == 0) p->prog.keeps_best[k] = 0; }
    if (nb) p->prog.nb[k] = *nb;
    if (best_metric) p->prog.best_metric[k] = *best_metric;
    return MFAS_OK;
}

extern "C" int mfas_population_train(mfas_population* p, const mfas_table* train, const mfas_table* dev,
                                     const int32_t* order, const float* step_scalars, int32_t epochs,
                                     int64_t max_steps, int32_t snapshot_best, mfas_epoch_stats* stats,
                                     int32_t* status) {
    return train_impl(p, train, dev, order, step_scalars, epochs, max_steps, snapshot_best, stats, status, 0, epochs, false);
}

extern "C" int mfas_population_train_from(mfas_population* p, const mfas_table* train, const mfas_table* dev, const int32_t* order,
                                          const float* step_scalars, int32_t epochs, int32_t first_epoch, int32_t last_epoch,
                                          int32_t snapshot_best, mfas_epoch_stats* stats, int32_t* status) {
    return train_impl(p, train, dev, order, step_scalars, epochs, -1, snapshot_best, stats, status, first_epoch, last_epoch, true);
}

extern "C" int mfas_population_forward(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0,
                                       int64_t nrows, float* logits, int64_t* corrects) {
    if (!p || k < 0 || k >= p->K || nrows <= 0 || row0 < 0) return fail(MFAS_EINVAL, "bad argument");
    int rc = check_table(p, tab, p->plan.g.multitask);
    if (rc) return rc;
    if (row0 + nrows > tab->N) return fail(MFAS_EINVAL, "row range outside the table");
    HIPCHK(hipSetDevice(p->device));
    EvalArgs ea = eval_args(p, *tab, p->plane.get(), p->plan.g);
    ea.row0 = row0; ea.nrows = nrows; ea.cand0 = k; ea.logits = logits;
    if (corrects) {
        HIPCHK(hipMemsetAsync(p->d_corr.get(), 0, sizeof(long long), p->stream));
        ea.corr_out = p->d_corr.get();
    }
    HIPCHK(launch_eval(p, ea, 1, p->stream));
    if (corrects) {
        long long h = 0;
        HIPCHK(hipMemcpyAsync(&h, p->d_corr.get(), sizeof(long long), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        *corrects = (int64_t)h;
    }
    return MFAS_OK;
}

extern "C" int mfas_population_evaluate(mfas_population* p, const mfas_table* tab, int32_t plane, const int32_t* members,
                                        const float* weights, int32_t M, int32_t combine, int64_t scratch_bytes,
                                        mfas_epoch_stats* member_stats, int32_t* member_preds, float* scores,
                                        mfas_epoch_stats* ensemble_stats) {
    return evaluate_impl(p, tab, plane, members, weights, M, combine, scratch_bytes, member_stats, member_preds, scores, ensemble_stats,
                         nullptr, nullptr, nullptr);
}

extern "C" int mfas_population_evaluate_report(mfas_population* p, const mfas_table* tab, int32_t plane, const int32_t* members,
                                               const float* weights, int32_t M, int32_t combine, int64_t scratch_bytes,
                                               mfas_epoch_stats* member_stats, int32_t* member_preds, float* scores,
                                               mfas_epoch_stats* ensemble_stats, int64_t* confusion, int64_t* rank_hist,
                                               int64_t* label_counts) {
    return evaluate_impl(p, tab, plane, members, weights, M, combine, scratch_bytes, member_stats, member_preds, scores, ensemble_stats,
                         confusion, rank_hist, label_counts);
}

extern "C" int mfas_population_forward_train(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows,
                                             int32_t step_index, float* logits) {
    return single_batch(p, k, tab, row0, nrows, step_index, logits, nullptr);      // (refuses a null logits itself)
}

extern "C" int mfas_population_backward(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows,
                                        int32_t step_index, const float* dlogits) {
    return single_batch(p, k, tab, row0, nrows, step_index, nullptr, dlogits);
}

extern "C" int mfas_population_backward_taps(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows,
                                             int32_t step_index, const float* dlogits, float* const* ds, float* const* dv) {
    if (!dlogits) return fail(MFAS_EINVAL, "bad argument");
    return single_batch(p, k, tab, row0, nrows, step_index, nullptr, dlogits, ds, dv);      // (no pointer set: mfas_population_backward)
}

extern "C" int mfas_stream_probe(int64_t bytes_per_plane, int32_t iters, double* gb_per_s) {
    if (bytes_per_plane < (1 << 20) || iters < 1 || !gb_per_s) return fail(MFAS_EINVAL, "bad argument");
    const size_t plane = (size_t)bytes_per_plane / 1024 * 256;   // floats, whole tiles
    DevBuf<float> P;
    HIPCHK(P.alloc(plane * 3));
    hipError_t e = hipMemset(P.get(), 0, plane * 4 * 3);
    hipEvent_t a = nullptr, b = nullptr;
    if (e == hipSuccess) e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    float ms = 0.f;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_stream_probe, dim3(2048), dim3(256), 0, 0, P.get(), plane, plane / 256);
        hipEventRecord(a, 0);
        for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(k_stream_probe, dim3(2048), dim3(256), 0, 0, P.get(), plane, plane / 256);
        hipEventRecord(b, 0);
        e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    }
    if (a) hipEventDestroy(a);      // (both events go on every path)
    if (b) hipEventDestroy(b);
    if (e != hipSuccess) return fail(MFAS_EHIP, hipGetErrorString(e));
    *gb_per_s = (double)plane * 4 * 3 * 2 * iters / 1e9 / (ms * 1e-3);
    return MFAS_OK;
}

extern "C" int mfas_global_pool(const void* x, int32_t dtype, int64_t rows, int64_t inner, void* out, int32_t out_dtype,
                                void* hip_stream) {
    if (!x || !out || rows <= 0 || inner <= 0 || dtype < 0 || dtype > 2 || out_dtype < 0 || out_dtype > 2)
        return fail(MFAS_EINVAL, "bad argument");
    const int64_t nblk = (rows + 3) / 4;
    if (nblk > 0x7FFFFFFF) return fail(MFAS_EINVAL, "too many rows");
    hipLaunchKernelGGL(k_pool, dim3((unsigned)nblk), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), x, (int)dtype,
                       rows, inner, out, (int)out_dtype);
    HIPCHK(hipGetLastError());
    return MFAS_OK;
}

extern "C" int mfas_population_set_pos_weight(mfas_population* p, const float* w) {
    if (!p || !w) return fail(MFAS_EINVAL, "null");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpy(p->d_posw.get(), w, sizeof(float) * p->plan.g.C, hipMemcpyHostToDevice));
    return MFAS_OK;
}

extern "C" int mfas_population_set_best_threshold(mfas_population* p, double threshold) {
    if (!p) return fail(MFAS_EINVAL, "null");
    p->best_threshold = threshold;
    return MFAS_OK;
}

extern "C" int mfas_population_set_profiling(mfas_population* p, int32_t on) {
    if (!p) return fail(MFAS_EINVAL, "null");
    p->profiling = on != 0;
    p->prof_every = p->tune.prof_every;
    return MFAS_OK;
}

extern "C" int mfas_population_schedule(const mfas_population* p, int32_t info[8]) {
    if (!p || !info) return fail(MFAS_EINVAL, "null");
    const LayoutPlan& pl = p->plan;
    info[0] = pl.persist ? 1 : 0; info[1] = pl.nres; info[2] = pl.nres_wg; info[3] = pl.res_nu;
    info[4] = pl.res_chain ? 1 : 0; info[5] = (pl.lean_chain ? 1 : 0) | (pl.wide ? 2 : 0) | (std::max(1, pl.chain_split) << 8); info[6] = pl.same_group ? -1 : (int32_t)pl.groups.size(); info[7] = p->K;
    return MFAS_OK;
}

// "family<template arguments>:launches ..." of the builds the last train call launched, sorted by name
extern "C" int mfas_population_launch_record(const mfas_population* p, char* buf, int32_t cap) {
    if (!p || !buf || cap <= 0) return fail(MFAS_EINVAL, "null");
    snprintf(buf, (size_t)cap, "%s", p->launched.describe().c_str());
    return MFAS_OK;
}

extern "C" int mfas_population_sweep_profile(const mfas_population* p, int64_t* launches, double* total_ms,
                                             double* bytes_per_launch) {
    if (!p) return fail(MFAS_EINVAL, "null");
    if (launches) *launches = p->prof_launches;
    if (total_ms) *total_ms = p->prof_ms;
    if (bytes_per_launch) *bytes_per_launch = p->bytes_per_launch;
    return MFAS_OK;
}
