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
// Source layout (ONE translation unit; this file includes the rest): common.hip.h (device records, helpers, LDS
// staging), sweep.hip.h (tile_run, sweep_body, sweep_tap_body), chain.hip.h (chain_body, chain_lean, softmax / BCE rows),
// wide.hip.h (k_chain_wide / k_sweep_wide: the batch walked in tiles, for batch sizes and widths the others cannot hold),
// eval.hip.h (k_eval), pack.hip.h (k_pack, k_vec, k_pool, k_stream_probe), plan.hip.h (host only: the switches, validate_inputs and
// plan_layout — layout, schedule, LDS budgets and work lists decided before anything is allocated); below: k_step / k_chain, the kernel
// tables (one function per kernel family: the only place an instantiation is named) and the host C ABI.
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
#include <algorithm>
#include <string>
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
    else sweep_body<MB, NT, SweepU<MB, WPE>::v>(a.sa, sweep_step_of(a.sa), bid - a.nchain - a.ga.nblocks - a.sa.ntap, lds);
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

#include "plan.hip.h"

// ================================================================================================
// Host side: C ABI
// ================================================================================================
struct mfas_population {
    mfas_hyper hp;
    Tuning tune;                    // the environment switches as they stood when the population was created
    int K = 0, device = 0, n_cus = 0;
    int chunk_cols_req = 0;         // chunk_cols the caller asked for at creation (the fallback layout is built with the same request)
    hipStream_t stream = nullptr;
    LayoutPlan plan;                // layout, schedule, LDS budgets, work lists (plan.hip.h): decided before anything was allocated, never changed
    float* plane = nullptr;
    float* wt = nullptr;
    float* stepbuf = nullptr;
    float* best = nullptr;          // snapshot_best: copy of plane 0
    CandDev* d_cands = nullptr;
    SegDesc* d_descs = nullptr;
    struct GroupDev { SegDesc* d_descs = nullptr; TapDesc* d_taps = nullptr; };
    std::vector<GroupDev> groups;   // device copies of plan.groups[i].descs / .taps
    DevStats* d_stats = nullptr;
    int32_t* d_status = nullptr;
    uint32_t* d_seeds = nullptr;
    long long* d_corr = nullptr;
    float* d_posw = nullptr;        // loss_mode 1: per-class positive weights (default 1)
    int stats_cap = 0;
    // profiling of the dominant kernel
    bool profiling = false;
    int prof_every = 16;            // HIP events bracket every prof_every-th sweep launch (event records are not free)
    std::vector<hipEvent_t> ev;     // pairs
    int64_t prof_launches = 0;
    double prof_ms = 0.0, bytes_per_launch = 0.0, prof_bytes = 0.0;
    double best_threshold = 0.0;    // snapshot_best: a dev metric must exceed this to count (init_f1, mmimdb.py:18; 0 for NTU)
    // Progress record (mfas_population_train_from): what train_ntu_track_acc keeps on its stack for one call (best_acc,
    // train_searchable/ntu.py:18,82-83) and where in its schedule every candidate stands, kept between calls.  Per candidate: a moved
    // candidate (mfas_population_move) brings its own.
    struct Progress {
        std::vector<int64_t> done, nb;      // epochs of the schedule that are complete; that schedule's batches per epoch
        std::vector<double> best_metric;    // best dev metric so far (starts at best_threshold)
        std::vector<int32_t> keeps_best;    // the schedule runs with snapshot_best: plane `best` holds this candidate's best epoch
        void reset(int K, double threshold) { done.assign(K, 0); nb.assign(K, 0); best_metric.assign(K, threshold); keeps_best.assign(K, 0); }
    } prog;
    float* d_move = nullptr;        // mfas_population_move: one candidate in flat state_dict order (grow-only scratch of the destination)
    int64_t move_cap = 0;
    uint32_t* d_red_cnt = nullptr;  // reduce-in-sweep arrival counters [K][4] (small populations, general chain)
    char* d_gather = nullptr;       // gathered rows [K][2 parities][taps][Bp][width] (two-group schedule, per-candidate orders; sweep.hip.h)
    size_t gather_cap = 0;
    uint32_t* d_cellflag = nullptr; // [K][CELLFLAG_STRIDE]
    float* d_xch = nullptr;         // chain_split's exchange area [K][XCH_CAND_FLOATS]
    // persistent step loop (persist.hip.h)
    SegDesc* d_pdescs = nullptr;    // plan.pdescs
    int fell_back = 0;              // the resident schedule was given up for launch-per-phase inside a train() call (roll call never complete)
    uint32_t* d_sync = nullptr;     // [K] flags | [K] counters | abort word (zeroed before every launch)
    int32_t* d_need = nullptr;      // plan.need
    int32_t* d_role = nullptr;      // plan.role
    float* d_scal = nullptr;        // device copy of the step scalars
    size_t scal_cap = 0;
    unsigned long long* d_trace = nullptr;
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
// Kernel tables: every instantiation of a family is named HERE and nowhere else.  create sets the dynamic-LDS limit through these
// functions (set_lds_all) and train / single_batch launch through them, so a build cannot be launched without its limit having been set.
// A parameter combination that is not built gives nullptr.
// ------------------------------------------------------------------------------------------------
typedef void (*StepKernel)(const StepArgs);
typedef void (*ChainKernel)(const ChainArgs);
typedef void (*PresidentKernel)(const PersistArgs, const int);

// (the order below is the order the builds come out in the code object: tools/kernel_resources.py lists them that way)
static StepKernel same_kernel(int MB, bool nt, int ns) {
#define K_(M, S) if (MB == M && ns == S) return !nt ? k_step_same<M, false, S> : k_step_same<M, true, S>
    K_(1, 1); K_(2, 1); K_(1, 4);
#undef K_
    return nullptr;
}

static StepKernel step_kernel(int MB, bool nt, int wpe, bool lean, int ns) {
#define K_(M, W, F, S) if (MB == M && wpe == W && lean == F && ns == S) return !nt ? k_step<M, false, W, F, S> : k_step<M, true, W, F, S>
    K_(1, 4, false, 4);
    K_(1, 4, false, 1); K_(2, 2, false, 1); K_(2, 4, false, 1); K_(4, 2, false, 1);
    K_(1, 4, true, 1); K_(2, 2, true, 1); K_(2, 4, true, 1);
#undef K_
    return nullptr;
}

static ChainKernel chain_kernel(int MB, bool lean) {
    if (!lean && MB == 1) return k_chain<1, false>;
    if (!lean && MB == 2) return k_chain<2, false>;
    if (!lean && MB == 4) return k_chain<4, false>;
    if (lean && MB == 1) return k_chain<1, true>;
    if (lean && MB == 2) return k_chain<2, true>;
    return nullptr;
}

// the wide path (wide.hip.h): one chain build, the sweep with cached / nontemporal W/m/v streaming
static ChainKernel wide_chain_kernel() { return k_chain_wide; }
static StepKernel wide_sweep_kernel(bool nt) { return !nt ? k_sweep_wide<false> : k_sweep_wide<true>; }

// one instantiation per unit form: f32 staging (one or two units per workgroup), 16-bit staging (the same, or one WIDE unit of up to
// 1024 columns); plain: the chain compiled for the search default (1), for `--batchnorm` alone (2), or the general one (0)
static PresidentKernel president_kernel(int MB, bool x16, bool wide, int nu, int plain) {
#define K_(M, P) if (MB == M && plain == P) { \
        if (!x16) return nu != 2 ? k_president<M, PERSIST_NTR, false, 1, P> : k_president<M, PERSIST_NTR, false, 2, P>; \
        if (wide) return k_president<M, PERSIST_NTR16, true, 1, P>; \
        return nu != 2 ? k_president<M, PERSIST_NTR, true, 1, P> : k_president<M, PERSIST_NTR, true, 2, P>; }
    K_(1, 0) K_(2, 0) K_(1, 1) K_(2, 1) K_(1, 2) K_(2, 2)
#undef K_
    return nullptr;
}

template <typename... A>
static void launch(void (*kernel)(A...), unsigned grid, size_t lds, hipStream_t stream, A... args) {
    void* argv[] = {const_cast<void*>(static_cast<const void*>(&args))...};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3(grid), dim3(STEP_THREADS), argv, lds, stream);    // (errors: hipGetLastError)
}

// the dynamic-LDS limit of every build a population with this plan may launch
static hipError_t set_lds_all(const LayoutPlan& pl) {
    hipError_t e = hipSuccess;
    auto set = [&e](auto kernel, size_t bytes) { if (kernel && e == hipSuccess) e = set_lds(kernel, bytes); };
    if (pl.wide) {
        set(wide_chain_kernel(), pl.lds_chain);
        for (int b = 0; b < 2; ++b) set(wide_sweep_kernel(b), pl.lds_step);
        return e;
    }
    for (int MB : {1, 2, 4})
        for (int b = 0; b < 2; ++b) {      // b: nontemporal (k_step*), lean (k_chain), 16-bit staging (k_president)
            for (int wpe : {2, 4}) { set(step_kernel(MB, b, wpe, false, 1), pl.lds_step); set(step_kernel(MB, b, wpe, true, 1), pl.lds_step); }
            if (pl.same_group) set(same_kernel(MB, b, 1), pl.lds_step);
            if (pl.chain_split) { set(same_kernel(MB, b, 4), pl.lds_split); set(step_kernel(MB, b, 4, false, 4), pl.lds_split); }
            set(chain_kernel(MB, b), pl.lds_chain);
            if (pl.persist)
                for (int plain = 0; plain < 3; ++plain) {
                    set(president_kernel(MB, b, false, 1, plain), pl.lds_president); set(president_kernel(MB, b, false, 2, plain), pl.lds_president);
                    if (b) set(president_kernel(MB, true, true, 1, plain), pl.lds_president);
                }
        }
    return e;
}

static int device_cus(int device) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
    return ncu;
}

template <typename T>
static hipError_t upload(T** dst, const std::vector<T>& v) {      // (an empty list stays a null pointer)
    if (v.empty()) return hipSuccess;
    hipError_t e = hipMalloc(dst, sizeof(T) * v.size());
    return e != hipSuccess ? e : hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

// validate -> plan (pure: plan.hip.h) -> allocate / upload / set the LDS limits from the plan; one error path that frees what was allocated
static int create_impl(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells,
                       const uint32_t* drop_seeds, int32_t K, int32_t device, void* hip_stream,
                       int32_t chunk_cols, mfas_population** out, const bool allow_persist, const Tuning* inherit = nullptr) {
    if (!out) return fail(MFAS_EINVAL, "null argument or K <= 0");
    if (int vrc = validate_inputs(hp, confs, n_cells, K)) return vrc;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(MFAS_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    mfas_population* p = new (std::nothrow) mfas_population();
    if (!p) return fail(MFAS_ENOMEM, "host alloc");
    p->hp = *hp;
    p->tune = inherit ? *inherit : tuning_from_env();      // (persist_fallback rebuilds a population under the switches it was created with)
    p->K = K;
    p->device = device;
    p->stream = reinterpret_cast<hipStream_t>(hip_stream);
    p->chunk_cols_req = chunk_cols;
    p->n_cus = device_cus(device);
    p->prog.reset(K, 0.0);
    if (int prc = plan_layout(hp, confs, n_cells, drop_seeds, K, chunk_cols, p->n_cus, allow_persist, p->tune, p->plan)) { delete p; return prc; }
    const LayoutPlan& pl = p->plan;
    if (!pl.fits_lds) { delete p; return fail(MFAS_EINVAL, "geometry does not fit the 160 KiB LDS (R / batchsize too large)"); }
    p->bytes_per_launch = pl.bytes_per_launch;

#define CREATE_CHK(x)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            std::string m_ = std::string(#x) + ": " + hipGetErrorString(e_);                       \
            mfas_population_destroy(p);                                                            \
            return fail(e_ == hipErrorOutOfMemory ? MFAS_ENOMEM : MFAS_EHIP, m_);                  \
        }                                                                                          \
    } while (0)
    const size_t wt_floats = (size_t)std::max<int64_t>(pl.wt_size, 64);
    CREATE_CHK(hipMalloc(&p->plane, sizeof(float) * 3 * (size_t)pl.plane_stride));
    CREATE_CHK(hipMalloc(&p->wt, sizeof(float) * wt_floats));
    CREATE_CHK(hipMalloc(&p->stepbuf, sizeof(float) * (size_t)pl.step_total));
    CREATE_CHK(hipMalloc(&p->d_status, sizeof(int32_t) * (K + 256)));   // + debug timestamp slots (MFAS_CHAIN_TIMING builds)
    CREATE_CHK(hipMemset(p->d_status, 0, sizeof(int32_t) * (K + 256)));
    CREATE_CHK(hipMalloc(&p->d_seeds, sizeof(uint32_t) * K));
    CREATE_CHK(hipMalloc(&p->d_corr, sizeof(long long)));
    CREATE_CHK(upload(&p->d_posw, std::vector<float>(pl.g.Cp, 1.0f)));
    CREATE_CHK(upload(&p->d_cands, pl.cands));
    CREATE_CHK(upload(&p->d_descs, pl.descs));
    p->groups.resize(pl.groups.size());
    for (size_t gi = 0; gi < pl.groups.size(); ++gi) {
        CREATE_CHK(upload(&p->groups[gi].d_descs, pl.groups[gi].descs));
        CREATE_CHK(upload(&p->groups[gi].d_taps, pl.groups[gi].taps));
    }
    if (pl.red_in_sweep) {
        CREATE_CHK(hipMalloc(&p->d_red_cnt, sizeof(uint32_t) * K * MFAS_MAX_CELLS));
        CREATE_CHK(hipMemset(p->d_red_cnt, 0, sizeof(uint32_t) * K * MFAS_MAX_CELLS));
    }
    if (pl.same_group) CREATE_CHK(hipMalloc(&p->d_cellflag, sizeof(uint32_t) * K * CELLFLAG_STRIDE));
    if (pl.chain_split) CREATE_CHK(hipMalloc(&p->d_xch, sizeof(float) * (size_t)K * XCH_CAND_FLOATS));
    CREATE_CHK(hipMemsetAsync(p->plane, 0, sizeof(float) * 3 * (size_t)pl.plane_stride, p->stream));
    CREATE_CHK(hipMemsetAsync(p->wt, 0, sizeof(float) * wt_floats, p->stream));
    CREATE_CHK(hipMemsetAsync(p->stepbuf, 0, sizeof(float) * (size_t)pl.step_total, p->stream));
    CREATE_CHK(set_lds_all(pl));
    if (pl.persist) {
        CREATE_CHK(upload(&p->d_pdescs, pl.pdescs));
        CREATE_CHK(upload(&p->d_need, pl.need));
        CREATE_CHK(upload(&p->d_role, pl.role));
        CREATE_CHK(hipMalloc(&p->d_sync, sizeof(uint32_t) * ((size_t)K * PERSIST_SYNC_STRIDE + 64)));
        if (p->tune.persist_trace) {
            CREATE_CHK(hipMalloc(&p->d_trace, sizeof(unsigned long long) * 256));
            CREATE_CHK(hipMemset(p->d_trace, 0, sizeof(unsigned long long) * 256));
        }
    }
    CREATE_CHK(hipStreamSynchronize(p->stream));
#undef CREATE_CHK
    *out = p;
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

extern "C" void mfas_population_destroy(mfas_population* p) {
    if (!p) return;
    hipSetDevice(p->device);
    hipStreamSynchronize(p->stream);
    for (hipEvent_t e : p->ev) hipEventDestroy(e);
    hipFree(p->plane); hipFree(p->wt); hipFree(p->stepbuf); hipFree(p->best);
    for (auto& gr : p->groups) { hipFree(gr.d_descs); hipFree(gr.d_taps); }
    hipFree(p->d_cands); hipFree(p->d_descs); hipFree(p->d_stats); hipFree(p->d_status);
    hipFree(p->d_seeds); hipFree(p->d_corr); hipFree(p->d_posw);
    hipFree(p->d_red_cnt);
    hipFree(p->d_gather);
    hipFree(p->d_cellflag);
    hipFree(p->d_xch);
    hipFree(p->d_move);
    hipFree(p->d_sync); hipFree(p->d_need); hipFree(p->d_role); hipFree(p->d_scal); hipFree(p->d_trace); hipFree(p->d_pdescs);
    delete p;
}

extern "C" int64_t mfas_population_param_count(const mfas_population* p, int32_t k) {
    if (!p || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad candidate index");
    return p->plan.nparams[k];
}

static PackArgs pack_args(mfas_population* p, int mode, int plane, float* flat) {
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.desc = p->d_descs; a.cands = p->d_cands; a.plane = p->plane; a.plane_stride = p->plan.plane_stride;
    a.wt = p->wt; a.flat = flat; a.seeds = p->d_seeds; a.mode = mode; a.sel_plane = plane; a.g = p->plan.g;
    return a;
}

extern "C" int mfas_population_set_params(mfas_population* p, int32_t k, const float* flat) {
    if (!p || !flat || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    PackArgs a = pack_args(p, PK_SET, 0, const_cast<float*>(flat));
    a.desc = p->d_descs + p->plan.desc_start[k];
    const int n = p->plan.desc_start[k + 1] - p->plan.desc_start[k];
    hipLaunchKernelGGL(k_pack, dim3(n), dim3(256), 0, p->stream, a);
    hipLaunchKernelGGL(k_vec, dim3(1), dim3(256), 0, p->stream, a, (int)k);
    HIPCHK(hipGetLastError());
    return MFAS_OK;
}

extern "C" int mfas_population_get_params(mfas_population* p, int32_t k, int32_t plane, float* flat) {
    if (!p || !flat || k < 0 || k >= p->K || plane < 0 || plane > 3) return fail(MFAS_EINVAL, "bad argument");
    if (plane == 3 && !(p->best && p->prog.keeps_best[k]))
        return fail(MFAS_EINVAL, "plane 3: candidate " + std::to_string(k) + " keeps no best-epoch parameters (no snapshot_best schedule in progress)");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemsetAsync(flat, 0, sizeof(float) * p->plan.nparams[k], p->stream));
    PackArgs a = pack_args(p, PK_GET, plane == 3 ? 0 : plane, flat);
    if (plane == 3) a.plane = p->best;      // (a full image of plane 0, BatchNorm running statistics included)
    a.desc = p->d_descs + p->plan.desc_start[k];
    const int n = p->plan.desc_start[k + 1] - p->plan.desc_start[k];
    hipLaunchKernelGGL(k_pack, dim3(n), dim3(256), 0, p->stream, a);
    hipLaunchKernelGGL(k_vec, dim3(1), dim3(256), 0, p->stream, a, (int)k);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MFAS_OK;
}

extern "C" int mfas_population_init(mfas_population* p, const uint32_t* seeds) {
    if (!p || !seeds) return fail(MFAS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(p->d_seeds, seeds, sizeof(uint32_t) * p->K, hipMemcpyHostToDevice, p->stream));
    PackArgs a = pack_args(p, PK_INIT, 0, nullptr);
    hipLaunchKernelGGL(k_pack, dim3((unsigned)p->plan.descs.size()), dim3(256), 0, p->stream, a);
    hipLaunchKernelGGL(k_vec, dim3(p->K), dim3(256), 0, p->stream, a, -1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));   // seeds is a host buffer
    return MFAS_OK;
}

// torch.manual_seed(seeds[k]) + the module's construction draws for every candidate, on the device (k_mt_uniform, pack.hip.h).
// bounds: per candidate 2 * (MFAS_MAX_CELLS + 1) floats — per cell {weight bound, bias bound}, then the classifier's — as the host
// computed them (kaiming_uniform_(a = sqrt 5) / 1 / sqrt(fan_in), nn.Linear.reset_parameters); alphas ~ N(alpha_mean, alpha_std)
// drawn LAST like Searchable_Skeleton_Image_Net.__init__ does (ntu_searchable.py:202-204), from the stream's next raw outputs with
// at::normal_distribution<double>'s arithmetic (Box-Muller: r = sqrt(-2 log1p(-u2)), theta = 2 pi u1; the sine sample is cached
// for the next draw) in host double precision / libm, exactly what torch's CPU path evaluates.
extern "C" int mfas_population_init_torch_streams(mfas_population* p, const uint64_t* seeds, const float* bounds, double alpha_mean,
                                                  double alpha_std) {
    if (!p || !seeds || !bounds) return fail(MFAS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    const int K = p->K, R = p->hp.R, C = p->hp.C, NB = 2 * (MFAS_MAX_CELLS + 1);
    int64_t maxp = 0;
    for (int k = 0; k < K; ++k) maxp = std::max(maxp, p->plan.nparams[k]);
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(K, (64LL << 20) / std::max<int64_t>(maxp, 1)));     // <= 256 MB of flat scratch
    float* flat = nullptr;
    MtCand* d_mt = nullptr;
    uint32_t* d_tail = nullptr;
    auto cleanup = [&]() { hipFree(flat); hipFree(d_mt); hipFree(d_tail); };
    hipError_t e = hipMalloc(&flat, sizeof(float) * (size_t)maxp * batch);
    if (e == hipSuccess) e = hipMalloc(&d_mt, sizeof(MtCand) * batch);
    if (e == hipSuccess) e = hipMalloc(&d_tail, sizeof(uint32_t) * MT_TAIL * batch);
    if (e != hipSuccess) { cleanup(); return fail(MFAS_ENOMEM, std::string("init_torch_streams: ") + hipGetErrorString(e)); }
    std::vector<MtCand> mt(batch);
    std::vector<uint32_t> tails((size_t)MT_TAIL * batch);
    std::vector<float> alpha((size_t)MFAS_MAX_CELLS * batch);
    for (int k0 = 0; k0 < K && e == hipSuccess; k0 += batch) {
        const int nb = std::min(batch, K - k0);
        for (int j = 0; j < nb; ++j) {
            const int k = k0 + j;
            const CandDev& c = p->plan.cands[k];
            MtCand& m = mt[j];
            memset(&m, 0, sizeof(m));
            m.seed = (uint32_t)(seeds[k] & 0xffffffffULL);
            m.flat_off = (int64_t)j * maxp;
            int64_t pos = 0;
            auto seg = [&](int64_t dst, int64_t n, float b) {
                m.start[m.nseg] = pos; m.dst[m.nseg] = dst; m.lo[m.nseg] = -b; m.hi[m.nseg] = b;
                pos += n; ++m.nseg;
            };
            for (int i = 0; i < c.L; ++i) {
                seg(c.f_W[i], (int64_t)R * c.K_in[i], bounds[k * NB + 2 * i]);
                seg(c.f_b[i], R, bounds[k * NB + 2 * i + 1]);
            }
            seg(c.f_Wc, (int64_t)C * R, bounds[k * NB + 2 * MFAS_MAX_CELLS]);
            seg(c.f_bc, C, bounds[k * NB + 2 * MFAS_MAX_CELLS + 1]);
            m.start[m.nseg] = pos;
            m.total = pos;
        }
        e = hipMemcpyAsync(d_mt, mt.data(), sizeof(MtCand) * nb, hipMemcpyHostToDevice, p->stream);
        if (e == hipSuccess) e = hipMemsetAsync(flat, 0, sizeof(float) * (size_t)maxp * nb, p->stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_mt_uniform, dim3(nb), dim3(256), 0, p->stream, d_mt, flat, d_tail);
        e = hipMemcpyAsync(tails.data(), d_tail, sizeof(uint32_t) * MT_TAIL * nb, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) break;
        for (int j = 0; j < nb && e == hipSuccess; ++j) {
            const int k = k0 + j;
            const CandDev& c = p->plan.cands[k];
            // BatchNorm defaults (gamma = 1, running_var = 1) and the alphas, then the usual repacking of a flat vector
            const uint32_t* t = tails.data() + (size_t)j * MT_TAIL;
            int used = 0;
            bool cached = false;
            double cache = 0.0;
            auto u53 = [&]() {      // uniform_real_distribution<double>: random64() = (first << 32) | second, 53 bits
                const uint64_t hi = t[used], lo = t[used + 1];
                used += 2;
                return (double)(((hi << 32) | lo) & ((1ULL << 53) - 1)) * (1.0 / 9007199254740992.0);
            };
            for (int i = 0; i < c.L; ++i) {
                double z;
                if (cached) { z = cache; cached = false; }
                else {
                    const double u1 = u53(), u2 = u53();
                    const double r = ::sqrt(-2.0 * ::log1p(-u2)), theta = 2.0 * 3.14159265358979323846 * u1;
                    cache = r * ::sin(theta);
                    cached = true;
                    z = r * ::cos(theta);
                }
                alpha[(size_t)j * MFAS_MAX_CELLS + i] = (float)(z * alpha_std + alpha_mean);
            }
            float* fk = flat + (int64_t)j * maxp;
            e = hipMemcpyAsync(fk + c.f_alpha, alpha.data() + (size_t)j * MFAS_MAX_CELLS, sizeof(float) * c.L, hipMemcpyHostToDevice, p->stream);
            if (e != hipSuccess) break;
            if (p->hp.bn) {
                for (int i = 0; i < c.L && e == hipSuccess; ++i) {
                    hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, p->stream, fk + c.f_bn[i], 1.0f, (int64_t)R);             // gamma
                    hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, p->stream, fk + c.f_bn[i] + 3 * (int64_t)R, 1.0f, (int64_t)R);   // running_var
                }
            }
            const int rc = mfas_population_set_params(p, k, fk);
            if (rc) { cleanup(); return rc; }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);       // the scratch is reused by the next batch
    }
    cleanup();
    if (e != hipSuccess) return fail(MFAS_EHIP, std::string("init_torch_streams: ") + hipGetErrorString(e));
    return MFAS_OK;
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

template <int MBE, int NRBW, int MSP = 0, bool XB = false, bool B3 = false>
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
    // one or two row blocks (R <= 32): the m-blocks of a row tile are split over the four waves (eval.hip.h)
    // (bf16 tables: the rows stay 16-bit in LDS)
    const bool xb = a.tab.dtype == MFAS_DT_BF16 && !p->tune.eval_no_x16;
#define EV_SPLIT(M, S) if (p->plan.mbe == M && p->plan.nrbw == 1 && p->plan.g.nrb == S && !p->tune.eval_no_msplit) \
        return xb ? launch_eval_t<M, 1, S, true>(p, a, ncand, st) : launch_eval_t<M, 1, S, false>(p, a, ncand, st);
    EV_SPLIT(4, 1) EV_SPLIT(4, 2) EV_SPLIT(2, 1) EV_SPLIT(2, 2) EV_SPLIT(1, 1) EV_SPLIT(1, 2)
#undef EV_SPLIT
    // two row blocks per wave (R = 72 .. 128), bf16 tables: exact bf16 x 3 feature products on the bf16 matrix pipe
    if (a.tab.dtype == MFAS_DT_BF16 && p->plan.nrbw == 2 && !p->tune.eval_no_b3) {
        if (p->plan.mbe == 4) return launch_eval_t<4, 2, 0, false, true>(p, a, ncand, st);
        if (p->plan.mbe == 2) return launch_eval_t<2, 2, 0, false, true>(p, a, ncand, st);
        if (p->plan.mbe == 1) return launch_eval_t<1, 2, 0, false, true>(p, a, ncand, st);
    }
#define EV_CASE(M, N) if (p->plan.mbe == M && p->plan.nrbw == N) return launch_eval_t<M, N>(p, a, ncand, st);
    EV_CASE(4, 1) EV_CASE(4, 2) EV_CASE(4, 4) EV_CASE(4, 8)
    EV_CASE(2, 1) EV_CASE(2, 2) EV_CASE(2, 4) EV_CASE(2, 8)
    EV_CASE(1, 1) EV_CASE(1, 2) EV_CASE(1, 4) EV_CASE(1, 8)
#undef EV_CASE
    return hipErrorInvalidValue;
}

// The resident persistent schedule needs every workgroup of its two launches on the GPU at the same time.  When that cannot be
// had — another process keeps CUs busy for good, the device is CU-masked, a tool serialises the two launches — the roll call fails
// BEFORE anything of the epoch has run (abort code 2), so the state in memory is that of the last completed epoch: rebuild the
// population in its launch-per-phase layout, carry W / m / v (+ the best-epoch snapshot) across through the reference's flat
// parameter order, and go on from the same epoch.  The handle keeps its identity: the two records swap contents.
static int persist_fallback(mfas_population* p) {
    const int K = p->K;
    std::vector<int32_t> confs((size_t)K * 12, 0), ncells(K);
    std::vector<uint32_t> seeds(K);
    int64_t maxp = 0;
    for (int k = 0; k < K; ++k) {
        const CandDev& c = p->plan.cands[k];
        ncells[k] = c.L;
        seeds[k] = c.drop_seed;
        for (int i = 0; i < c.L; ++i)
            for (int j = 0; j < 3; ++j) confs[(k * 4 + i) * 3 + j] = c.conf[i][j];
        maxp = std::max(maxp, p->plan.nparams[k]);
    }
    mfas_population* q = nullptr;
    int rc = create_impl(&p->hp, confs.data(), ncells.data(), seeds.data(), K, p->device, p->stream, p->chunk_cols_req, &q, false, &p->tune);
    if (rc) return rc;
    float* flat = nullptr;
    hipError_t e = hipMalloc(&flat, sizeof(float) * (size_t)maxp);
    if (e != hipSuccess) { mfas_population_destroy(q); return fail(MFAS_ENOMEM, "persist_fallback: scratch"); }
    if (p->best && !q->best) {
        e = hipMalloc(&q->best, sizeof(float) * (size_t)q->plan.plane_stride);
        if (e == hipSuccess) e = hipMemsetAsync(q->best, 0, sizeof(float) * (size_t)q->plan.plane_stride, p->stream);
        if (e != hipSuccess) { hipFree(flat); mfas_population_destroy(q); return fail(MFAS_ENOMEM, "persist_fallback: snapshot"); }
    }
    auto move = [&](int k, float* src_plane, int src_sel, float* dst_plane, int dst_sel, int mode, bool with_wt) {
        PackArgs a = pack_args(p, PK_GET, src_sel, flat);
        a.plane = src_plane;
        a.desc = p->d_descs + p->plan.desc_start[k];
        hipMemsetAsync(flat, 0, sizeof(float) * p->plan.nparams[k], p->stream);
        hipLaunchKernelGGL(k_pack, dim3(p->plan.desc_start[k + 1] - p->plan.desc_start[k]), dim3(256), 0, p->stream, a);
        hipLaunchKernelGGL(k_vec, dim3(1), dim3(256), 0, p->stream, a, k);
        PackArgs b = pack_args(q, mode, dst_sel, flat);
        b.plane = dst_plane;
        if (!with_wt) b.wt = nullptr;
        b.desc = q->d_descs + q->plan.desc_start[k];
        hipLaunchKernelGGL(k_pack, dim3(q->plan.desc_start[k + 1] - q->plan.desc_start[k]), dim3(256), 0, p->stream, b);
        hipLaunchKernelGGL(k_vec, dim3(1), dim3(256), 0, p->stream, b, k);
    };
    for (int k = 0; k < K; ++k) {
        move(k, p->plane, 0, q->plane, 0, PK_SET, true);        // W (+ transposed OUT / HEAD images), zeroes m / v
        move(k, p->plane, 1, q->plane, 1, PK_PUT, false);       // Adam first moment
        move(k, p->plane, 2, q->plane, 2, PK_PUT, false);       // Adam second moment
        if (p->best) move(k, p->best, 0, q->best, 0, PK_PUT, false);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_posw, p->d_posw, sizeof(float) * p->plan.g.Cp, hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_status, p->d_status, sizeof(int32_t) * K, hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    hipFree(flat);
    if (e != hipSuccess) { mfas_population_destroy(q); return fail(MFAS_EHIP, std::string("persist_fallback: ") + hipGetErrorString(e)); }
    std::swap(q->d_stats, p->d_stats);
    std::swap(q->stats_cap, p->stats_cap);
    std::swap(q->d_scal, p->d_scal);
    std::swap(q->scal_cap, p->scal_cap);
    q->best_threshold = p->best_threshold;
    q->prog = p->prog;
    q->profiling = p->profiling;
    q->prof_every = p->prof_every;
    q->ev.swap(p->ev);
    q->fell_back = 1;
    std::swap(*p, *q);
    mfas_population_destroy(q);      // the resident layout
    return MFAS_OK;
}

// ------------------------------------------------------------------------------------------------
// mfas_population_train: the state of one call and the launches of the two schedules over it
// ------------------------------------------------------------------------------------------------
struct TrainCall {
    mfas_population* p = nullptr;
    const mfas_table* train = nullptr;
    const int32_t* order = nullptr;
    const float* step_scalars = nullptr;
    int epochs = 0, B = 0;
    int64_t N = 0, nb = 0;              // train rows, batches per epoch
    AdamC ac;
    StepArgs st;
    int NG = 0;                         // candidate groups A/B: every launch pairs the sweep of one group with the chain of the other (k_step)
    int64_t split_launches[2] = {0, 0}; // chain_split launches of this call per candidate group (exchange parity)
    size_t ev_used = 0;                 // profiling: events used by this call, algorithmic bytes of each bracketed launch
    std::vector<double> ev_bytes;
    int64_t nlaunch = 0;
    // Gathered rows (sweep.hip.h, gather_body): two-group streaming schedule + per-candidate sample orders.  The rows of batch
    // t + 1 of group g are gathered by the launch that carries chain(g, t) (t >= 1) — the launch BEFORE sweep(g, t), which stages
    // them as x_{t+1} and, a step later, as x_t; batches 0 and 1 are gathered by the group's forward-only prologue launch.
    int64_t Tcur = 0;
    bool use_gather = false;
    int64_t g_par_stride = 0, g_cand_stride = 0;
    std::vector<uint32_t> aborts;       // abort word of every epoch's resident launch
    int elt() const { return train->dtype == MFAS_DT_F32 ? 4 : 2; }
};

static hipError_t init_args(TrainCall& c) {     // (again after persist_fallback: the population's buffers and layout have changed)
    mfas_population* p = c.p;
    const LayoutPlan& pl = p->plan;
    const int K = p->K;
    StepArgs& st = c.st;
    c.NG = (int)pl.groups.size();
    Geo g = pl.g;
    g.order_stride = (p->hp.order_per_candidate && c.order) ? (int64_t)c.epochs * c.N : 0;    // order: [K][epochs][N_train]
    memset(&st, 0, sizeof(st));
    st.sa.cands = p->d_cands; st.sa.plane = p->plane; st.sa.plane_stride = pl.plane_stride; st.sa.wt = p->wt;
    st.sa.stepbuf = p->stepbuf; st.sa.tab = *c.train; st.sa.order = c.order; st.sa.g = g; st.sa.ac = c.ac;
    st.ca.plane = p->plane; st.ca.plane_stride = pl.plane_stride; st.ca.wt = p->wt; st.ca.stepbuf = p->stepbuf;
    st.ca.tab = *c.train; st.ca.order = c.order; st.ca.E = c.epochs; st.ca.g = g; st.ca.stats = p->d_stats;
    st.ca.status = p->d_status; st.ca.ac = c.ac; st.ca.yf_in_lds = pl.yf_in_lds ? 1 : 0; st.ca.pos_w = p->d_posw;
    st.ca.vec_in_lds = pl.vec_in_lds ? 1 : 0;
    st.sa.red_cnt = pl.red_in_sweep ? p->d_red_cnt : nullptr;
    st.ca.yf_reduced = pl.red_in_sweep ? 1 : 0;
    hipError_t e_ = hipSuccess;
    if (pl.red_in_sweep) e_ = hipMemsetAsync(p->d_red_cnt, 0, sizeof(uint32_t) * K * MFAS_MAX_CELLS, p->stream);
    if (e_ == hipSuccess && pl.same_group) e_ = hipMemsetAsync(p->d_cellflag, 0, sizeof(uint32_t) * K * CELLFLAG_STRIDE, p->stream);
    // chain_split: every piece of both parities "not written" (all-ones words), parity counter back to 0
    if (e_ == hipSuccess && pl.chain_split) e_ = hipMemsetAsync(p->d_xch, 0xFF, sizeof(float) * (size_t)K * XCH_CAND_FLOATS, p->stream);
    st.ca.xch = p->d_xch; st.ca.nsplit = pl.chain_split; st.ca.xpar = 0;
    c.split_launches[0] = c.split_launches[1] = 0;
    return e_;
}

// chain_split in the same-group launch counts ARRIVALS on the per-cell flags: every part adds 1 per step and a sweep unit waits for
// parts * (gstep + 1).  init_args zeroes the flags, which is right for a call that starts at step 0; one that starts at epoch `ep`
// (a later segment of a schedule, or the launch-per-phase layout taking over mid-call) starts them where steps 0 .. ep * nb - 1
// would have left them.  (The one-part chain stores its target and needs nothing.)
static hipError_t seed_cellflags(TrainCall& c, int64_t ep) {
    mfas_population* p = c.p;
    if (ep <= 0 || !p->plan.same_group || !p->plan.chain_split) return hipSuccess;
    return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->d_cellflag), (int)((uint32_t)p->plan.chain_split * (uint32_t)(ep * c.nb)),
                             (size_t)p->K * CELLFLAG_STRIDE, p->stream);
}

static hipError_t setup_gather(TrainCall& c) {
    mfas_population* p = c.p;
    const Geo& g = c.st.sa.g;
    c.use_gather = c.NG == 2 && !p->plan.persist && c.order && g.order_stride > 0 && !p->tune.no_gather;
    if (!c.use_gather) return hipSuccess;
    int64_t totw = 0;
    for (int u = 0; u < MFAS_MAX_TAPS; ++u) totw += g.sw[u] + g.vw[u];
    c.g_par_stride = totw * g.Bp * c.elt();
    c.g_cand_stride = 2 * c.g_par_stride;
    const size_t need = (size_t)c.g_cand_stride * p->K;
    if (p->gather_cap < need) {
        hipFree(p->d_gather); p->d_gather = nullptr; p->gather_cap = 0;
        hipError_t e = hipMalloc(&p->d_gather, need);
        if (e != hipSuccess) { c.use_gather = false; (void)hipGetLastError(); return hipSuccess; }   // an optimisation: train without it
        p->gather_cap = need;
    }
    if (p->tune.gather_verbose) fprintf(stderr, "[gather] on: %d candidates, %.1f MB of gathered rows\n", p->K, (double)need / 1e6);
    return hipSuccess;
}

// HIP events around one profiled launch (the pairs are kept in the population and reused by later calls)
struct ProfBracket {
    TrainCall& c;
    const bool on;
    const double bytes;             // algorithmic HBM bytes of the launch
    ProfBracket(TrainCall& c_, bool on_, double bytes_) : c(c_), on(on_), bytes(bytes_) {
        if (!on) return;
        mfas_population* p = c.p;
        if (p->ev.size() < c.ev_used + 2) {
            hipEvent_t e0, e1;
            hipEventCreate(&e0); hipEventCreate(&e1);
            p->ev.push_back(e0); p->ev.push_back(e1);
        }
        hipEventRecord(p->ev[c.ev_used], p->stream);
    }
    ~ProfBracket() {
        if (!on) return;
        hipEventRecord(c.p->ev[c.ev_used + 1], c.p->stream);
        c.ev_used += 2;
        c.ev_bytes.push_back(bytes);
    }
};

// one fused launch: sweep of group gs at step ts (gs < 0: none) + chain of group gc at step tc (gc < 0: none)
static void step(TrainCall& c, int gs, int upd, int fwd, int64_t ep, int64_t ts, int gc, int64_t tc) {
    mfas_population* p = c.p;
    const LayoutPlan& pl = p->plan;
    StepArgs& st = c.st;
    const int64_t N = c.N, nb = c.nb;
    const int B = c.B, MB = pl.g.MB;
    auto gather_set = [&](GatherArgs& ga, int s, int64_t t) {
        ga.pos[s] = ep * N + t * B; ga.base[s] = (int)(t * B);
        ga.nvalid[s] = (int)std::min<int64_t>(B, N - t * B); ga.par[s] = (int)(t & 1);
    };
    unsigned nsw = 0, nch = 0;
    st.ga.nblocks = 0; st.ga.nsets = 0; st.sa.gather = nullptr;
    if (c.use_gather) {
        GatherArgs& ga = st.ga;
        ga.buf = p->d_gather; ga.cand_stride = c.g_cand_stride; ga.par_stride = c.g_par_stride;
        int gg = -1;
        if (gs >= 0 && !upd && fwd && ts == 0) {                    // prologue of group gs: batches 0 and 1
            gg = gs;
            gather_set(ga, 0, 0); ga.nsets = 1;
            if (c.Tcur > 1) { gather_set(ga, 1, 1); ga.nsets = 2; }
        } else if (gc >= 0 && gs >= 0 && tc >= 1 && tc + 1 < c.Tcur) { // chain(gc, tc) rides with a sweep: batch tc + 1 of group gc
            gg = gc;
            gather_set(ga, 0, tc + 1); ga.nsets = 1;
        }
        if (gg >= 0) { ga.cands = p->d_cands + pl.groups[gg].c0; ga.nblocks = pl.groups[gg].nc; }
        if (gs >= 0 && upd) {
            st.sa.gather = p->d_gather; st.sa.g_cand_stride = c.g_cand_stride; st.sa.g_par_stride = c.g_par_stride;
            st.sa.g_par_t = (int)(ts & 1); st.sa.g_par_n = (int)((ts + 1) & 1);
        }
    }
    if (gs >= 0) {
        SweepArgs& s = st.sa;
        s.desc = p->groups[gs].d_descs;
        s.tdesc = p->groups[gs].d_taps; s.ntap = (int)pl.groups[gs].taps.size();
        s.do_update = upd; s.do_forward = fwd;
        s.pos_t = ep * N + ts * B; s.base_t = (int)(ts * B);
        s.nvalid_t = (int)std::min<int64_t>(B, N - ts * B);
        const int64_t tn = fwd ? (upd ? ts + 1 : ts) : ts;
        s.pos_n = ep * N + tn * B; s.base_n = (int)(tn * B);
        s.nvalid_n = (int)std::min<int64_t>(B, N - tn * B);
        const int64_t gstep = ep * nb + ts;
        s.ac.ss = upd ? c.step_scalars[2 * gstep] : 0.f;
        s.ac.bc2s = upd ? c.step_scalars[2 * gstep + 1] : 1.f;
        nsw = (unsigned)(pl.groups[gs].descs.size() + pl.groups[gs].taps.size());
    }
    if (gc >= 0) {
        ChainArgs& ca = st.ca;
        ca.cands = p->d_cands + pl.groups[gc].c0;
        ca.pos_t = ep * N + tc * B; ca.base_t = (int)(tc * B);
        ca.nvalid = (int)std::min<int64_t>(B, N - tc * B);
        const int64_t gstep = ep * nb + tc;
        ca.gstep = (int)gstep; ca.epoch = (int)ep;
        ca.ac.ss = c.step_scalars[2 * gstep]; ca.ac.bc2s = c.step_scalars[2 * gstep + 1];
        nch = (unsigned)pl.groups[gc].nc;
    }
    st.nchain = (int)nch;
    if (gs < 0) { st.sa.ntap = 0; }
    if (nsw == 0) {   // chain only: the latency-tuned standalone kernel (wide populations: theirs)
        launch(pl.wide ? wide_chain_kernel() : chain_kernel(MB, pl.lean_chain), nch, pl.lds_chain, p->stream, st.ca);
        return;
    }
    // algorithmic HBM bytes of this group's update+forward sweep: 24 B/param + the batch's taps + labels
    ProfBracket prof(c, p->profiling && gs >= 0 && upd && fwd && ((c.nlaunch++ % p->prof_every) == 0),
                     pl.groups[gs].alg_state + pl.groups[gs].alg_feat * c.elt() + 8.0 * B * pl.groups[gs].nc);
    if (pl.wide) {    // launch per phase only: the sweep of the one group, after its chain's launch
        launch(wide_sweep_kernel(pl.nontemporal), nsw, pl.lds_step, p->stream, st);
        return;
    }
    const bool same = pl.same_group && gc == gs && upd;      // chain(g, t) and sweep(g, t) in ONE launch, per-cell flags
    const bool split = pl.chain_split && nch > 0;            // the chain blocks are chain_split parts (two-group launch: no flags, the kernel boundary)
    if (split) {      // NS parts per candidate, chain blocks = NS * ceil8(candidates)
        st.ca.ncand = (int)nch; st.ca.xpar = (int)(c.split_launches[gc & 1]++ & 1);
        st.nchain = pl.chain_split * (int)((nch + 7) & ~7u);
    }
    if (same) {       // (NS parts: the per-cell flags count arrivals)
        st.sa.cellflag = p->d_cellflag; st.ca.cellflag = p->d_cellflag;
        st.sa.flag_target = st.ca.flag_target = (split ? (uint32_t)pl.chain_split : 1u) * ((uint32_t)st.ca.gstep + 1u);
        st.sa.flag_status = p->d_status;
    }
    // MB == 2: the two-workgroups-per-CU build unless a co-scheduled chain would bound the launch (see SweepU)
    // (lean chain: the 128-VGPR build spills 8 registers of the element-parallel chain to scratch and is still the faster
    //  one — R=16, B=20, 50 / 128 / 512 candidates: 47.2 / 99.2 / 418 us per step against 50.5 / 117.4 / 447 for the 2-workgroup build)
    const bool occ = nch == 0 || pl.groups[gs].alg_state > pl.occ_bytes;
    const int wpe = MB == 1 || (MB == 2 && (occ || pl.lean_chain)) ? 4 : 2;
    const StepKernel k = same ? same_kernel(MB, pl.nontemporal, split ? pl.chain_split : 1)
                       : split ? step_kernel(MB, pl.nontemporal, 4, false, pl.chain_split) : step_kernel(MB, pl.nontemporal, wpe, pl.lean_chain, 1);
    launch(k, (unsigned)st.nchain + st.ga.nblocks + nsw, split ? pl.lds_split : pl.lds_step, p->stream, st);
    if (same) { st.sa.cellflag = nullptr; st.ca.cellflag = nullptr; }
}

// one persistent launch = all train steps of one epoch (persist.hip.h)
static hipError_t persist_epoch_once(TrainCall& c, int ep, int64_t T) {
    mfas_population* p = c.p;
    const LayoutPlan& pl = p->plan;
    const Geo& g = pl.g;
    const int K = p->K;
    // (test_not_resident: -1 in the product library; the MFAS_TEST_HOOKS variant: from this epoch on every roll call "fails" — nothing is launched)
    if (p->tune.test_not_resident >= 0 && ep >= p->tune.test_not_resident) { c.aborts[ep] = PERSIST_ABORT_NOT_RESIDENT; return hipSuccess; }
    hipError_t e = hipMemsetAsync(p->d_sync, 0, sizeof(uint32_t) * ((size_t)K * PERSIST_SYNC_STRIDE + 64), p->stream);
    if (e != hipSuccess) return e;
    PersistArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.sa = c.st.sa; pa.ca = c.st.ca;
    pa.sa.desc = p->d_pdescs; pa.sa.tdesc = nullptr; pa.sa.ntap = 0;
    pa.ca.cands = p->d_cands;
    pa.nchain = K; pa.nitems = (int)pl.pdescs.size(); pa.nres = pl.nres; pa.res_chain = pl.res_chain ? 1 : 0; pa.res_wide = pl.res_wide ? 1 : 0;
    pa.res_nu = pl.res_nu; pa.nres_wg = pl.nres_wg; pa.res_buf_words = pl.res_buf_words;
    pa.T = (int)T; pa.epoch = ep;
    pa.lose_step = p->tune.test_lose_step;
    pa.N = c.N; pa.pos0 = (int64_t)ep * c.N;
    pa.B = c.B; pa.gstep0 = (int)((int64_t)ep * c.nb);
    pa.scal = p->d_scal; pa.sync = p->d_sync; pa.need = p->d_need; pa.role = p->d_role; pa.trace = p->d_trace;
    const unsigned grid = (unsigned)(K + pa.nres_wg);
    if ((int)grid > p->n_cus) return hipErrorInvalidConfiguration;
    {
        // algorithmic bytes of the launch: T update+forward sweeps of every candidate
        ProfBracket prof(c, p->profiling, (double)T * (pl.groups[0].alg_state + pl.groups[0].alg_feat * c.elt() + 8.0 * c.B * K));
        const int lw = (int)(pl.lds_president / 4) - PERSIST_LDS_WORDS;
        // the search default — no BatchNorm, no alphas, single-task softmax CE — runs the chain compiled for exactly that (chain_lean PLAIN)
        // (round 6: and `--batchnorm` alone, /root/reference/main_searchable_ntu.py:48, the chain compiled for exactly THAT — PLAIN = 2)
        const bool simple = !g.alphas && !g.multitask && g.loss_mode == 0 && !p->tune.no_plain_chain;
        const bool x16 = c.train->dtype != MFAS_DT_F32;
        launch(president_kernel(g.MB, x16, x16 && pl.res_wide, pl.res_nu, simple ? (g.bn ? 2 : 1) : 0), grid, pl.lds_president, p->stream, pa, lw);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(&c.aborts[ep], p->d_sync + (size_t)K * PERSIST_SYNC_STRIDE, sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream);
}

    // The launch is only valid when its whole grid is resident at once (roll call, persist.hip.h).  When another process holds
    // part of the GPU the roll call fails BEFORE anything is modified (abort code 2): wait a little (jittered, so that two
    // processes that collided do not collide again in lockstep) and launch the epoch again — up to PERSIST_MAX_RELAUNCHES times
    // (~0.3 s of trying); after that the caller gives the resident schedule up for this population (persist_fallback).
static hipError_t persist_epoch(TrainCall& c, int ep, int64_t T) {
    mfas_population* p = c.p;
    std::vector<uint32_t>& aborts = c.aborts;
    for (int attempt = 0;; ++attempt) {
        hipError_t e = persist_epoch_once(c, ep, T);
        if (e != hipSuccess) return e;
        e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) return e;
        if (p->tune.persist_verbose >= 2)
            fprintf(stderr, "[persist] epoch %d attempt %d: abort word %u\n", ep, attempt, aborts[ep]);
        if (aborts[ep] != PERSIST_ABORT_NOT_RESIDENT || attempt >= PERSIST_MAX_RELAUNCHES || p->tune.test_not_resident >= 0) {
            if (attempt && p->tune.persist_verbose) fprintf(stderr, "[persist] epoch %d: grid not resident at once, relaunched %d time(s)\n", ep, attempt);
            return hipSuccess;
        }
        if (p->profiling && c.ev_used >= 2) { c.ev_used -= 2; c.ev_bytes.pop_back(); }       // the failed attempt is not a measurement
        aborts[ep] = 0;
        std::this_thread::sleep_for(std::chrono::microseconds(200 + (uint64_t)((reinterpret_cast<uintptr_t>(p) >> 6) * 2654435761u % 1800u) + 50u * (attempt % 16)));
    }
}

// MFAS_PERSIST_TRACE: the step-phase timestamps of the last resident launch
static void dump_persist_trace(const mfas_population* p) {
    unsigned long long tr[256];
    if (hipMemcpy(tr, p->d_trace, sizeof(tr), hipMemcpyDeviceToHost) != hipSuccess) return;
    // step 12 of candidate 0: chain published at tr[4*8+3]; per resident unit: saw-flag / compute-done / arrived, relative to it
    const long long pub = (long long)tr[4 * 8 + 3];
    fprintf(stderr, "[persist trace step 12, candidate 0 units, ticks after the chain published: saw-flag done arrived]");
    for (int u = 0; u < 64; ++u)
        if (tr[64 + u]) fprintf(stderr, " u%d:%lld/%lld/%lld", u, (long long)tr[64 + u] - pub, (long long)tr[128 + u] - pub, (long long)tr[192 + u] - pub);
    fprintf(stderr, "\n[chain ready for step 13 at +%lld]\n", (long long)tr[5 * 8 + 1] - pub);
    fprintf(stderr, "[persist trace, 10 ns ticks; per step: chain wait0 ready done published | sweep-unit-0 wait0 ready done arrived]\n");
    for (int t = 0; t < 8; ++t) {
        fprintf(stderr, "  step %2d:", t + 8);
        for (int j = 0; j < 8; ++j) fprintf(stderr, " %lld", (long long)(tr[t * 8 + j] - tr[0]));
        fprintf(stderr, "\n");
    }
}

#ifdef MFAS_CHAIN_TIMING
static void dump_chain_timing(const mfas_population* p) {
    int32_t ts[40];
    if (hipMemcpy(ts, p->d_status + 64, sizeof(ts), hipMemcpyDeviceToHost) != hipSuccess) return;
    fprintf(stderr, "[chain timing, shader cycles since kernel entry, candidate 0 step 3]");
    for (int i = 0; i < 13; ++i) fprintf(stderr, " %d", ts[i]);
    if (p->plan.chain_split) {      // chain_split's extra stamps: forward cell 1 product done | out sent | tail done | fetched;  backward cell 2 the same;  softmax done;  entry staged
        fprintf(stderr, "  | split:");
        for (int i = 13; i < 23; ++i) fprintf(stderr, " %d", ts[i]);
        fprintf(stderr, "  | entry: record here %d, slabs summed %d, vector block in LDS %d", ts[34], ts[35], ts[36]);
        fprintf(stderr, "  | 10 ns ticks: chain of step 3 %d, end of chain 3 -> entry of chain 4 %d, chain of step 4 %d", ts[24] - ts[23], ts[25] - ts[24], ts[26] - ts[25]);
        fprintf(stderr, "; end of chain 3 -> first cell-0 unit sees its flag %d -> last sweep unit of the launch ends %d -> entry of chain 4 %d", (int32_t)((uint32_t)ts[28] - (uint32_t)ts[24]), (int32_t)((uint32_t)ts[27] - (uint32_t)ts[28]), (int32_t)((uint32_t)ts[25] - (uint32_t)ts[27]));
        fprintf(stderr, "; unit (cell 0, S, chunk 0) after the end of chain 3: flag seen %d, dy staged %d, tiles done %d, slab drained %d, arrival counted %d",
                ts[29] - ts[24], ts[30] - ts[24], ts[31] - ts[24], ts[32] - ts[24], ts[33] - ts[24]);
        int32_t ue[16];
        if (hipMemcpy(ue, p->d_status + 128, sizeof(ue), hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "; last unit end after the end of chain 3, per cell [S V OUT HEAD]:");
            for (int i = 0; i < 16; ++i) fprintf(stderr, "%s%d", (i & 3) ? " " : " | ", ue[i] ? (int32_t)((uint32_t)ue[i] - (uint32_t)ts[24]) : 0);
        }
    }
    fprintf(stderr, "\n");
    int32_t cs[24];
    if (hipMemcpy(cs, p->d_status + 96, sizeof(cs), hipMemcpyDeviceToHost) == hipSuccess) {
        fprintf(stderr, "[chain checksums, candidate 0 global step 0: sums x4, out x4, logits, dlogits, dy x4, d x4]");
        for (int i = 0; i < 18; ++i) fprintf(stderr, " %08x", (unsigned)cs[i]);
        fprintf(stderr, "\n");
    }
}
#endif

// The loop of mfas_population_train and mfas_population_train_from: epochs [first, last) of a schedule of `epochs` epochs.
// segment = false is mfas_population_train (first = 0, last = epochs, the record is reset); segment = true keeps the progress record,
// and with first > 0 goes on from the state the previous segment left instead of from a fresh optimizer.
static int train_impl(mfas_population* p, const mfas_table* train, const mfas_table* dev, const int32_t* order, const float* step_scalars,
                      int32_t epochs, int64_t max_steps, int32_t snapshot_best, mfas_epoch_stats* stats, int32_t* status,
                      const int32_t first, const int32_t last, const bool segment) {
    if (!p || !step_scalars || epochs <= 0 || !stats) return fail(MFAS_EINVAL, "bad argument");
    if (first < 0 || last <= first || last > epochs)
        return fail(MFAS_EINVAL, "train_from: epochs [" + std::to_string(first) + ", " + std::to_string(last) + ") are no segment of a schedule of " + std::to_string(epochs));
    int rc = check_table(p, train, p->plan.g.multitask);
    if (rc) return rc;
    const bool do_dev = max_steps < 0;
    if (do_dev) { rc = check_table(p, dev, p->plan.g.multitask); if (rc) return rc; }
    HIPCHK(hipSetDevice(p->device));
    const Geo& g = p->plan.g;
    const int K = p->K, B = g.B;
    const int64_t N = train->N;
    const int64_t nb = (N + B - 1) / B;
    if (p->plan.persist && p->plan.nres > 0 && p->hp.tap_bits == 16 && train->dtype == MFAS_DT_F32)
        return fail(MFAS_EINVAL, "this population was created for 16-bit feature tables (mfas_hyper.tap_bits = 16); f32 tables need tap_bits = 32 or 0");
    if (N - (nb - 1) * B == 1 && g.bn)   // torch BatchNorm1d raises on a size-1 train batch
        return fail(MFAS_EINVAL, "final train batch of size 1 with batchnorm (reference raises ValueError)");
    const bool resume = first > 0;
    if (resume)      // nothing has been touched yet: a refused segment leaves the population as it was
        for (int k = 0; k < K; ++k) {
            const mfas_population::Progress& pr = p->prog;
            if (pr.done[k] != first || pr.nb[k] != nb)
                return fail(MFAS_EINVAL, "train_from: first_epoch = " + std::to_string(first) + " of a schedule with " + std::to_string(nb) +
                                         " batches per epoch, but candidate " + std::to_string(k) + "'s progress record says " + std::to_string(pr.done[k]) +
                                         " epoch(s) complete of a schedule with " + std::to_string(pr.nb[k]) + " batches per epoch");
            if ((pr.keeps_best[k] != 0) != (snapshot_best != 0) || (snapshot_best && !p->best))
                return fail(MFAS_EINVAL, "train_from: snapshot_best = " + std::to_string(snapshot_best != 0) + " at first_epoch = " + std::to_string(first) +
                                         ", but candidate " + std::to_string(k) + "'s schedule was started with snapshot_best = " + std::to_string(pr.keeps_best[k]));
        }
    if (!segment) p->prog.reset(K, p->best_threshold);      // a plain train() call owes nothing to an earlier schedule

    if (p->stats_cap < K * epochs) {
        hipFree(p->d_stats); p->d_stats = nullptr;
        HIPCHK(hipMalloc(&p->d_stats, sizeof(DevStats) * K * epochs));
        p->stats_cap = K * epochs;
    }
    HIPCHK(hipMemsetAsync(p->d_stats, 0, sizeof(DevStats) * K * epochs, p->stream));
    if (!resume) HIPCHK(hipMemsetAsync(p->d_status, 0, sizeof(int32_t) * K, p->stream));      // (sticky across the segments of a schedule)
#ifdef MFAS_CHAIN_TIMING
    HIPCHK(hipMemsetAsync(p->d_status + 64 + 27, 0, sizeof(int32_t), p->stream));
    HIPCHK(hipMemsetAsync(p->d_status + 128, 0, 16 * sizeof(int32_t), p->stream));
    HIPCHK(hipMemsetAsync(p->d_status + 64 + 28, 0xFF, sizeof(int32_t), p->stream));
#endif
    // every call is a freshly built torch.optim.Adam (ntu_searchable.py:65; main_found_ntu.py:108,128): zero exp_avg / exp_avg_sq
    // (a segment that goes on finds the optimizer's state where the previous one left it)
    if (!resume) HIPCHK(hipMemsetAsync(p->plane + p->plan.plane_stride, 0, sizeof(float) * 2 * (size_t)p->plan.plane_stride, p->stream));
    if (snapshot_best && !p->best) HIPCHK(hipMalloc(&p->best, sizeof(float) * (size_t)p->plan.plane_stride));
    // best_model_sd starts as a copy of the INITIAL state_dict (train_searchable/ntu.py:17) and is what the model is
    // left with if no epoch's dev metric beats the starting threshold (0 for accuracy, init_f1 for F1)
    if (snapshot_best && max_steps < 0 && !resume)
        HIPCHK(hipMemcpyAsync(p->best, p->plane, sizeof(float) * (size_t)p->plan.plane_stride, hipMemcpyDeviceToDevice, p->stream));
    std::vector<double> best_acc(K, p->best_threshold);
    if (resume) best_acc = p->prog.best_metric;
    const double metric_scale = g.loss_mode == 1 ? 1.0 / 4294967296.0 : 1.0;   // F1 sums are 32.32 fixed point
    std::vector<DevStats> hstats((size_t)K * epochs);

    RangeGuard call_range("mfas_population_train K=" + std::to_string(K) + " R=" + std::to_string(g.R) + " B=" + std::to_string(B) +
                          " E=" + std::to_string(epochs) + (p->plan.persist ? " resident" : " launch-per-phase"));
    const mfas_hyper& hp = p->hp;
    TrainCall c;
    c.p = p; c.train = train; c.order = order; c.step_scalars = step_scalars; c.epochs = epochs; c.B = B; c.N = N; c.nb = nb;
    c.ac.w1 = (float)(1.0 - hp.beta1); c.ac.b2 = (float)hp.beta2; c.ac.w2 = (float)(1.0 - hp.beta2);
    c.ac.eps = (float)hp.adam_eps; c.ac.wd = (float)hp.wd; c.ac.ss = 0.f; c.ac.bc2s = 1.f;
    c.aborts.assign(epochs, 0u);
    std::vector<uint32_t>& aborts = c.aborts;
    HIPCHK(init_args(c));
    HIPCHK(seed_cellflags(c, first));
    p->prof_launches = 0; p->prof_ms = 0.0; p->prof_bytes = 0.0;
    HIPCHK(setup_gather(c));
    if (p->plan.persist) {   // the step scalars live on the device: the kernel walks the steps itself
        const size_t nsc = (size_t)epochs * nb * 2;
        if (p->scal_cap < nsc) {
            hipFree(p->d_scal); p->d_scal = nullptr;
            HIPCHK(hipMalloc(&p->d_scal, sizeof(float) * nsc));
            p->scal_cap = nsc;
        }
        const size_t have = (size_t)(max_steps >= 0 ? std::min<int64_t>(max_steps, (int64_t)epochs * nb) : (int64_t)epochs * nb) * 2;
        HIPCHK(hipMemcpyAsync(p->d_scal, step_scalars, sizeof(float) * have, hipMemcpyHostToDevice, p->stream));
    }

    int64_t done = 0;   // train steps completed (max_steps bookkeeping)
    for (int ep = first; ep < last; ++ep) {
        int64_t T = nb;
        if (max_steps >= 0) T = std::min<int64_t>(nb, max_steps - done);
        if (T <= 0) break;
        c.Tcur = T;
        RangeGuard epoch_range("epoch " + std::to_string(ep));
        if (p->plan.persist) {
            HIPCHK(persist_epoch(c, ep, T));
            if (aborts[ep] == PERSIST_ABORT_NOT_RESIDENT) {
                // every attempt failed its roll call: nothing of this epoch has run.  Train it — and the rest — launch per phase.
                if (p->tune.persist_verbose) fprintf(stderr, "[persist] epoch %d: the resident grid never became resident; falling back to launch-per-phase\n", ep);
                rc = persist_fallback(p);
                if (rc) return rc;
                HIPCHK(init_args(c));
                HIPCHK(seed_cellflags(c, ep));
                HIPCHK(setup_gather(c));
                aborts[ep] = 0;
            } else if (aborts[ep]) {
                HIPCHK(hipStreamSynchronize(p->stream));
                return fail(MFAS_EHIP, "persistent step loop: a workgroup timed out waiting for its dependency (abort code 1: the epoch was "
                                       "abandoned half way, this population's parameters are not usable)");
            }
        }
        if (!p->plan.persist) {
            const int NG = c.NG;
            for (int gi = 0; gi < NG; ++gi) step(c, gi, 0, 1, ep, 0, -1, 0);   // prologue: forward sums of batch 0
            if (NG == 1 && p->plan.same_group) {
                for (int64_t t = 0; t < T; ++t) step(c, 0, 1, (t + 1 < T) ? 1 : 0, ep, t, 0, t);
            } else if (NG == 1) {
                for (int64_t t = 0; t < T; ++t) {
                    step(c, -1, 0, 0, ep, 0, 0, t);
                    step(c, 0, 1, (t + 1 < T) ? 1 : 0, ep, t, -1, 0);
                }
            } else {
                step(c, -1, 0, 0, ep, 0, 0, 0);   // chain(A, 0)
                for (int64_t t = 0; t < T; ++t) {
                    const int fwd = (t + 1 < T) ? 1 : 0;
                    step(c, 0, 1, fwd, ep, t, 1, t);                       // sweep(A, t)  ||  chain(B, t)
                    step(c, 1, 1, fwd, ep, t, fwd ? 0 : -1, t + 1);        // sweep(B, t)  ||  chain(A, t+1)
                }
            }
        }
        done += T;
        HIPCHK(hipGetLastError());
        if (do_dev) {
            EvalArgs ea;
            memset(&ea, 0, sizeof(ea));
            ea.cands = p->d_cands; ea.plane = p->plane; ea.tab = *dev; ea.row0 = 0; ea.nrows = dev->N;
            ea.cand0 = 0; ea.epoch = ep; ea.E = epochs; ea.g = c.st.sa.g; ea.stats = p->d_stats; ea.pos_w = p->d_posw;
            HIPCHK(launch_eval(p, ea, K, p->stream));
            if (snapshot_best) {
                HIPCHK(hipMemcpyAsync(hstats.data(), p->d_stats, sizeof(DevStats) * K * epochs, hipMemcpyDeviceToHost, p->stream));
                HIPCHK(hipStreamSynchronize(p->stream));
                for (int k = 0; k < K; ++k) {
                    const double acc = (double)hstats[(size_t)k * epochs + ep].dev_corr * metric_scale / (double)dev->N;
                    if (acc > best_acc[k]) {   // strict >, from 0 (train_searchable/ntu.py:82) / init_f1 (mmimdb.py:18)
                        best_acc[k] = acc;
                        HIPCHK(hipMemcpyAsync(p->best + p->plan.cand_plane_base[k], p->plane + p->plan.cand_plane_base[k],
                                              sizeof(float) * p->plan.cand_plane_size[k], hipMemcpyDeviceToDevice, p->stream));
                    }
                }
            }
        }
    }
    if (snapshot_best && do_dev && last == epochs) {   // model.load_state_dict(best_model_sd) (:86), unconditionally — once the schedule is complete
        HIPCHK(hipMemcpyAsync(p->plane, p->best, sizeof(float) * (size_t)p->plan.plane_stride, hipMemcpyDeviceToDevice, p->stream));
        // the transposed OUT / HEAD tiles the backward chain reads still hold the last epoch's weights: re-derive them
        PackArgs pa = pack_args(p, PK_WT, 0, nullptr);
        hipLaunchKernelGGL(k_pack, dim3((unsigned)p->plan.descs.size()), dim3(256), 0, p->stream, pa);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(hstats.data(), p->d_stats, sizeof(DevStats) * K * epochs, hipMemcpyDeviceToHost, p->stream));
    std::vector<int32_t> hstatus(K, 0);
    HIPCHK(hipMemcpyAsync(hstatus.data(), p->d_status, sizeof(int32_t) * K, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    for (uint32_t ab : aborts)
        if (ab) return fail(MFAS_EHIP, ab == PERSIST_ABORT_NOT_RESIDENT ? "persistent step loop: the grid never became resident (abort code 2)"
                                                                         : "persistent step loop: a workgroup timed out waiting for its dependency (abort code 1)");
    for (int32_t sv : hstatus)
        if (sv == 2) return fail(MFAS_EHIP, "same-group fused launch: a sweep unit timed out waiting for its cell's dy");
    if (p->d_trace && p->plan.persist) dump_persist_trace(p);
    for (size_t i = 0; i < hstats.size(); ++i) {
        stats[i].train_loss_sum = hstats[i].train_loss;
        stats[i].dev_loss_sum = hstats[i].dev_loss;
        stats[i].train_corrects = hstats[i].train_corr;
        stats[i].dev_corrects = hstats[i].dev_corr;
    }
    if (status) memcpy(status, hstatus.data(), sizeof(int32_t) * K);
    if (segment) {      // the record: where the schedule stands, and best_acc (train_searchable/ntu.py:18,82-83) so far
        for (int k = 0; k < K; ++k) {
            for (int ep = first; ep < last && !snapshot_best; ++ep)      // (snapshot_best has kept best_acc up to date epoch by epoch)
                best_acc[k] = std::max(best_acc[k], (double)hstats[(size_t)k * epochs + ep].dev_corr * metric_scale / (double)dev->N);
            p->prog.done[k] = last; p->prog.nb[k] = nb; p->prog.best_metric[k] = best_acc[k]; p->prog.keeps_best[k] = snapshot_best ? 1 : 0;
        }
    }
#ifdef MFAS_CHAIN_TIMING
    dump_chain_timing(p);
#endif
    if (p->profiling) {
        for (size_t i = 0; i + 1 < c.ev_used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p->ev[i], p->ev[i + 1]) == hipSuccess) {
                p->prof_ms += ms; p->prof_launches++; p->prof_bytes += c.ev_bytes[i / 2];
            }
        }
        p->bytes_per_launch = p->prof_launches ? p->prof_bytes / p->prof_launches : 0.0;
    }
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

// ------------------------------------------------------------------------------------------------
// Candidate state in and out of a population: single planes, the progress record, a whole candidate device to device
// ------------------------------------------------------------------------------------------------
// flat (state_dict order) -> one plane of candidate k of p; dst_plane / sel as in persist_fallback's move
static void put_plane(mfas_population* p, int k, float* dst_plane, int sel, int mode, bool with_wt, float* flat, hipStream_t st) {
    PackArgs b = pack_args(p, mode, sel, flat);
    b.plane = dst_plane;
    if (!with_wt) b.wt = nullptr;
    b.desc = p->d_descs + p->plan.desc_start[k];
    hipLaunchKernelGGL(k_pack, dim3(p->plan.desc_start[k + 1] - p->plan.desc_start[k]), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_vec, dim3(1), dim3(256), 0, st, b, k);
}

// the kept-best plane of a population that has none yet: every candidate's starts as a copy of its live parameters
static int ensure_best(mfas_population* p, hipStream_t st) {
    if (p->best) return MFAS_OK;
    HIPCHK(hipMalloc(&p->best, sizeof(float) * (size_t)p->plan.plane_stride));
    HIPCHK(hipMemcpyAsync(p->best, p->plane, sizeof(float) * (size_t)p->plan.plane_stride, hipMemcpyDeviceToDevice, st));
    return MFAS_OK;
}

extern "C" int mfas_population_set_state(mfas_population* p, int32_t k, int32_t plane, const float* flat) {
    if (!p || !flat || k < 0 || k >= p->K) return fail(MFAS_EINVAL, "bad argument");
    if (plane < 1 || plane > 3)
        return fail(MFAS_EINVAL, "set_state: plane " + std::to_string(plane) + " (1 = exp_avg, 2 = exp_avg_sq, 3 = kept best; plane 0 is mfas_population_set_params)");
    HIPCHK(hipSetDevice(p->device));
    if (plane == 3) {
        if (int rc = ensure_best(p, p->stream)) return rc;
        put_plane(p, k, p->best, 0, PK_PUT, false, const_cast<float*>(flat), p->stream);
        p->prog.keeps_best[k] = 1;
    } else put_plane(p, k, p->plane, plane, PK_PUT, false, const_cast<float*>(flat), p->stream);
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
        HIPCHK(hipMemcpyAsync(status, p->d_status + k, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
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
        HIPCHK(hipMemcpyAsync(p->d_status + k, status, sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));      // status is a host word
    }
    if (epochs_done) { p->prog.done[k] = *epochs_done; if (*epochs_done == 0) p->prog.keeps_best[k] = 0; }
    if (nb) p->prog.nb[k] = *nb;
    if (best_metric) p->prog.best_metric[k] = *best_metric;
    return MFAS_OK;
}

extern "C" int mfas_population_move(mfas_population* dst, int32_t kd, mfas_population* src, int32_t ks) {
    if (!dst || !src || kd < 0 || kd >= dst->K || ks < 0 || ks >= src->K) return fail(MFAS_EINVAL, "bad argument");
    if (dst->device != src->device) return fail(MFAS_EINVAL, "move: the two populations live on different devices");
    const mfas_hyper &hd = dst->hp, &hs = src->hp;
    if (hd.R != hs.R || hd.C != hs.C || (hd.bn != 0) != (hs.bn != 0) || (hd.alphas != 0) != (hs.alphas != 0) ||
        memcmp(hd.s_sizes, hs.s_sizes, sizeof(hd.s_sizes)) || memcmp(hd.v_sizes, hs.v_sizes, sizeof(hd.v_sizes)))
        return fail(MFAS_EINVAL, "move: the two populations' hyper-parameters (R, C, bn, alphas, tap widths) differ");
    const CandDev &cd = dst->plan.cands[kd], &cs = src->plan.cands[ks];
    bool same = cd.L == cs.L;
    for (int i = 0; same && i < cd.L; ++i)
        for (int j = 0; j < 3; ++j) same = same && cd.conf[i][j] == cs.conf[i][j];
    if (!same || dst->plan.nparams[kd] != src->plan.nparams[ks])
        return fail(MFAS_EINVAL, "move: candidate " + std::to_string(ks) + " of the source and slot " + std::to_string(kd) + " of the destination have different configurations");
    HIPCHK(hipSetDevice(dst->device));
    const int64_t n = src->plan.nparams[ks];
    if (dst->move_cap < n) {
        HIPCHK(hipStreamSynchronize(dst->stream));      // (an earlier move may still read the scratch)
        hipFree(dst->d_move); dst->d_move = nullptr; dst->move_cap = 0;
        HIPCHK(hipMalloc(&dst->d_move, sizeof(float) * (size_t)n));
        dst->move_cap = n;
    }
    const bool with_best = src->best && src->prog.keeps_best[ks];
    if (with_best) if (int rc = ensure_best(dst, dst->stream)) return rc;
    if (src->stream != dst->stream) HIPCHK(hipStreamSynchronize(src->stream));      // what src trained is in memory
    hipStream_t st = dst->stream;
    float* flat = dst->d_move;
    auto carry = [&](float* src_plane, int src_sel, float* dst_plane, int dst_sel, int mode, bool with_wt) {
        PackArgs a = pack_args(src, PK_GET, src_sel, flat);
        a.plane = src_plane;
        a.desc = src->d_descs + src->plan.desc_start[ks];
        hipMemsetAsync(flat, 0, sizeof(float) * (size_t)n, st);
        hipLaunchKernelGGL(k_pack, dim3(src->plan.desc_start[ks + 1] - src->plan.desc_start[ks]), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_vec, dim3(1), dim3(256), 0, st, a, ks);
        put_plane(dst, kd, dst_plane, dst_sel, mode, with_wt, flat, st);
    };
    carry(src->plane, 0, dst->plane, 0, PK_SET, true);          // W + BatchNorm running statistics (+ the transposed OUT / HEAD images); zeroes m / v
    carry(src->plane, 1, dst->plane, 1, PK_PUT, false);         // Adam first moment
    carry(src->plane, 2, dst->plane, 2, PK_PUT, false);         // Adam second moment
    if (with_best) carry(src->best, 0, dst->best, 0, PK_PUT, false);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst->d_status + kd, src->d_status + ks, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    dst->prog.done[kd] = src->prog.done[ks]; dst->prog.nb[kd] = src->prog.nb[ks];
    dst->prog.best_metric[kd] = src->prog.best_metric[ks]; dst->prog.keeps_best[kd] = with_best ? 1 : 0;
    return MFAS_OK;
}

extern "C" int mfas_population_forward(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0,
                                       int64_t nrows, float* logits, int64_t* corrects) {
    if (!p || k < 0 || k >= p->K || nrows <= 0 || row0 < 0) return fail(MFAS_EINVAL, "bad argument");
    int rc = check_table(p, tab, p->plan.g.multitask);
    if (rc) return rc;
    if (row0 + nrows > tab->N) return fail(MFAS_EINVAL, "row range outside the table");
    HIPCHK(hipSetDevice(p->device));
    EvalArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.cands = p->d_cands; ea.plane = p->plane; ea.tab = *tab; ea.row0 = row0; ea.nrows = nrows;
    ea.cand0 = k; ea.epoch = 0; ea.E = 1; ea.g = p->plan.g; ea.logits = logits; ea.pos_w = p->d_posw;
    if (corrects) {
        HIPCHK(hipMemsetAsync(p->d_corr, 0, sizeof(long long), p->stream));
        ea.corr_out = p->d_corr;
    }
    HIPCHK(launch_eval(p, ea, 1, p->stream));
    if (corrects) {
        long long h = 0;
        HIPCHK(hipMemcpyAsync(&h, p->d_corr, sizeof(long long), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        *corrects = (int64_t)h;
    }
    return MFAS_OK;
}

// One batch through candidate k in TRAIN mode: forward only (logits out), or forward + backward of an external loss
// (dlogits in): then every parameter's Adam first-moment slot receives its exact GRADIENT and nothing else changes — the step
// runs with beta1 = 0 (m <- m + 1 * (g - m) = g), weight decay 0 and learning rate 0 (w <- w - 0 * m / denom = w).
static int single_batch(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows, int32_t step_index,
                        float* logits, const float* dlogits) {
    if (!p || (!logits && !dlogits) || k < 0 || k >= p->K || row0 < 0) return fail(MFAS_EINVAL, "bad argument");
    int rc = check_table(p, tab, false);
    if (rc) return rc;
    const Geo& g = p->plan.g;
    if (nrows < 1 || nrows > g.B) return fail(MFAS_EINVAL, "train-mode forward: 1 <= rows <= the population's batch size");
    if (nrows == 1 && g.bn) return fail(MFAS_EINVAL, "train-mode BatchNorm needs more than 1 row (reference: ValueError)");
    if (row0 + nrows > tab->N) return fail(MFAS_EINVAL, "row range outside the table");
    HIPCHK(hipSetDevice(p->device));
    AdamC ac;
    ac.w1 = 1.0f; ac.b2 = (float)p->hp.beta2; ac.w2 = (float)(1.0 - p->hp.beta2); ac.eps = (float)p->hp.adam_eps; ac.wd = 0.f; ac.ss = 0.f; ac.bc2s = 1.f;
    StepArgs st;
    memset(&st, 0, sizeof(st));
    st.sa.cands = p->d_cands; st.sa.plane = p->plane; st.sa.plane_stride = p->plan.plane_stride; st.sa.wt = p->wt;
    st.sa.stepbuf = p->stepbuf; st.sa.tab = *tab; st.sa.order = nullptr; st.sa.g = g; st.sa.g.order_stride = 0;
    st.sa.desc = p->plan.wide ? p->groups[0].d_descs + p->plan.wide_start[k] : p->d_descs + p->plan.desc_start[k];
    st.sa.tdesc = nullptr; st.sa.ntap = 0;
    st.sa.do_update = 0; st.sa.do_forward = 1;
    st.sa.pos_n = row0; st.sa.base_n = (int)row0; st.sa.nvalid_n = nrows;
    st.sa.pos_t = row0; st.sa.base_t = (int)row0; st.sa.nvalid_t = nrows;
    st.sa.ac = ac;
    st.nchain = 0;
    const LayoutPlan& pl = p->plan;
    const unsigned nsw = pl.wide ? (unsigned)(pl.wide_start[k + 1] - pl.wide_start[k]) : (unsigned)(pl.desc_start[k + 1] - pl.desc_start[k]);
    size_t lds_need = pl.lds_step;   // (a population laid out for resident units budgets its streaming LDS without them)
    if (!pl.wide)
        for (int j = pl.desc_start[k]; j < pl.desc_start[k + 1]; ++j) lds_need = std::max(lds_need, sweep_unit_lds(g, pl.descs[j]));
    if (lds_need > 150 * 1024) return fail(MFAS_EINVAL, "train-mode forward: this population's units are too wide for the streaming kernels");
    const StepKernel sweep_k = pl.wide ? wide_sweep_kernel(false) : step_kernel(g.MB, false, g.MB == 1 ? 4 : 2, false, 1);
    if (lds_need > pl.lds_step) HIPCHK(set_lds(sweep_k, lds_need));
    auto sweep = [&]() { launch(sweep_k, nsw, lds_need, p->stream, st); };
    if (dlogits) {
        // The gradient lands in the first-moment slot as m <- m + 1 * (g - m): exact only from m = 0 (1 + (1e-9 - 1) cancels to 0),
        // and a stale second moment would turn the zero-step's 0 * (m / denom) into 0 * inf.  Whatever this handle has trained
        // before, candidate k's m and v planes start from zero here (the header documents them as scratch after this call).
        HIPCHK(hipMemsetAsync(p->plane + p->plan.plane_stride + p->plan.cand_plane_base[k], 0, sizeof(float) * (size_t)p->plan.cand_plane_size[k], p->stream));
        HIPCHK(hipMemsetAsync(p->plane + 2 * p->plan.plane_stride + p->plan.cand_plane_base[k], 0, sizeof(float) * (size_t)p->plan.cand_plane_size[k], p->stream));
    }
    // 1. forward partial sums of the batch (no update): the sweep's forward half over this candidate's units
    sweep();
    // 2. the chain: batch-statistics BN (running statistics move like in any train-mode forward), dropout stream of step_index;
    //    forward only: stops at the logits; backward: continues from the caller's dL/dlogits and leaves dy_i for the sweep
    ChainArgs& c = st.ca;
    c.cands = p->d_cands + k; c.plane = p->plane; c.plane_stride = p->plan.plane_stride; c.wt = p->wt; c.stepbuf = p->stepbuf;
    c.tab = *tab; c.order = nullptr; c.pos_t = row0; c.base_t = (int)row0; c.nvalid = nrows;
    c.gstep = step_index; c.epoch = 0; c.E = 1; c.g = st.sa.g; c.stats = nullptr; c.status = p->d_status;
    c.yf_in_lds = p->plan.yf_in_lds ? 1 : 0; c.vec_in_lds = p->plan.vec_in_lds ? 1 : 0; c.pos_w = p->d_posw;
    c.yf_reduced = 0; c.logits_out = dlogits ? nullptr : logits; c.dlogits_in = dlogits; c.ac = ac;
    launch(pl.wide ? wide_chain_kernel() : chain_kernel(g.MB, pl.lean_chain), 1u, pl.lds_chain, p->stream, st.ca);
    if (dlogits) {   // 3. dW of every matrix into its m slot (see the header comment); W, v-scaled-by-lr-0 steps leave W as it was
        st.sa.do_update = 1; st.sa.do_forward = 0;
        sweep();
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MFAS_OK;
}

extern "C" int mfas_population_forward_train(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows,
                                             int32_t step_index, float* logits) {
    if (!logits) return fail(MFAS_EINVAL, "bad argument");
    return single_batch(p, k, tab, row0, nrows, step_index, logits, nullptr);
}

extern "C" int mfas_population_backward(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows,
                                        int32_t step_index, const float* dlogits) {
    if (!dlogits) return fail(MFAS_EINVAL, "bad argument");
    return single_batch(p, k, tab, row0, nrows, step_index, nullptr, dlogits);
}

extern "C" int mfas_stream_probe(int64_t bytes_per_plane, int32_t iters, double* gb_per_s) {
    if (bytes_per_plane < (1 << 20) || iters < 1 || !gb_per_s) return fail(MFAS_EINVAL, "bad argument");
    const size_t plane = (size_t)bytes_per_plane / 1024 * 256;   // floats, whole tiles
    float* P = nullptr;
    HIPCHK(hipMalloc(&P, plane * 4 * 3));
    hipError_t e = hipMemset(P, 0, plane * 4 * 3);
    hipEvent_t a, b;
    if (e == hipSuccess) e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e != hipSuccess) { hipFree(P); return fail(MFAS_EHIP, hipGetErrorString(e)); }
    hipLaunchKernelGGL(k_stream_probe, dim3(2048), dim3(256), 0, 0, P, plane, plane / 256);
    hipEventRecord(a, 0);
    for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(k_stream_probe, dim3(2048), dim3(256), 0, 0, P, plane, plane / 256);
    hipEventRecord(b, 0);
    e = hipEventSynchronize(b);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b); hipFree(P);
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
    HIPCHK(hipMemcpy(p->d_posw, w, sizeof(float) * p->plan.g.C, hipMemcpyHostToDevice));
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

extern "C" int mfas_population_sweep_profile(const mfas_population* p, int64_t* launches, double* total_ms,
                                             double* bytes_per_launch) {
    if (!p) return fail(MFAS_EINVAL, "null");
    if (launches) *launches = p->prof_launches;
    if (total_ms) *total_ms = p->prof_ms;
    if (bytes_per_launch) *bytes_per_launch = p->bytes_per_launch;
    return MFAS_OK;
}
