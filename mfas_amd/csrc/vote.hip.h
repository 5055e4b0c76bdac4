// vote.hip.h — k_vote: the ensemble of M members' score rows (mfas_population_evaluate), and the host side of that call
// (part of the single translation unit mfas_hip.hip; see the header comment there and DESIGN.md §4)
#pragma once
// ------------------------------------------------------------------------------------------------
// k_vote — per table row: every member's decision, the weighted mean of the members' probabilities (combine 0) or the probability of
// the weighted mean score (combine 1), the ensemble's decision and loss.  Input: the logits k_eval wrote for a block of rows,
// [M][rows][C].  LPR lanes cooperate on a row (16 / 32 / 64 for C <= 64 / 128 / 256); lane j holds classes j, j + LPR, j + 2 LPR,
// j + 3 LPR, so a member's row is ONE coalesced pass (each logit is read exactly once) and the maximum and the sum are shuffle
// butterflies inside the lane group.  The member loop runs in list order with the mean accumulated in registers.
// No workgroup reads what another writes; the only atomics are 64-bit integer adds; the row losses go to a per-row buffer that
// k_vote_loss sums in a fixed order — so the outputs do not depend on the run, nor on how the rows were cut into blocks.
// ------------------------------------------------------------------------------------------------
struct VoteArgs {
    const float* logits;        // [M][rows][C] of this row block
    const float* weights;       // [M], normalised
    const int32_t* label;       // table columns (whole table: indexed by the global row)
    const float* vlogit;
    const float* slogit;
    const float* multilabel;
    const float* pos_w;
    int64_t row0, rows, N;      // first table row of the block, rows of the block, table rows (stride of member_preds)
    int32_t M, C, loss_mode, multitask, combine;
    float f1_th;
    int32_t* member_preds;      // optional [M][N]
    float* scores;              // optional (N, C)
    float* row_loss;            // [N]
    unsigned long long* corr;   // the ensemble's corrects (loss_mode 0) / 32.32 fixed-point F1 sum (loss_mode 1)
};

struct VoteOut {                // what the call copies back
    double loss;
    unsigned long long corr;
};

#define VOTE_NEG_INF (-__builtin_huge_valf())

// (value, class) maximum over the LPR lanes of a row: ties go to the LOWER class — the first maximum, as k_eval's serial loop takes it
template <int LPR>
__device__ __forceinline__ void vote_argmax(float& v, int& i) {
#pragma unroll
    for (int o = LPR >> 1; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}
template <int LPR>
__device__ __forceinline__ float vote_sum(float v) {
#pragma unroll
    for (int o = LPR >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);     // (a + b == b + a: every lane of the row ends with the same bits)
    return v;
}
// the lane's first maximum of its (up to) four classes; a NaN never wins a comparison (k_eval: `t > best`)
__device__ __forceinline__ void vote_lane_max(const float (&x)[4], const int (&cls)[4], float& v, int& i) {
    v = x[0] == x[0] ? x[0] : VOTE_NEG_INF; i = cls[0];
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (x[q] > v) { v = x[q]; i = cls[q]; }
}

template <int LPR>
__global__ void __launch_bounds__(256) k_vote(const VoteArgs a) {
    constexpr int RPB = 256 / LPR;                  // rows per workgroup
    const int tid = threadIdx.x, sub = tid & (LPR - 1), lane = tid & 63;
    const int64_t r = (int64_t)blockIdx.x * RPB + tid / LPR;
    const bool live = r < a.rows;
    const int64_t rc = live ? r : a.rows - 1;       // lane groups past the block's end redo its last row and write nothing
    const int64_t grow = a.row0 + rc;
    const int C = a.C, M = a.M;
    int cls[4];
    bool has[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { cls[q] = sub + LPR * q; has[q] = cls[q] < C; }
    const bool ce = a.loss_mode == 0;
    const bool need_max = ce && (a.combine == 0 || a.member_preds != nullptr);

    float vl[4], sl[4], acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] = 0.f;
        vl[q] = (ce && a.multitask && has[q]) ? a.vlogit[grow * C + cls[q]] : 0.f;
        sl[q] = (ce && a.multitask && has[q]) ? a.slogit[grow * C + cls[q]] : 0.f;
    }
    for (int m = 0; m < M; ++m) {
        const float* zr = a.logits + ((int64_t)m * a.rows + rc) * C;
        const float w = a.weights[m];
        float z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            z[q] = has[q] ? zr[cls[q]] : VOTE_NEG_INF;
            if (ce && a.multitask && has[q]) z[q] = (z[q] + vl[q]) + sl[q];     // what k_eval compares: sum(output), ntu.py:118
        }
        if (need_max) {
            float mx;
            int best;
            vote_lane_max(z, cls, mx, best);
            vote_argmax<LPR>(mx, best);
            const float z0 = __shfl(z[0], lane & ~(LPR - 1));       // k_eval starts at class 0, and nothing beats a NaN there
            if (a.member_preds && live && sub == 0) a.member_preds[(int64_t)m * a.N + grow] = z0 != z0 ? 0 : best;
            if (a.combine == 0) {
                float e[4], se = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) { e[q] = has[q] ? expf(z[q] - mx) : 0.f; se += e[q]; }
                se = vote_sum<LPR>(se);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += w * (e[q] / se);
            }
        } else if (!ce && a.combine == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += w * (has[q] ? 1.0f / (1.0f + expf(-z[q])) : 0.f);
        }
        if (a.combine == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += has[q] ? w * z[q] : 0.f;
        }
    }

    float loss = 0.f;
    unsigned long long corr = 0;
    if (ce) {
        if (a.combine == 1) {           // probability of the mean score
            float zb[4], mx;
            int bi;
#pragma unroll
            for (int q = 0; q < 4; ++q) zb[q] = has[q] ? acc[q] : VOTE_NEG_INF;
            vote_lane_max(zb, cls, mx, bi);
            vote_argmax<LPR>(mx, bi);
            float se = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) { acc[q] = has[q] ? expf(zb[q] - mx) : 0.f; se += acc[q]; }
            se = vote_sum<LPR>(se);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = acc[q] / se;
        }
        float pb[4], bv;
        int best;
#pragma unroll
        for (int q = 0; q < 4; ++q) pb[q] = has[q] ? acc[q] : VOTE_NEG_INF;
        vote_lane_max(pb, cls, bv, best);
        vote_argmax<LPR>(bv, best);
        const float p0 = __shfl(acc[0], lane & ~(LPR - 1));
        if (p0 != p0) best = 0;
        const int lab = a.label[grow];
        const int lq = lab / LPR;
        const float mine = lq == 0 ? acc[0] : (lq == 1 ? acc[1] : (lq == 2 ? acc[2] : acc[3]));
        const float pl = __shfl(mine, (lane & ~(LPR - 1)) + (lab & (LPR - 1)));
        const float tiny = 1.17549435e-38f;         // 2^-126
        loss = -logf(pl < tiny ? tiny : pl);
        corr = best == lab ? 1 : 0;
    } else {
        if (a.combine == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = 1.0f / (1.0f + expf(-acc[q]));
        }
        int cnt = 0;                    // tp | np << 10 | nt << 20 (each <= 256)
        float ls = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (has[q]) {
                const float t = a.multilabel[grow * C + cls[q]];
                const bool pr = acc[q] > a.f1_th, tr = t > 0.5f;
                cnt += ((pr && tr) ? 1 : 0) + (pr ? 1 << 10 : 0) + (tr ? 1 << 20 : 0);
                if (a.combine == 1) ls += a.pos_w[cls[q]] * t * -logf(acc[q]) + (1.0f - t) * -logf(1.0f - acc[q]);
            }
#pragma unroll
        for (int o = LPR >> 1; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        ls = vote_sum<LPR>(ls);
        loss = a.combine == 1 ? ls / (float)C : 0.f;     // (the mean of probabilities has no score to take the BCE of: reported as 0)
        const int tp = cnt & 1023, np = (cnt >> 10) & 1023, nt = cnt >> 20;
        corr = (np + nt) > 0 ? (((unsigned long long)(2 * tp)) << 32) / (unsigned long long)(np + nt) : 0;
    }
    if (a.scores && live) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (has[q]) a.scores[grow * C + cls[q]] = acc[q];
    }
    if (live && sub == 0) a.row_loss[grow] = loss;
    if (!(live && sub == 0)) corr = 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) corr += __shfl_xor(corr, o);
    if (lane == 0 && corr) atomicAdd(a.corr, corr);
}

// the row losses summed in ONE fixed order (a thread's rows in sequence, then a tree over the threads), in double
__global__ void __launch_bounds__(256) k_vote_loss(const float* row_loss, const int64_t N, double* out) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < N; i += 256) s += (double)row_loss[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid == 0) *out = part[0];
}

// ------------------------------------------------------------------------------------------------
// Host side of mfas_population_evaluate: every check first (a refused call changes nothing), then per row block one k_eval launch
// per member (ncand = 1, the path mfas_population_forward takes; its statistics go to the call's own slots) and one k_vote.
// Everything the call writes on the device lies in the population's evaluate arena (grow-only, read by nothing else) or in the
// caller's output buffers.  With any of confusion / rank_hist / label_counts (mfas_population_evaluate_report) every row block's
// k_vote is followed by one k_tally (tally.hip.h); with none of them the call launches, clears and allocates what it always did.
// ------------------------------------------------------------------------------------------------
static size_t vote_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// k_tally's launch for one row block (tally.hip.h): the per-class tallies of mfas_population_evaluate_report
static hipError_t tally_block(const VoteArgs& va, int64_t* confusion, int64_t* rank_hist, int64_t* label_counts, int lpr, hipStream_t st);

static int evaluate_impl(mfas_population* p, const mfas_table* tab, int32_t plane, const int32_t* members, const float* weights,
                         int32_t M, int32_t combine, int64_t scratch_bytes, mfas_epoch_stats* member_stats, int32_t* member_preds,
                         float* scores, mfas_epoch_stats* ensemble_stats, int64_t* confusion, int64_t* rank_hist, int64_t* label_counts) {
    if (!p) return fail(MFAS_EINVAL, "evaluate: null population");
    const Geo& g = p->plan.g;
    if (M <= 0) return fail(MFAS_EINVAL, "evaluate: M = " + std::to_string(M) + " members (at least one)");
    if (!members && M != p->K)
        return fail(MFAS_EINVAL, "evaluate: members == NULL means all " + std::to_string(p->K) + " candidates, but M = " + std::to_string(M));
    if (plane != 0 && plane != 3) return fail(MFAS_EINVAL, "evaluate: plane " + std::to_string(plane) + " (0 = live parameters, 3 = kept best)");
    if (combine != 0 && combine != 1)
        return fail(MFAS_EINVAL, "evaluate: combine " + std::to_string(combine) + " (0 = mean of probabilities, 1 = mean of scores)");
    if (scratch_bytes < 0) return fail(MFAS_EINVAL, "evaluate: scratch_bytes " + std::to_string(scratch_bytes) + " is negative");
    std::vector<int32_t> mem(M);
    for (int m = 0; m < M; ++m) {
        mem[m] = members ? members[m] : m;
        if (mem[m] < 0 || mem[m] >= p->K)
            return fail(MFAS_EINVAL, "evaluate: member " + std::to_string(m) + " is candidate " + std::to_string(mem[m]) + ", outside [0, " + std::to_string(p->K) + ")");
        if (plane == 3 && !(p->best && p->prog.keeps_best[mem[m]]))
            return fail(MFAS_EINVAL, "plane 3: candidate " + std::to_string(mem[m]) + " keeps no best-epoch parameters (no snapshot_best schedule in progress)");
    }
    std::vector<float> wn(M, (float)(1.0 / (double)M));
    if (weights) {
        double sum = 0.0;
        for (int m = 0; m < M; ++m) {
            if (!(weights[m] >= 0.0f) || !std::isfinite(weights[m]))
                return fail(MFAS_EINVAL, "evaluate: weight " + std::to_string(m) + " is " + std::to_string(weights[m]) + " (weights are finite and >= 0)");
            sum += (double)weights[m];
        }
        if (!(sum > 0.0) || !std::isfinite(sum)) return fail(MFAS_EINVAL, "evaluate: the weights sum to " + std::to_string(sum) + " (must be > 0)");
        for (int m = 0; m < M; ++m) wn[m] = (float)((double)weights[m] / sum);
    }
    if (member_preds && g.loss_mode == 1) return fail(MFAS_EINVAL, "evaluate: member_preds with loss_mode 1 (a multi-label member has no single decision)");
    if (confusion && g.loss_mode == 1) return fail(MFAS_EINVAL, "evaluate: confusion with loss_mode 1 (a multi-label member has no single decision)");
    if (rank_hist && g.loss_mode == 1) return fail(MFAS_EINVAL, "evaluate: rank_hist with loss_mode 1 (a multi-label row has no single label to rank)");
    if (label_counts && g.loss_mode == 0) return fail(MFAS_EINVAL, "evaluate: label_counts with loss_mode 0 (per-class positives belong to the multi-label head)");
    const bool report = confusion || rank_hist || label_counts;
    if (report && M >= 65535) return fail(MFAS_EINVAL, "evaluate: a report of M = " + std::to_string(M) + " members (at most 65534: one grid row per slot)");
    if (int rc = check_table(p, tab, g.multitask)) return rc;
    const int64_t N = tab->N, row_bytes = (int64_t)M * g.C * 4;
    if (scratch_bytes == 0) scratch_bytes = (int64_t)64 << 20;
    if (scratch_bytes < row_bytes)
        return fail(MFAS_EINVAL, "evaluate: scratch_bytes " + std::to_string(scratch_bytes) + " holds no row of " + std::to_string(M) + " members' logits (" +
                                     std::to_string(row_bytes) + " bytes)");
    // whole k_eval row tiles per block where the scratch allows: every tile then holds the rows it holds in the dev pass
    int64_t brows = std::min(N, scratch_bytes / row_bytes);
    if (brows < N && brows >= 64) brows &= ~(int64_t)63;
    const int lpr = g.C <= 64 ? 16 : (g.C <= 128 ? 32 : 64);
    if ((brows + 256 / lpr - 1) / (256 / lpr) > 0x7FFFFFFF) return fail(MFAS_EINVAL, "evaluate: too many rows in a block (lower scratch_bytes)");

    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = p->stream;
    // the arena: weights | member statistics | ensemble result | row losses | logits scratch | (a report without the caller's scores:) scores
    const size_t o_w = 0, o_st = o_w + vote_align(sizeof(float) * M), o_out = o_st + vote_align(sizeof(DevStats) * M),
                 o_rl = o_out + vote_align(sizeof(VoteOut)), o_lg = o_rl + vote_align(sizeof(float) * (size_t)N),
                 o_sc = o_lg + vote_align((size_t)brows * (size_t)row_bytes),
                 need = o_sc + ((report && !scores) ? vote_align(sizeof(float) * (size_t)N * (size_t)g.C) : 0);
    if (hipError_t e = p->d_vote.reserve(need))
        return fail(e == hipErrorOutOfMemory ? MFAS_ENOMEM : MFAS_EHIP, std::string("evaluate: arena: ") + hipGetErrorString(e));
    char* const arena = p->d_vote.get();
    float* d_w = reinterpret_cast<float*>(arena + o_w);
    DevStats* d_st = reinterpret_cast<DevStats*>(arena + o_st);
    VoteOut* d_out = reinterpret_cast<VoteOut*>(arena + o_out);
    float* d_rl = reinterpret_cast<float*>(arena + o_rl);
    float* d_lg = reinterpret_cast<float*>(arena + o_lg);
    HIPCHK(hipMemcpyAsync(d_w, wn.data(), sizeof(float) * M, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(arena + o_st, 0, o_rl - o_st, st));
    const size_t slots = (size_t)M + 1, nc = (size_t)g.C;
    if (confusion) HIPCHK(hipMemsetAsync(confusion, 0, sizeof(int64_t) * slots * nc * nc, st));
    if (rank_hist) HIPCHK(hipMemsetAsync(rank_hist, 0, sizeof(int64_t) * slots * nc, st));
    if (label_counts) HIPCHK(hipMemsetAsync(label_counts, 0, sizeof(int64_t) * slots * nc * 3, st));

    EvalArgs ea = eval_args(p, *tab, plane == 3 ? p->best.get() : p->plane.get(), g);
    VoteArgs va;
    memset(&va, 0, sizeof(va));
    va.logits = d_lg; va.weights = d_w; va.label = tab->label; va.vlogit = tab->vlogit; va.slogit = tab->slogit; va.multilabel = tab->multilabel;
    va.pos_w = p->d_posw.get(); va.N = N; va.M = M; va.C = g.C; va.loss_mode = g.loss_mode; va.multitask = g.multitask; va.combine = combine;
    va.f1_th = g.f1_th; va.member_preds = member_preds; va.scores = (report && !scores) ? reinterpret_cast<float*>(arena + o_sc) : scores; va.row_loss = d_rl; va.corr = &d_out->corr;
    for (int64_t row0 = 0; row0 < N; row0 += brows) {
        const int64_t rows = std::min(brows, N - row0);
        for (int m = 0; m < M; ++m) {
            ea.row0 = row0; ea.nrows = rows; ea.cand0 = mem[m];
            ea.epoch = m - mem[m];      // k_eval adds to stats[cand * E + epoch]: slot m of the call's own statistics
            ea.stats = d_st; ea.logits = d_lg + (size_t)m * (size_t)rows * g.C;
            HIPCHK(launch_eval(p, ea, 1, st));
        }
        va.row0 = row0; va.rows = rows;
        const unsigned grid = (unsigned)((rows + 256 / lpr - 1) / (256 / lpr));
        if (lpr == 16) hipLaunchKernelGGL(k_vote<16>, dim3(grid), dim3(256), 0, st, va);
        else if (lpr == 32) hipLaunchKernelGGL(k_vote<32>, dim3(grid), dim3(256), 0, st, va);
        else hipLaunchKernelGGL(k_vote<64>, dim3(grid), dim3(256), 0, st, va);
        HIPCHK(hipGetLastError());
        if (report) HIPCHK(tally_block(va, confusion, rank_hist, label_counts, lpr, st));
    }
    hipLaunchKernelGGL(k_vote_loss, dim3(1), dim3(256), 0, st, (const float*)d_rl, N, &d_out->loss);
    HIPCHK(hipGetLastError());
    std::vector<DevStats> hst(M);
    VoteOut hout;
    HIPCHK(hipMemcpyAsync(hst.data(), d_st, sizeof(DevStats) * M, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hout, d_out, sizeof(VoteOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (member_stats)
        for (int m = 0; m < M; ++m) {
            member_stats[m].train_loss_sum = 0.0; member_stats[m].train_corrects = 0;
            member_stats[m].dev_loss_sum = hst[m].dev_loss; member_stats[m].dev_corrects = hst[m].dev_corr;
        }
    if (ensemble_stats) {
        ensemble_stats->train_loss_sum = 0.0; ensemble_stats->train_corrects = 0;
        ensemble_stats->dev_loss_sum = hout.loss; ensemble_stats->dev_corrects = (int64_t)hout.corr;
    }
    return MFAS_OK;
}
