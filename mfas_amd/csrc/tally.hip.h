// tally.hip.h — k_tally: per-class tallies of an evaluate call (mfas_population_evaluate_report): the confusion matrix and the label's
// rank histogram (loss_mode 0), or per-class (true positives, predicted positives, actual positives) (loss_mode 1), for every member
// and for the ensemble  (part of the single translation unit mfas_hip.hip)
#pragma once
// ------------------------------------------------------------------------------------------------
// One launch per row block, after that block's k_vote.  Grid (row groups, M + 1): blockIdx.y is the SLOT — slots 0 .. M-1 are the
// members in list order, slot M is the ensemble.  256 threads, LPR lanes per row exactly as in k_vote; lane j holds classes j, j + LPR,
// j + 2 LPR, j + 3 LPR.  A workgroup strides over the rows of its slot, so its private tallies amortise.
//   score row   member: its logits row of the block (multitask: (z + vlogit) + slogit, in that order); ensemble: the row k_vote wrote
//               to `scores` (the caller's buffer, or an (N, C) area of the arena when the caller passed none).
//   decision    loss_mode 0: vote_lane_max + vote_argmax<LPR>, the functions k_vote calls, and k_vote's rule that a NaN in class 0
//               decides class 0: slot s decides row r as member_preds[s][r], bit for bit.
//               loss_mode 1, per class: member 1.0f / (1.0f + expf(-z)) > f1_th (k_eval's and k_vote's expression); ensemble
//               scores > f1_th; truth multilabel > 0.5f.
//   label rank  the number of classes that precede the label in the order "score descending, NaN last, equal scores by lower class
//               first".  Rank 0 coincides with "decided correctly" on every row whose class-0 score is not NaN.
//   sums        integers only.  The C-length tallies (rank histogram / 3 x C label counts) are workgroup-private int32 in LDS (the
//               label counts first in registers: a lane's classes never change), flushed once per workgroup, non-zero cells only, with
//               64-bit global atomic adds; a confusion cell takes one 64-bit global atomic add per live row (a workgroup-private
//               C x C LDS tile for C <= 64 measured the same within the run-to-run spread: profiles/evaluate_report.log).  No float
//               atomics, no workgroup reads what another writes: the outputs depend neither on the run nor on how the rows were cut
//               into blocks.
// A label outside [0, C) (the Python face refuses such a table) is tallied nowhere.
// ------------------------------------------------------------------------------------------------
struct TallyArgs {
    VoteArgs v;                 // the block's k_vote arguments; v.scores is never null here
    int64_t* confusion;         // optional [(M + 1)][C][C]
    int64_t* rank_hist;         // optional [(M + 1)][C]
    int64_t* label_counts;      // optional [(M + 1)][C][3]
};

__device__ __forceinline__ void tally_add(int64_t* p, int v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

template <int LPR>
__global__ void __launch_bounds__(256) k_tally(const TallyArgs t) {
    constexpr int RPB = 256 / LPR;                  // rows per pass of the workgroup
    __shared__ int cells[3 * 256];                  // rank histogram [C] / label counts [C][3]
    const VoteArgs& a = t.v;
    const int tid = threadIdx.x, sub = tid & (LPR - 1), lane = tid & 63, first = lane & ~(LPR - 1);
    const int C = a.C, slot = (int)blockIdx.y;
    const bool ens = slot == a.M, ce = a.loss_mode == 0;
    const int ncell = ce ? C : 3 * C;
    for (int i = tid; i < ncell; i += 256) cells[i] = 0;
    __syncthreads();
    int cls[4], tp[4], np[4], nt[4];
    bool has[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { cls[q] = sub + LPR * q; has[q] = cls[q] < C; tp[q] = np[q] = nt[q] = 0; }

    for (int64_t base = (int64_t)blockIdx.x * RPB; base < a.rows; base += (int64_t)gridDim.x * RPB) {      // (uniform over the workgroup)
        const int64_t r = base + tid / LPR;
        const bool live = r < a.rows;
        const int64_t rc = live ? r : a.rows - 1;   // lane groups past the block's end redo its last row and tally nothing
        const int64_t grow = a.row0 + rc;
        float x[4];
        if (ens) {
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = has[q] ? a.scores[grow * C + cls[q]] : VOTE_NEG_INF;
        } else {
            const float* zr = a.logits + ((int64_t)slot * a.rows + rc) * C;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] = has[q] ? zr[cls[q]] : VOTE_NEG_INF;
                if (ce && a.multitask && has[q]) x[q] = (x[q] + a.vlogit[grow * C + cls[q]]) + a.slogit[grow * C + cls[q]];
            }
        }
        if (ce) {
            float mx;
            int best;
            vote_lane_max(x, cls, mx, best);
            vote_argmax<LPR>(mx, best);
            const float x0 = __shfl(x[0], first);   // nothing beats a NaN in class 0 (k_vote, k_eval)
            if (x0 != x0) best = 0;
            const int lab = a.label[grow];
            const bool ok = live && (unsigned)lab < (unsigned)C;
            const int lq = lab / LPR;
            const float mine = lq == 0 ? x[0] : (lq == 1 ? x[1] : (lq == 2 ? x[2] : x[3]));
            const float xl = __shfl(mine, first + (lab & (LPR - 1)));
            int before = 0;                         // classes that precede the label
            if (t.rank_hist) {
                const bool lnan = xl != xl;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool lower = cls[q] < lab;
                    const bool p = lnan ? (x[q] == x[q] || lower) : (x[q] > xl || (x[q] == xl && lower));
                    before += (has[q] && p) ? 1 : 0;
                }
#pragma unroll
                for (int o = LPR >> 1; o > 0; o >>= 1) before += __shfl_xor(before, o);
            }
            if (ok && sub == 0) {
                if (t.rank_hist) atomicAdd(&cells[before], 1);
                if (t.confusion) tally_add(t.confusion + ((int64_t)slot * C + lab) * C + best, 1);
            }
        } else if (live) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (has[q]) {
                    const bool pr = ens ? x[q] > a.f1_th : 1.0f / (1.0f + expf(-x[q])) > a.f1_th;
                    const bool tr = a.multilabel[grow * C + cls[q]] > 0.5f;
                    tp[q] += (pr && tr) ? 1 : 0; np[q] += pr ? 1 : 0; nt[q] += tr ? 1 : 0;
                }
        }
    }
    if (!ce) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (has[q]) {
                if (tp[q]) atomicAdd(&cells[3 * cls[q] + 0], tp[q]);
                if (np[q]) atomicAdd(&cells[3 * cls[q] + 1], np[q]);
                if (nt[q]) atomicAdd(&cells[3 * cls[q] + 2], nt[q]);
            }
    }
    __syncthreads();
    int64_t* out = ce ? t.rank_hist : t.label_counts;
    if (out)
        for (int i = tid; i < ncell; i += 256)
            if (cells[i]) tally_add(out + (int64_t)slot * ncell + i, cells[i]);
}

// the launch of one row block (declared in vote.hip.h, where evaluate_impl calls it)
static hipError_t tally_block(const VoteArgs& va, int64_t* confusion, int64_t* rank_hist, int64_t* label_counts, int lpr, hipStream_t st) {
    TallyArgs ta;
    ta.v = va; ta.confusion = confusion; ta.rank_hist = rank_hist; ta.label_counts = label_counts;
    const int64_t groups = (va.rows + 256 / lpr - 1) / (256 / lpr);
    const dim3 grid((unsigned)((groups + 7) / 8), (unsigned)(va.M + 1));       // eight passes per workgroup where the block has them
    if (lpr == 16) hipLaunchKernelGGL(k_tally<16>, grid, dim3(256), 0, st, ta);
    else if (lpr == 32) hipLaunchKernelGGL(k_tally<32>, grid, dim3(256), 0, st, ta);
    else hipLaunchKernelGGL(k_tally<64>, grid, dim3(256), 0, st, ta);
    return hipGetLastError();
}
