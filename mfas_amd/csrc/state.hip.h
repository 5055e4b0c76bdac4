// state.hip.h — candidate state in and out of a population (host only, included by mfas_hip.hip): single planes through the reference's
// flat state_dict order, the one candidate carry built on them (mfas_population_move, persist_fallback), the construction draws.
#pragma once

static PackArgs pack_args(mfas_population* p, int mode, int plane, float* flat) {
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.desc = p->d_descs.get(); a.cands = p->d_cands.get(); a.plane = p->plane.get(); a.plane_stride = p->plan.plane_stride;
    a.wt = p->wt.get(); a.flat = flat; a.seeds = p->d_seeds.get(); a.mode = mode; a.sel_plane = plane; a.g = p->plan.g;
    return a;
}

// k_pack over candidate k's descriptors + k_vec for its vector block; k < 0: every candidate's (errors: hipGetLastError)
static void run_pack(mfas_population* p, PackArgs a, int k, bool vec, hipStream_t st) {
    const int d0 = k < 0 ? 0 : p->plan.desc_start[k], d1 = k < 0 ? (int)p->plan.descs.size() : p->plan.desc_start[k + 1];
    a.desc = p->d_descs.get() + d0;
    hipLaunchKernelGGL(k_pack, dim3((unsigned)(d1 - d0)), dim3(256), 0, st, a);
    if (vec) hipLaunchKernelGGL(k_vec, dim3(k < 0 ? p->K : 1), dim3(256), 0, st, a, k);
}

// one plane of candidate k -> flat (state_dict order).  plane_base / sel: p->plane with sel 0 / 1 / 2 = W / exp_avg / exp_avg_sq, or
// p->best with sel 0: the kept-best plane is "plane 0 of another base pointer" (a full image, BatchNorm running statistics included)
static hipError_t get_plane(mfas_population* p, int k, float* plane_base, int sel, float* flat, hipStream_t st) {
    hipError_t e = hipMemsetAsync(flat, 0, sizeof(float) * p->plan.nparams[k], st);
    if (e != hipSuccess) return e;
    PackArgs a = pack_args(p, PK_GET, sel, flat);
    a.plane = plane_base;
    run_pack(p, a, k, true, st);
    return hipSuccess;
}

// flat -> one plane of candidate k.  PK_SET (plane 0 of a live population): W, the transposed OUT / HEAD images (with_wt), zeroes m / v;
// PK_PUT: that plane alone
static void put_plane(mfas_population* p, int k, float* plane_base, int sel, int mode, bool with_wt, const float* flat, hipStream_t st) {
    PackArgs b = pack_args(p, mode, sel, const_cast<float*>(flat));
    b.plane = plane_base;
    if (!with_wt) b.wt = nullptr;
    run_pack(p, b, k, true, st);
}

// candidate ks of src -> slot kd of dst, device to device: W + BatchNorm running statistics, both Adam moments, and with_best the
// kept-best plane; `flat` holds one candidate, the copies are ordered by `st`.  Indifferent to the two layouts (chunk size, resident or
// not, wide or not).
static hipError_t carry_candidate(mfas_population* dst, int kd, mfas_population* src, int ks, bool with_best, float* flat, hipStream_t st) {
    for (int i = 0; i < (with_best ? 4 : 3); ++i) {     // W (PK_SET: + the transposed images, zeroes m / v), m, v, the kept best
        const int sel = i % 3;
        if (hipError_t e = get_plane(src, ks, i == 3 ? src->best.get() : src->plane.get(), sel, flat, st)) return e;
        put_plane(dst, kd, i == 3 ? dst->best.get() : dst->plane.get(), sel, i == 0 ? PK_SET : PK_PUT, i == 0, flat, st);
    }
    return hipGetLastError();
}

// The kept-best plane: allocated here and nowhere else, when a caller first needs it.  `init` = what it holds on return:
//   BEST_LIVE_IF_NEW  a new plane is a copy of the live parameters, an existing one keeps the other candidates' best: set_state of plane 3, the destination of a move
//   BEST_LIVE         a copy of the live parameters, new or not: train_begin of a schedule that starts with a dev pass (best_model_sd = the INITIAL state_dict)
//   BEST_AS_IS        a new plane as allocated, an existing one as it is: train_begin otherwise (a later segment goes on; without a dev pass nothing reads it)
//   BEST_ZERO         a new plane zeroed: persist_fallback's launch-per-phase record, before every candidate's is carried into it
enum BestInit { BEST_LIVE_IF_NEW, BEST_LIVE, BEST_AS_IS, BEST_ZERO };
static hipError_t keep_best(mfas_population* p, BestInit init, hipStream_t st) {
    const size_t n = (size_t)p->plan.plane_stride;
    const bool fresh = !p->best;
    if (fresh) if (hipError_t e = p->best.alloc(n)) return e;
    if (init == BEST_LIVE || (init == BEST_LIVE_IF_NEW && fresh)) return hipMemcpyAsync(p->best.get(), p->plane.get(), sizeof(float) * n, hipMemcpyDeviceToDevice, st);
    if (init == BEST_ZERO && fresh) return hipMemsetAsync(p->best.get(), 0, sizeof(float) * n, st);
    return hipSuccess;
}

// torch.manual_seed(seeds[k]) + the module's construction draws for every candidate, on the device (k_mt_uniform, pack.hip.h).
// bounds: per candidate 2 * (MFAS_MAX_CELLS + 1) floats — per cell {weight bound, bias bound}, then the classifier's — as the host
// computed them (kaiming_uniform_(a = sqrt 5) / 1 / sqrt(fan_in), nn.Linear.reset_parameters); alphas ~ N(alpha_mean, alpha_std)
// drawn LAST like Searchable_Skeleton_Image_Net.__init__ does (ntu_searchable.py:202-204), from the stream's next raw outputs with
// at::normal_distribution<double>'s arithmetic (Box-Muller: r = sqrt(-2 log1p(-u2)), theta = 2 pi u1; the sine sample is cached
// for the next draw) in host double precision / libm, exactly what torch's CPU path evaluates.
static void mt_segments(const CandDev& c, int R, int C, const float* b, uint32_t seed, int64_t flat_off, MtCand& m) {
    memset(&m, 0, sizeof(m));
    m.seed = seed; m.flat_off = flat_off;
    int64_t pos = 0;
    auto seg = [&](int64_t dst, int64_t n, float bd) {
        m.start[m.nseg] = pos; m.dst[m.nseg] = dst; m.lo[m.nseg] = -bd; m.hi[m.nseg] = bd;
        pos += n; ++m.nseg;
    };
    for (int i = 0; i < c.L; ++i) {
        seg(c.f_W[i], (int64_t)R * c.K_in[i], b[2 * i]);
        seg(c.f_b[i], R, b[2 * i + 1]);
    }
    seg(c.f_Wc, (int64_t)C * R, b[2 * MFAS_MAX_CELLS]);
    seg(c.f_bc, C, b[2 * MFAS_MAX_CELLS + 1]);
    m.start[m.nseg] = pos; m.total = pos;
}

static void draw_alphas(const uint32_t* t, int L, double alpha_mean, double alpha_std, float* alpha) {
    int used = 0; bool cached = false; double cache = 0.0;
    auto u53 = [&]() {      // uniform_real_distribution<double>: random64() = (first << 32) | second, 53 bits
        const uint64_t hi = t[used], lo = t[used + 1];
        used += 2;
        return (double)(((hi << 32) | lo) & ((1ULL << 53) - 1)) * (1.0 / 9007199254740992.0);
    };
    for (int i = 0; i < L; ++i) {
        double z;
        if (cached) { z = cache; cached = false; }
        else {
            const double u1 = u53(), u2 = u53();
            const double r = ::sqrt(-2.0 * ::log1p(-u2)), theta = 2.0 * 3.14159265358979323846 * u1;
            cache = r * ::sin(theta); cached = true;
            z = r * ::cos(theta);
        }
        alpha[i] = (float)(z * alpha_std + alpha_mean);
    }
}

extern "C" int mfas_population_init_torch_streams(mfas_population* p, const uint64_t* seeds, const float* bounds, double alpha_mean,
                                                  double alpha_std) {
    if (!p || !seeds || !bounds) return fail(MFAS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    const int K = p->K, R = p->hp.R, C = p->hp.C, NB = 2 * (MFAS_MAX_CELLS + 1);
    int64_t maxp = 0;
    for (int k = 0; k < K; ++k) maxp = std::max(maxp, p->plan.nparams[k]);
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(K, (64LL << 20) / std::max<int64_t>(maxp, 1)));     // <= 256 MB of flat scratch
    DevBuf<float> flat; DevBuf<MtCand> d_mt; DevBuf<uint32_t> d_tail;      // scratch of this call
    hipError_t e = flat.alloc((size_t)maxp * batch);
    if (e == hipSuccess) e = d_mt.alloc(batch);
    if (e == hipSuccess) e = d_tail.alloc((size_t)MT_TAIL * batch);
    if (e != hipSuccess) return fail(MFAS_ENOMEM, std::string("init_torch_streams: ") + hipGetErrorString(e));
    std::vector<MtCand> mt(batch);
    std::vector<uint32_t> tails((size_t)MT_TAIL * batch);
    std::vector<float> alpha((size_t)MFAS_MAX_CELLS * batch);
    for (int k0 = 0; k0 < K && e == hipSuccess; k0 += batch) {
        const int nb = std::min(batch, K - k0);
        for (int j = 0; j < nb; ++j)
            mt_segments(p->plan.cands[k0 + j], R, C, bounds + (size_t)(k0 + j) * NB, (uint32_t)(seeds[k0 + j] & 0xffffffffULL), (int64_t)j * maxp, mt[j]);
        e = hipMemcpyAsync(d_mt.get(), mt.data(), sizeof(MtCand) * nb, hipMemcpyHostToDevice, p->stream);
        if (e == hipSuccess) e = hipMemsetAsync(flat.get(), 0, sizeof(float) * (size_t)maxp * nb, p->stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_mt_uniform, dim3(nb), dim3(256), 0, p->stream, d_mt.get(), flat.get(), d_tail.get());
        e = hipMemcpyAsync(tails.data(), d_tail.get(), sizeof(uint32_t) * MT_TAIL * nb, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) break;
        for (int j = 0; j < nb && e == hipSuccess; ++j) {
            const int k = k0 + j;
            const CandDev& c = p->plan.cands[k];
            // BatchNorm defaults (gamma = 1, running_var = 1) and the alphas, then the usual repacking of a flat vector
            draw_alphas(tails.data() + (size_t)j * MT_TAIL, c.L, alpha_mean, alpha_std, alpha.data() + (size_t)j * MFAS_MAX_CELLS);
            float* fk = flat.get() + (int64_t)j * maxp;
            e = hipMemcpyAsync(fk + c.f_alpha, alpha.data() + (size_t)j * MFAS_MAX_CELLS, sizeof(float) * c.L, hipMemcpyHostToDevice, p->stream);
            if (e != hipSuccess) break;
            for (int i = 0; i < c.L && p->hp.bn; ++i) {
                hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, p->stream, fk + c.f_bn[i], 1.0f, (int64_t)R);             // gamma
                hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, p->stream, fk + c.f_bn[i] + 3 * (int64_t)R, 1.0f, (int64_t)R);   // running_var
            }
            if (const int rc = mfas_population_set_params(p, k, fk)) return rc;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);       // the scratch is reused by the next batch
    }
    if (e != hipSuccess) return fail(MFAS_EHIP, std::string("init_torch_streams: ") + hipGetErrorString(e));
    return MFAS_OK;
}

// a whole candidate from one population to another, its progress record included
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
    if (dst->d_move.size() < (size_t)n) HIPCHK(hipStreamSynchronize(dst->stream));      // (an earlier move may still read the scratch)
    HIPCHK(dst->d_move.reserve((size_t)n));
    const bool with_best = src->best && src->prog.keeps_best[ks];
    if (with_best) HIPCHK(keep_best(dst, BEST_LIVE_IF_NEW, dst->stream));
    if (src->stream != dst->stream) HIPCHK(hipStreamSynchronize(src->stream));      // what src trained is in memory
    HIPCHK(carry_candidate(dst, kd, src, ks, with_best, dst->d_move.get(), dst->stream));
    HIPCHK(hipMemcpyAsync(dst->d_status.get() + kd, src->d_status.get() + ks, sizeof(int32_t), hipMemcpyDeviceToDevice, dst->stream));
    dst->prog.done[kd] = src->prog.done[ks]; dst->prog.nb[kd] = src->prog.nb[ks];
    dst->prog.best_metric[kd] = src->prog.best_metric[ks]; dst->prog.keeps_best[kd] = with_best ? 1 : 0;
    return MFAS_OK;
}

// The resident persistent schedule needs every workgroup of its two launches on the GPU at the same time.  When that cannot be
// had — another process keeps CUs busy for good, the device is CU-masked, a tool serialises the two launches — the roll call fails
// BEFORE anything of the epoch has run (abort code 2), so the state in memory is that of the last completed epoch: create the
// launch-per-phase population, carry every candidate (the kept-best plane whenever there is one), swap the two records' contents — the
// handle keeps its identity — and go on from the same epoch.
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
    mfas_population* made = nullptr;
    if (int rc = create_impl(&p->hp, confs.data(), ncells.data(), seeds.data(), K, p->device, p->stream, p->chunk_cols_req, &made, false, &p->tune)) return rc;
    std::unique_ptr<mfas_population> q(made);      // (leaves with this function: the new record on a failure, the resident layout after the swap)
    DevBuf<float> flat;
    if (flat.alloc((size_t)maxp) != hipSuccess) return fail(MFAS_ENOMEM, "persist_fallback: scratch");
    const bool with_best = (bool)p->best;
    if (with_best && keep_best(q.get(), BEST_ZERO, p->stream) != hipSuccess) return fail(MFAS_ENOMEM, "persist_fallback: snapshot");
    hipError_t e = hipSuccess;
    for (int k = 0; k < K && e == hipSuccess; ++k) e = carry_candidate(q.get(), k, p, k, with_best, flat.get(), p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_posw.get(), p->d_posw.get(), sizeof(float) * p->plan.g.Cp, hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_status.get(), p->d_status.get(), sizeof(int32_t) * K, hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return fail(MFAS_EHIP, std::string("persist_fallback: ") + hipGetErrorString(e));
    // the handle keeps the whole progress record, the stats / event storage and what it was asked to profile (the device copy of the
    // step scalars goes with the resident layout: only k_president reads it)
    std::swap(q->d_stats, p->d_stats);
    std::swap(q->ev, p->ev); q->profiling = p->profiling; q->prof_every = p->prof_every;
    q->best_threshold = p->best_threshold; q->prog = p->prog; q->fell_back = 1;
    q->launched = p->launched;      // (the call's launch record goes on: the resident launches that were made, then the launch-per-phase ones)
    std::swap(*p, *q);
    return MFAS_OK;
}
