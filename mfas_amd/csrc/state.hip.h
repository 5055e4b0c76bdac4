// state.hip.h — candidate state in and out of a population (host only, included by mfas_hip.hip): single planes through the reference's
// flat state_dict order, the one candidate carry built on them (mfas_population_move, persist_fallback), the construction draws.
#pragma once

static PackArgs pack_args(mfas_population* p, int mode, int plane, float* flat) {
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.desc = p->d_descs; a.cands = p->d_cands; a.plane = p->plane; a.plane_stride = p->plan.plane_stride;
    a.wt = p->wt; a.flat = flat; a.seeds = p->d_seeds; a.mode = mode; a.sel_plane = plane; a.g = p->plan.g;
    return a;
}

// k_pack over candidate k's descriptors + k_vec for its vector block; k < 0: every candidate's (errors: hipGetLastError)
static void run_pack(mfas_population* p, PackArgs a, int k, bool vec, hipStream_t st) {
    const int d0 = k < 0 ? 0 : p->plan.desc_start[k], d1 = k < 0 ? (int)p->plan.descs.size() : p->plan.desc_start[k + 1];
    a.desc = p->d_descs + d0;
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
        if (hipError_t e = get_plane(src, ks, i == 3 ? src->best : src->plane, sel, flat, st)) return e;
        put_plane(dst, kd, i == 3 ? dst->best : dst->plane, sel, i == 0 ? PK_SET : PK_PUT, i == 0, flat, st);
    }
    return hipGetLastError();
}

// the kept-best plane of a population that has none yet: every candidate's starts as a copy of its live parameters
static int ensure_best(mfas_population* p, hipStream_t st) {
    if (p->best) return MFAS_OK;
    HIPCHK(hipMalloc(&p->best, sizeof(float) * (size_t)p->plan.plane_stride));
    HIPCHK(hipMemcpyAsync(p->best, p->plane, sizeof(float) * (size_t)p->plan.plane_stride, hipMemcpyDeviceToDevice, st));
    return MFAS_OK;
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
    float* flat = nullptr; MtCand* d_mt = nullptr; uint32_t* d_tail = nullptr;
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
        for (int j = 0; j < nb; ++j)
            mt_segments(p->plan.cands[k0 + j], R, C, bounds + (size_t)(k0 + j) * NB, (uint32_t)(seeds[k0 + j] & 0xffffffffULL), (int64_t)j * maxp, mt[j]);
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
            draw_alphas(tails.data() + (size_t)j * MT_TAIL, c.L, alpha_mean, alpha_std, alpha.data() + (size_t)j * MFAS_MAX_CELLS);
            float* fk = flat + (int64_t)j * maxp;
            e = hipMemcpyAsync(fk + c.f_alpha, alpha.data() + (size_t)j * MFAS_MAX_CELLS, sizeof(float) * c.L, hipMemcpyHostToDevice, p->stream);
            if (e != hipSuccess) break;
            for (int i = 0; i < c.L && p->hp.bn; ++i) {
                hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, p->stream, fk + c.f_bn[i], 1.0f, (int64_t)R);             // gamma
                hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, p->stream, fk + c.f_bn[i] + 3 * (int64_t)R, 1.0f, (int64_t)R);   // running_var
            }
            if (const int rc = mfas_population_set_params(p, k, fk)) { cleanup(); return rc; }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);       // the scratch is reused by the next batch
    }
    cleanup();
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
    if (dst->move_cap < n) {
        HIPCHK(hipStreamSynchronize(dst->stream));      // (an earlier move may still read the scratch)
        hipFree(dst->d_move); dst->d_move = nullptr; dst->move_cap = 0;
        HIPCHK(hipMalloc(&dst->d_move, sizeof(float) * (size_t)n));
        dst->move_cap = n;
    }
    const bool with_best = src->best && src->prog.keeps_best[ks];
    if (with_best) if (int rc = ensure_best(dst, dst->stream)) return rc;
    if (src->stream != dst->stream) HIPCHK(hipStreamSynchronize(src->stream));      // what src trained is in memory
    HIPCHK(carry_candidate(dst, kd, src, ks, with_best, dst->d_move, dst->stream));
    HIPCHK(hipMemcpyAsync(dst->d_status + kd, src->d_status + ks, sizeof(int32_t), hipMemcpyDeviceToDevice, dst->stream));
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
    for (int k = 0; k < K && e == hipSuccess; ++k) e = carry_candidate(q, k, p, k, p->best != nullptr, flat, p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_posw, p->d_posw, sizeof(float) * p->plan.g.Cp, hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_status, p->d_status, sizeof(int32_t) * K, hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    hipFree(flat);
    if (e != hipSuccess) { mfas_population_destroy(q); return fail(MFAS_EHIP, std::string("persist_fallback: ") + hipGetErrorString(e)); }
    // the handle keeps the whole progress record, the stats / scalar / event storage and what it was asked to profile
    std::swap(q->d_stats, p->d_stats); std::swap(q->stats_cap, p->stats_cap);
    std::swap(q->d_scal, p->d_scal); std::swap(q->scal_cap, p->scal_cap);
    q->ev.swap(p->ev); q->profiling = p->profiling; q->prof_every = p->prof_every;
    q->best_threshold = p->best_threshold; q->prog = p->prog; q->fell_back = 1;
    q->launched = p->launched;      // (the call's launch record goes on: the resident launches that were made, then the launch-per-phase ones)
    std::swap(*p, *q);
    mfas_population_destroy(q);      // the resident layout
    return MFAS_OK;
}
