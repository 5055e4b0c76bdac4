// train.hip.h — mfas_population_train / _train_from (host only, included by mfas_hip.hip after the kernel tables and state.hip.h): the
// state of one call, the step-independent kernel arguments, one function that turns a record of the launch list (launches.hip.h) into
// a launch, the resident epoch with its relaunch and fallback, and the call in named steps: check, begin, epoch, dev, end.
#pragma once
struct TrainCall {
    mfas_population* p = nullptr;
    const mfas_table *train = nullptr, *dev = nullptr;
    const int32_t* order = nullptr; const float* step_scalars = nullptr;
    int epochs = 0, first = 0, last = 0, B = 0;
    bool segment = false, resume = false, do_dev = false, snapshot_best = false;
    int64_t max_steps = -1, N = 0, nb = 0;  // train rows, batches per epoch
    AdamC ac; StepArgs st;
    std::vector<Launch> launches;       // the launches of an epoch of launches_T steps (only max_steps makes an epoch shorter)
    int64_t launches_T = -1;
    // host state that spans epochs: the exchange parity counts launches over the whole call (and restarts after a fallback)
    int64_t split_launches[2] = {0, 0}; // chain_split launches of this call per candidate group (exchange parity)
    size_t ev_used = 0;                 // profiling: events used by this call, algorithmic bytes of each bracketed launch, sweep launches so far
    std::vector<double> ev_bytes; int64_t nlaunch = 0;
    bool use_gather = false;            // gathered rows (sweep.hip.h, gather_body): two-group streaming schedule + per-candidate sample orders
    int64_t g_par_stride = 0, g_cand_stride = 0;
    std::vector<uint32_t> aborts;       // abort word of every epoch's resident launch
    std::vector<double> best_acc;       // best dev metric so far per candidate (train_searchable/ntu.py:18,82-83)
    double metric_scale = 1.0; std::vector<DevStats> hstats;
    int elt() const { return train->dtype == MFAS_DT_F32 ? 4 : 2; }
    double dev_metric(int k, int ep) const { return (double)hstats[(size_t)k * epochs + ep].dev_corr * metric_scale / (double)dev->N; }
};

// The step-independent kernel arguments of population p over one table (sa / ca zeroed by the caller): what train, the resident
// launch and single_batch share.  What a launch adds: work list, positions, step scalars, flags.
static void base_args(mfas_population* p, const mfas_table& tab, const int32_t* order, const Geo& g, const AdamC& ac, SweepArgs& sa, ChainArgs& ca) {
    const LayoutPlan& pl = p->plan;
    sa.cands = p->d_cands.get(); sa.plane = p->plane.get(); sa.plane_stride = pl.plane_stride; sa.wt = p->wt.get();
    sa.stepbuf = p->stepbuf.get(); sa.tab = tab; sa.order = order; sa.g = g; sa.ac = ac;
    ca.plane = p->plane.get(); ca.plane_stride = pl.plane_stride; ca.wt = p->wt.get(); ca.stepbuf = p->stepbuf.get();
    ca.tab = tab; ca.order = order; ca.g = g; ca.status = p->d_status.get(); ca.ac = ac;
    ca.yf_in_lds = pl.yf_in_lds ? 1 : 0; ca.vec_in_lds = pl.vec_in_lds ? 1 : 0; ca.pos_w = p->d_posw.get();
}

// base_args' counterpart for k_eval: the step-independent EvalArgs of population p over one table, reading the parameters at plane_base
// (p->plane or p->best) — one schedule of one epoch (E = 1).  What a caller adds: rows, candidate, epoch, statistics and output pointers.
static EvalArgs eval_args(mfas_population* p, const mfas_table& tab, float* plane_base, const Geo& g) {
    EvalArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.cands = p->d_cands.get(); ea.plane = plane_base; ea.tab = tab; ea.g = g; ea.pos_w = p->d_posw.get(); ea.E = 1;
    return ea;
}

static hipError_t setup_gather(TrainCall& c) {
    mfas_population* p = c.p;
    const Geo& g = c.st.sa.g;
    c.use_gather = p->plan.groups.size() == 2 && !p->plan.persist && c.order && g.order_stride > 0 && !p->tune.no_gather;
    if (!c.use_gather) return hipSuccess;
    int64_t totw = 0;
    for (int u = 0; u < MFAS_MAX_TAPS; ++u) totw += g.sw[u] + g.vw[u];
    c.g_par_stride = totw * g.Bp * c.elt(); c.g_cand_stride = row_sets(p->plan.defer) * c.g_par_stride;     // (a deferring plan keeps three batches)
    const size_t need = (size_t)c.g_cand_stride * p->K;
    if (p->d_gather.reserve(need) != hipSuccess) { c.use_gather = false; (void)hipGetLastError(); return hipSuccess; }   // an optimisation: train without it
    if (p->tune.gather_verbose)
        fprintf(stderr, "[gather] on: %d candidates, %.1f MB of gathered rows, %d row sets%s\n", p->K, (double)need / 1e6, row_sets(p->plan.defer),
                p->plan.defer ? " (feature segments store W / m / v every second step)" : "");
    return hipSuccess;
}

// everything launch_record needs, for a call — or the launch-per-phase layout taking over after persist_fallback — that starts at epoch ep
static hipError_t init_args(TrainCall& c, int64_t ep) {
    mfas_population* p = c.p; StepArgs& st = c.st;
    const LayoutPlan& pl = p->plan; const int K = p->K;
    c.launches_T = -1;
    Geo g = pl.g;
    g.order_stride = (p->hp.order_per_candidate && c.order) ? (int64_t)c.epochs * c.N : 0;    // order: [K][epochs][N_train]
    memset(&st, 0, sizeof(st));
    base_args(p, *c.train, c.order, g, c.ac, st.sa, st.ca);
    st.ca.E = c.epochs; st.ca.stats = p->d_stats.get();
    st.sa.red_cnt = p->d_red_cnt.get(); st.ca.yf_reduced = pl.red_in_sweep ? 1 : 0;
    hipError_t e_ = hipSuccess;
    if (pl.red_in_sweep) e_ = hipMemsetAsync(p->d_red_cnt.get(), 0, sizeof(uint32_t) * K * MFAS_MAX_CELLS, p->stream);
    if (e_ == hipSuccess && pl.same_group) e_ = hipMemsetAsync(p->d_cellflag.get(), 0, sizeof(uint32_t) * K * CELLFLAG_STRIDE, p->stream);
    // chain_split: every piece of both parities "not written" (all-ones words), parity counter back to 0
    if (e_ == hipSuccess && pl.chain_split) e_ = hipMemsetAsync(p->d_xch.get(), 0xFF, sizeof(float) * (size_t)K * XCH_CAND_FLOATS, p->stream);
    st.ca.xch = p->d_xch.get(); st.ca.nsplit = pl.chain_split; st.ca.xpar = 0;
    c.split_launches[0] = c.split_launches[1] = 0;
    // chain_split in the same-group launch counts ARRIVALS on the per-cell flags: every part adds 1 per step and a sweep unit waits for
    // parts * (gstep + 1).  Zero is right for a call that starts at step 0; one that starts at epoch ep (a later segment, or a fallback
    // mid-call) starts them where steps 0 .. ep * nb - 1 would have left them.  (The one-part chain stores its target and needs nothing.)
    if (e_ == hipSuccess && ep > 0 && pl.same_group && pl.chain_split)
        e_ = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->d_cellflag.get()), (int)((uint32_t)pl.chain_split * (uint32_t)(ep * c.nb)),
                               (size_t)K * CELLFLAG_STRIDE, p->stream);
    return e_ != hipSuccess ? e_ : setup_gather(c);
}

// HIP events around one profiled launch (the pairs are kept in the population and reused by later calls)
struct ProfBracket {
    TrainCall& c;
    bool on;                        // (off for this launch when its events cannot be created)
    const double bytes;             // algorithmic HBM bytes of the launch
    ProfBracket(TrainCall& c_, bool on_, double bytes_) : c(c_), on(on_), bytes(bytes_) {
        if (!on) return;
        mfas_population* p = c.p;
        if (p->ev.v.size() < c.ev_used + 2 && !p->ev.add_pair()) {
            on = false;
            return;
        }
        hipEventRecord(p->ev.v[c.ev_used], p->stream);
    }
    ~ProfBracket() {
        if (!on) return;
        hipEventRecord(c.p->ev.v[c.ev_used + 1], c.p->stream);
        c.ev_used += 2; c.ev_bytes.push_back(bytes);
    }
};

// one record of the launch list -> one launch of epoch ep: the step-dependent arguments (positions and valid rows, step scalars, flag
// target, exchange parity, gather parities), the build, the launch
static void launch_record(TrainCall& c, int64_t ep, const Launch& L) {
    mfas_population* p = c.p;
    const LayoutPlan& pl = p->plan;
    StepArgs& st = c.st;
    const int64_t N = c.N;
    const int B = c.B, gs = L.sweep_g, gc = L.chain_g;
    auto nvalid = [&](int64_t t) { return (int)std::min<int64_t>(B, N - t * B); };
    unsigned nsw = 0, nch = 0;
    st.ga.nblocks = 0; st.ga.nsets = 0; st.sa.gather = nullptr;
    if (c.use_gather) {
        GatherArgs& ga = st.ga;
        ga.buf = p->d_gather.get(); ga.cand_stride = c.g_cand_stride; ga.par_stride = c.g_par_stride;
        for (int s = 0; s < L.gather_n; ++s) {
            const int64_t t = L.gather_b + s;
            ga.pos[s] = ep * N + t * B; ga.base[s] = (int)(t * B); ga.nvalid[s] = nvalid(t); ga.par[s] = row_set_of(t, pl.defer);
        }
        if (L.gather_g >= 0) { ga.nsets = L.gather_n; ga.cands = p->d_cands.get() + pl.groups[L.gather_g].c0; ga.nblocks = pl.groups[L.gather_g].nc; }
        if (gs >= 0 && L.upd) {
            st.sa.gather = p->d_gather.get(); st.sa.g_cand_stride = c.g_cand_stride; st.sa.g_par_stride = c.g_par_stride;
            st.sa.g_par_t = row_set_of(L.sweep_t, pl.defer); st.sa.g_par_n = row_set_of(L.sweep_t + 1, pl.defer);
            st.sa.g_par_p = row_set_of(std::max<int64_t>(L.sweep_t - 1, 0), pl.defer);
        }
    }
    if (gs >= 0) {
        SweepArgs& s = st.sa;
        const int64_t ts = L.sweep_t, tn = L.fwd && L.upd ? ts + 1 : ts, gstep = ep * c.nb + ts;
        s.desc = p->groups[gs].d_descs.get();
        s.tdesc = p->groups[gs].d_taps.get(); s.ntap = (int)pl.groups[gs].taps.size();
        s.do_update = L.upd; s.do_forward = L.fwd;
        s.pos_t = ep * N + ts * B; s.base_t = (int)(ts * B); s.nvalid_t = nvalid(ts);
        s.pos_n = ep * N + tn * B; s.base_n = (int)(tn * B); s.nvalid_n = nvalid(tn);
        s.ac.ss = L.upd ? c.step_scalars[2 * gstep] : 0.f;
        s.ac.bc2s = L.upd ? c.step_scalars[2 * gstep + 1] : 1.f;
        // deferred stores: the mode, this step's dy area and — a double pass replays step ts - 1 first — that step's rows, dy area and scalars
        s.mode = L.mode;
        s.g.sb_dy = dy_area_of(ts, pl.defer) ? pl.sb_dy_alt : pl.g.sb_dy;
        if (L.mode == LAUNCH_DOUBLE) {
            s.pos_p = ep * N + (ts - 1) * B; s.base_p = (int)((ts - 1) * B); s.nvalid_p = nvalid(ts - 1);
            s.sb_dy_prev = dy_area_of(ts - 1, pl.defer) ? pl.sb_dy_alt : pl.g.sb_dy;
            s.ss_p = c.step_scalars[2 * (gstep - 1)]; s.bc2s_p = c.step_scalars[2 * (gstep - 1) + 1];
        }
        nsw = (unsigned)(pl.groups[gs].descs.size() + pl.groups[gs].taps.size());
    } else st.sa.ntap = 0;
    if (gc >= 0) {
        ChainArgs& ca = st.ca;
        const int64_t tc = L.chain_t, gstep = ep * c.nb + tc;
        ca.cands = p->d_cands.get() + pl.groups[gc].c0;
        ca.pos_t = ep * N + tc * B; ca.base_t = (int)(tc * B); ca.nvalid = nvalid(tc);
        ca.gstep = (int)gstep; ca.epoch = (int)ep;
        ca.ac.ss = c.step_scalars[2 * gstep]; ca.ac.bc2s = c.step_scalars[2 * gstep + 1];
        ca.g.sb_dy = dy_area_of(tc, pl.defer) ? pl.sb_dy_alt : pl.g.sb_dy;      // (the sweep of step tc reads it there)
        nch = (unsigned)pl.groups[gc].nc;
    }
    st.nchain = (int)nch;
    if (nsw == 0) {   // chain only: the latency-tuned standalone kernel (wide populations: theirs)
        launch_build(p, chain_build(chain_key(plan_facts(pl))), nch, pl.lds_chain, p->stream, st.ca);
        return;
    }
    // algorithmic HBM bytes of this group's update+forward sweep: 24 B/param + the batch's taps + labels
    // (every prof_every-th such launch, alternately that one and the one two launches on: in a deferring plan launch 16 k is always the
    // same group's virtual pass and 16 k + 2 its double pass, so the sample weighs the short and the long kind equally)
    bool sampled = false;
    if (p->profiling && L.upd && L.fwd) {
        const int64_t n = c.nlaunch++, pe = p->prof_every;
        sampled = n % pe == (((n / pe) & 1) ? 2 % pe : 0);
    }
    ProfBracket prof(c, sampled,
                     pl.groups[gs].alg_state + pl.groups[gs].alg_feat * c.elt() + 8.0 * B * pl.groups[gs].nc);
    const bool same = pl.same_group && gc == gs && L.upd, split = pl.chain_split && nch > 0;     // (split in a two-group launch: no flags, the kernel boundary)
    if (split) {    // NS parts per candidate, chain blocks = NS * ceil8(candidates)
        st.ca.ncand = (int)nch; st.ca.xpar = (int)(c.split_launches[gc & 1]++ & 1);
        st.nchain = pl.chain_split * (int)((nch + 7) & ~7u);
    }
    if (same) {       // (NS parts: the per-cell flags count arrivals)
        st.sa.cellflag = st.ca.cellflag = p->d_cellflag.get();
        st.sa.flag_target = st.ca.flag_target = (split ? (uint32_t)pl.chain_split : 1u) * ((uint32_t)st.ca.gstep + 1u);
        st.sa.flag_status = p->d_status.get();
    }
    const BuildKey key = step_key(plan_facts(pl), nch, same, pl.groups[gs].alg_state > pl.occ_bytes);
    launch_build(p, step_build(key), (unsigned)st.nchain + st.ga.nblocks + nsw, split ? pl.lds_split : pl.lds_step, p->stream, st);
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
    hipError_t e = hipMemsetAsync(p->d_sync.get(), 0, sizeof(uint32_t) * ((size_t)K * PERSIST_SYNC_STRIDE + 64), p->stream);
    if (e != hipSuccess) return e;
    PersistArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.sa = c.st.sa; pa.ca = c.st.ca;      // (init_args: the step-independent arguments)
    pa.sa.desc = p->d_pdescs.get(); pa.sa.tdesc = nullptr; pa.sa.ntap = 0;
    pa.ca.cands = p->d_cands.get();
    pa.nchain = K; pa.nitems = (int)pl.pdescs.size(); pa.nres = pl.nres; pa.res_chain = pl.res_chain ? 1 : 0; pa.res_wide = pl.res_wide ? 1 : 0;
    pa.res_nu = pl.res_nu; pa.nres_wg = pl.nres_wg; pa.res_buf_words = pl.res_buf_words;
    pa.T = (int)T; pa.epoch = ep;
    pa.lose_step = p->tune.test_lose_step;
    pa.N = c.N; pa.pos0 = (int64_t)ep * c.N;
    pa.B = c.B; pa.gstep0 = (int)((int64_t)ep * c.nb);
    pa.scal = p->d_scal.get(); pa.sync = p->d_sync.get(); pa.need = p->d_need.get(); pa.role = p->d_role.get(); pa.trace = p->d_trace.get();
    const unsigned grid = (unsigned)(K + pa.nres_wg);
    if ((int)grid > p->n_cus) return hipErrorInvalidConfiguration;
    {
        // algorithmic bytes of the launch: T update+forward sweeps of every candidate
        ProfBracket prof(c, p->profiling, (double)T * (pl.groups[0].alg_state + pl.groups[0].alg_feat * c.elt() + 8.0 * c.B * K));
        const int lw = (int)(pl.lds_president / 4) - PERSIST_LDS_WORDS;
        // (PLAIN = 2: `--batchnorm` alone, main_searchable_ntu.py:48 of the reference)
        const int plain = president_plain(g.alphas, g.multitask, g.loss_mode, g.bn, p->tune.no_plain_chain);
        launch_build(p, president_build(president_key(plan_facts(pl), c.train->dtype != MFAS_DT_F32, plain)), grid, pl.lds_president, p->stream, pa, lw);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(&c.aborts[ep], p->d_sync.get() + (size_t)K * PERSIST_SYNC_STRIDE, sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream);
}

// The launch is only valid when its whole grid is resident at once (roll call, persist.hip.h).  When another process holds
// part of the GPU the roll call fails BEFORE anything is modified (abort code 2): wait a little (jittered, so that two
// processes that collided do not collide again in lockstep) and launch the epoch again — up to PERSIST_MAX_RELAUNCHES times
// (~0.3 s of trying); after that the caller gives the resident schedule up for this population (persist_fallback).
static hipError_t persist_epoch(TrainCall& c, int ep, int64_t T) {
    mfas_population* p = c.p;
    for (int attempt = 0;; ++attempt) {
        hipError_t e = persist_epoch_once(c, ep, T);
        if (e != hipSuccess) return e;
        e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) return e;
        if (p->tune.persist_verbose >= 2)
            fprintf(stderr, "[persist] epoch %d attempt %d: abort word %u\n", ep, attempt, c.aborts[ep]);
        if (c.aborts[ep] != PERSIST_ABORT_NOT_RESIDENT || attempt >= PERSIST_MAX_RELAUNCHES || p->tune.test_not_resident >= 0) {
            if (attempt && p->tune.persist_verbose) fprintf(stderr, "[persist] epoch %d: grid not resident at once, relaunched %d time(s)\n", ep, attempt);
            return hipSuccess;
        }
        if (p->profiling && c.ev_used >= 2) { c.ev_used -= 2; c.ev_bytes.pop_back(); }       // the failed attempt is not a measurement
        c.aborts[ep] = 0;
        std::this_thread::sleep_for(std::chrono::microseconds(200 + (uint64_t)((reinterpret_cast<uintptr_t>(p) >> 6) * 2654435761u % 1800u) + 50u * (attempt % 16)));
    }
}
// MFAS_PERSIST_TRACE: the step-phase timestamps of the last resident launch
static void dump_persist_trace(const mfas_population* p) {
    unsigned long long tr[256];
    if (hipMemcpy(tr, p->d_trace.get(), sizeof(tr), hipMemcpyDeviceToHost) != hipSuccess) return;
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
    if (hipMemcpy(ts, p->d_status.get() + 64, sizeof(ts), hipMemcpyDeviceToHost) != hipSuccess) return;
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
        if (hipMemcpy(ue, p->d_status.get() + 128, sizeof(ue), hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "; last unit end after the end of chain 3, per cell [S V OUT HEAD]:");
            for (int i = 0; i < 16; ++i) fprintf(stderr, "%s%d", (i & 3) ? " " : " | ", ue[i] ? (int32_t)((uint32_t)ue[i] - (uint32_t)ts[24]) : 0);
        }
    }
    fprintf(stderr, "\n");
    int32_t cs[24];
    if (hipMemcpy(cs, p->d_status.get() + 96, sizeof(cs), hipMemcpyDeviceToHost) == hipSuccess) {
        fprintf(stderr, "[chain checksums, candidate 0 global step 0: sums x4, out x4, logits, dlogits, dy x4, d x4]");
        for (int i = 0; i < 18; ++i) fprintf(stderr, " %08x", (unsigned)cs[i]);
        fprintf(stderr, "\n");
    }
}
#endif

// mfas_population_train and mfas_population_train_from in five steps: epochs [first, last) of a schedule of `epochs` epochs.
// segment = false is mfas_population_train (first = 0, last = epochs, the record is reset); segment = true keeps the progress record,
// and with first > 0 goes on from the state the previous segment left instead of from a fresh optimizer.
// check: everything that can refuse, touching nothing — a refused segment leaves the population as it was
static int train_check(TrainCall& c, const mfas_epoch_stats* stats) {
    mfas_population* p = c.p;
    const int first = c.first, last = c.last, epochs = c.epochs;
    if (!p || !c.step_scalars || epochs <= 0 || !stats) return fail(MFAS_EINVAL, "bad argument");
    if (first < 0 || last <= first || last > epochs)
        return fail(MFAS_EINVAL, "train_from: epochs [" + std::to_string(first) + ", " + std::to_string(last) + ") are no segment of a schedule of " + std::to_string(epochs));
    if (int rc = check_table(p, c.train, p->plan.g.multitask)) return rc;
    c.do_dev = c.max_steps < 0;
    if (c.do_dev) if (int rc = check_table(p, c.dev, p->plan.g.multitask)) return rc;
    HIPCHK(hipSetDevice(p->device));
    const Geo& g = p->plan.g;
    c.B = g.B; c.N = c.train->N;
    const int64_t nb = c.nb = (c.N + c.B - 1) / c.B;
    if (p->plan.persist && p->plan.nres > 0 && p->hp.tap_bits == 16 && c.train->dtype == MFAS_DT_F32)
        return fail(MFAS_EINVAL, "this population was created for 16-bit feature tables (mfas_hyper.tap_bits = 16); f32 tables need tap_bits = 32 or 0");
    if (c.N - (nb - 1) * c.B == 1 && g.bn)   // torch BatchNorm1d raises on a size-1 train batch
        return fail(MFAS_EINVAL, "final train batch of size 1 with batchnorm (reference raises ValueError)");
    c.resume = first > 0;
    for (int k = 0; k < p->K && c.resume; ++k) {
        const mfas_population::Progress& pr = p->prog;
        if (pr.done[k] != first || pr.nb[k] != nb)
            return fail(MFAS_EINVAL, "train_from: first_epoch = " + std::to_string(first) + " of a schedule with " + std::to_string(nb) +
                                     " batches per epoch, but candidate " + std::to_string(k) + "'s progress record says " + std::to_string(pr.done[k]) +
                                     " epoch(s) complete of a schedule with " + std::to_string(pr.nb[k]) + " batches per epoch");
        if ((pr.keeps_best[k] != 0) != c.snapshot_best || (c.snapshot_best && !p->best))
            return fail(MFAS_EINVAL, "train_from: snapshot_best = " + std::to_string(c.snapshot_best) + " at first_epoch = " + std::to_string(first) +
                                     ", but candidate " + std::to_string(k) + "'s schedule was started with snapshot_best = " + std::to_string(pr.keeps_best[k]));
    }
    return MFAS_OK;
}

// begin: the record, the buffers and their memsets, the call's arguments
static int train_begin(TrainCall& c) {
    mfas_population* p = c.p;
    const int K = p->K, epochs = c.epochs;
    const size_t plane = (size_t)p->plan.plane_stride;
    if (!c.segment) p->prog.reset(K, p->best_threshold);      // a plain train() call owes nothing to an earlier schedule
    HIPCHK(p->d_stats.reserve((size_t)K * epochs));
    HIPCHK(hipMemsetAsync(p->d_stats.get(), 0, sizeof(DevStats) * K * epochs, p->stream));
    if (!c.resume) HIPCHK(hipMemsetAsync(p->d_status.get(), 0, sizeof(int32_t) * K, p->stream));      // (sticky across the segments of a schedule)
#ifdef MFAS_CHAIN_TIMING
    HIPCHK(hipMemsetAsync(p->d_status.get() + 64 + 27, 0, sizeof(int32_t), p->stream));
    HIPCHK(hipMemsetAsync(p->d_status.get() + 128, 0, 16 * sizeof(int32_t), p->stream));
    HIPCHK(hipMemsetAsync(p->d_status.get() + 64 + 28, 0xFF, sizeof(int32_t), p->stream));
#endif
    // every call is a freshly built torch.optim.Adam (ntu_searchable.py:65; main_found_ntu.py:108,128): zero exp_avg / exp_avg_sq
    // (a segment that goes on finds the optimizer's state where the previous one left it)
    if (!c.resume) HIPCHK(hipMemsetAsync(p->plane.get() + plane, 0, sizeof(float) * 2 * plane, p->stream));
    // best_model_sd starts as a copy of the INITIAL state_dict (train_searchable/ntu.py:17) and is what the model is
    // left with if no epoch's dev metric beats the starting threshold (0 for accuracy, init_f1 for F1)
    if (c.snapshot_best) HIPCHK(keep_best(p, c.do_dev && !c.resume ? BEST_LIVE : BEST_AS_IS, p->stream));
    c.best_acc.assign(K, p->best_threshold);
    if (c.resume) c.best_acc = p->prog.best_metric;
    c.metric_scale = p->plan.g.loss_mode == 1 ? 1.0 / 4294967296.0 : 1.0;   // F1 sums are 32.32 fixed point
    c.hstats.resize((size_t)K * epochs);
    const mfas_hyper& hp = p->hp;
    c.ac.w1 = (float)(1.0 - hp.beta1); c.ac.b2 = (float)hp.beta2; c.ac.w2 = (float)(1.0 - hp.beta2);
    c.ac.eps = (float)hp.adam_eps; c.ac.wd = (float)hp.wd; c.ac.ss = 0.f; c.ac.bc2s = 1.f;
    c.aborts.assign(epochs, 0u);
    HIPCHK(init_args(c, c.first));
    p->prof_launches = 0; p->prof_ms = 0.0; p->prof_bytes = 0.0;
    if (p->plan.persist) {   // the step scalars live on the device: the kernel walks the steps itself
        const int64_t steps = (int64_t)epochs * c.nb;
        HIPCHK(p->d_scal.reserve((size_t)steps * 2));
        const size_t have = (size_t)(c.max_steps >= 0 ? std::min<int64_t>(c.max_steps, steps) : steps) * 2;
        HIPCHK(hipMemcpyAsync(p->d_scal.get(), c.step_scalars, sizeof(float) * have, hipMemcpyHostToDevice, p->stream));
    }
    return MFAS_OK;
}

// one epoch of T train steps: the resident launch (relaunched while its grid is not resident; given up for launch-per-phase when it
// never is), or the launch list
static int train_epoch(TrainCall& c, int ep, int64_t T) {
    mfas_population* p = c.p;
    if (p->plan.persist) {
        HIPCHK(persist_epoch(c, ep, T));
        if (c.aborts[ep] == PERSIST_ABORT_NOT_RESIDENT) {
            // every attempt failed its roll call: nothing of this epoch has run.  Train it — and the rest — launch per phase.
            if (p->tune.persist_verbose) fprintf(stderr, "[persist] epoch %d: the resident grid never became resident; falling back to launch-per-phase\n", ep);
            if (int rc = persist_fallback(p)) return rc;
            HIPCHK(init_args(c, ep));
            c.aborts[ep] = 0;
        } else if (c.aborts[ep]) {
            HIPCHK(hipStreamSynchronize(p->stream));
            return fail(MFAS_EHIP, "persistent step loop: a workgroup timed out waiting for its dependency (abort code 1: the epoch was "
                                   "abandoned half way, this population's parameters are not usable)");
        }
    }
    if (!p->plan.persist) {
        if (c.launches_T != T) {
            epoch_launches((int)p->plan.groups.size(), p->plan.same_group, T, c.use_gather, c.launches);
            if (p->plan.defer) mark_deferred((int)p->plan.groups.size(), p->plan.same_group, c.launches);
            c.launches_T = T;
        }
        for (const Launch& L : c.launches) launch_record(c, ep, L);
    }
    HIPCHK(hipGetLastError());
    return MFAS_OK;
}

// the dev pass of epoch ep, and with snapshot_best the best-epoch bookkeeping
static int train_dev(TrainCall& c, int ep) {
    mfas_population* p = c.p;
    const int K = p->K;
    EvalArgs ea = eval_args(p, *c.dev, p->plane.get(), c.st.sa.g);      // (the call's g: its order stride)
    ea.nrows = c.dev->N; ea.epoch = ep; ea.E = c.epochs; ea.stats = p->d_stats.get();
    HIPCHK(launch_eval(p, ea, K, p->stream));
    if (!c.snapshot_best) return MFAS_OK;
    HIPCHK(hipMemcpyAsync(c.hstats.data(), p->d_stats.get(), sizeof(DevStats) * K * c.epochs, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    for (int k = 0; k < K; ++k) {
        const double acc = c.dev_metric(k, ep);
        if (acc > c.best_acc[k]) {   // strict >, from 0 (train_searchable/ntu.py:82) / init_f1 (mmimdb.py:18)
            c.best_acc[k] = acc;
            HIPCHK(hipMemcpyAsync(p->best.get() + p->plan.cand_plane_base[k], p->plane.get() + p->plan.cand_plane_base[k],
                                  sizeof(float) * p->plan.cand_plane_size[k], hipMemcpyDeviceToDevice, p->stream));
        }
    }
    return MFAS_OK;
}

// end: the best parameters back, statistics and status out, aborts and timeouts reported, the progress record, the profiling sums
static int train_end(TrainCall& c, mfas_epoch_stats* stats, int32_t* status) {
    mfas_population* p = c.p;
    const int K = p->K, epochs = c.epochs;
    if (c.snapshot_best && c.do_dev && c.last == epochs) {   // model.load_state_dict(best_model_sd) (:86), unconditionally — once the schedule is complete
        HIPCHK(hipMemcpyAsync(p->plane.get(), p->best.get(), sizeof(float) * (size_t)p->plan.plane_stride, hipMemcpyDeviceToDevice, p->stream));
        // the transposed OUT / HEAD tiles the backward chain reads still hold the last epoch's weights: re-derive them
        run_pack(p, pack_args(p, PK_WT, 0, nullptr), -1, false, p->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(c.hstats.data(), p->d_stats.get(), sizeof(DevStats) * K * epochs, hipMemcpyDeviceToHost, p->stream));
    std::vector<int32_t> hstatus(K, 0);
    HIPCHK(hipMemcpyAsync(hstatus.data(), p->d_status.get(), sizeof(int32_t) * K, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    for (uint32_t ab : c.aborts)
        if (ab) return fail(MFAS_EHIP, ab == PERSIST_ABORT_NOT_RESIDENT ? "persistent step loop: the grid never became resident (abort code 2)"
                                                                         : "persistent step loop: a workgroup timed out waiting for its dependency (abort code 1)");
    for (int32_t sv : hstatus)
        if (sv == 2) return fail(MFAS_EHIP, "same-group fused launch: a sweep unit timed out waiting for its cell's dy");
    if (p->d_trace && p->plan.persist) dump_persist_trace(p);
    for (size_t i = 0; i < c.hstats.size(); ++i) {
        stats[i].train_loss_sum = c.hstats[i].train_loss; stats[i].dev_loss_sum = c.hstats[i].dev_loss;
        stats[i].train_corrects = c.hstats[i].train_corr; stats[i].dev_corrects = c.hstats[i].dev_corr;
    }
    if (status) memcpy(status, hstatus.data(), sizeof(int32_t) * K);
    if (c.segment) {      // the record: where the schedule stands, and best_acc (train_searchable/ntu.py:18,82-83) so far
        for (int k = 0; k < K; ++k) {
            for (int ep = c.first; ep < c.last && !c.snapshot_best; ++ep)      // (snapshot_best has kept best_acc up to date epoch by epoch)
                c.best_acc[k] = std::max(c.best_acc[k], c.dev_metric(k, ep));
            p->prog.done[k] = c.last; p->prog.nb[k] = c.nb; p->prog.best_metric[k] = c.best_acc[k]; p->prog.keeps_best[k] = c.snapshot_best ? 1 : 0;
        }
    }
#ifdef MFAS_CHAIN_TIMING
    dump_chain_timing(p);
#endif
    if (p->profiling) {
        for (size_t i = 0; i + 1 < c.ev_used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p->ev.v[i], p->ev.v[i + 1]) == hipSuccess) { p->prof_ms += ms; p->prof_launches++; p->prof_bytes += c.ev_bytes[i / 2]; }
        }
        p->bytes_per_launch = p->prof_launches ? p->prof_bytes / p->prof_launches : 0.0;
    }
    return MFAS_OK;
}

static int train_impl(mfas_population* p, const mfas_table* train, const mfas_table* dev, const int32_t* order, const float* step_scalars,
                      int32_t epochs, int64_t max_steps, int32_t snapshot_best, mfas_epoch_stats* stats, int32_t* status,
                      const int32_t first, const int32_t last, const bool segment) {
    TrainCall c;
    c.p = p; c.train = train; c.dev = dev; c.order = order; c.step_scalars = step_scalars; c.epochs = epochs; c.max_steps = max_steps;
    c.snapshot_best = snapshot_best != 0; c.first = first; c.last = last; c.segment = segment;
    if (int rc = train_check(c, stats)) return rc;
    p->launched.clear();      // the launch record is the record of this call (launch_record, persist_epoch_once)
    RangeGuard call_range("mfas_population_train K=" + std::to_string(p->K) + " R=" + std::to_string(p->plan.g.R) + " B=" + std::to_string(c.B) +
                          " E=" + std::to_string(epochs) + (p->plan.persist ? " resident" : " launch-per-phase"));
    if (int rc = train_begin(c)) return rc;
    int64_t done = 0;   // train steps completed (max_steps bookkeeping)
    for (int ep = first; ep < last; ++ep) {
        const int64_t T = max_steps >= 0 ? std::min<int64_t>(c.nb, max_steps - done) : c.nb;
        if (T <= 0) break;
        RangeGuard epoch_range("epoch " + std::to_string(ep));
        if (int rc = train_epoch(c, ep, T)) return rc;
        done += T;
        if (c.do_dev) if (int rc = train_dev(c, ep)) return rc;
    }
    return train_end(c, stats, status);
}

// One batch through candidate k in TRAIN mode: forward only (logits out), or forward + backward of an external loss
// (dlogits in): then every parameter's Adam first-moment slot receives its exact GRADIENT and nothing else changes — the step
// runs with beta1 = 0 (m <- m + 1 * (g - m) = g), weight decay 0 and learning rate 0 (w <- w - 0 * m / denom = w).
// ds / dv (backward only; HOST [MFAS_MAX_TAPS] of DEVICE pointers or NULL): the gradients of those taps too — one k_tap_grad launch
// (tapgrad.hip.h) behind the chain's dy, before the call's one synchronise; with no pointer set nothing of it runs.
static int single_batch(mfas_population* p, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows, int32_t step_index,
                        float* logits, const float* dlogits, float* const* ds = nullptr, float* const* dv = nullptr) {
    if (!p || (!logits && !dlogits) || k < 0 || k >= p->K || row0 < 0) return fail(MFAS_EINVAL, "bad argument");
    if (int rc = check_table(p, tab, false)) return rc;
    const LayoutPlan& pl = p->plan;
    if (nrows < 1 || nrows > pl.g.B) return fail(MFAS_EINVAL, "train-mode forward: 1 <= rows <= the population's batch size");
    if (nrows == 1 && pl.g.bn) return fail(MFAS_EINVAL, "train-mode BatchNorm needs more than 1 row (reference: ValueError)");
    if (row0 + nrows > tab->N) return fail(MFAS_EINVAL, "row range outside the table");
    HIPCHK(hipSetDevice(p->device));
    AdamC ac;
    ac.w1 = 1.0f; ac.b2 = (float)p->hp.beta2; ac.w2 = (float)(1.0 - p->hp.beta2); ac.eps = (float)p->hp.adam_eps; ac.wd = 0.f; ac.ss = 0.f; ac.bc2s = 1.f;
    Geo g = pl.g; g.order_stride = 0;
    StepArgs st;
    ChainArgs ca;
    memset(&st, 0, sizeof(st)); memset(&ca, 0, sizeof(ca));
    base_args(p, *tab, nullptr, g, ac, st.sa, ca);
    // the sweep over this candidate's units alone, forward half first; the chain of this candidate alone, dropout stream of step_index
    st.sa.desc = pl.wide ? p->groups[0].d_descs.get() + pl.wide_start[k] : p->d_descs.get() + pl.desc_start[k];
    st.sa.do_update = 0; st.sa.do_forward = 1;
    st.sa.pos_n = st.sa.pos_t = ca.pos_t = row0; st.sa.base_n = st.sa.base_t = ca.base_t = (int)row0;
    st.sa.nvalid_n = st.sa.nvalid_t = ca.nvalid = nrows;
    ca.cands = p->d_cands.get() + k; ca.gstep = step_index; ca.E = 1;
    ca.logits_out = dlogits ? nullptr : logits; ca.dlogits_in = dlogits;
    const unsigned nsw = pl.wide ? (unsigned)(pl.wide_start[k + 1] - pl.wide_start[k]) : (unsigned)(pl.desc_start[k + 1] - pl.desc_start[k]);
    size_t lds_need = pl.lds_step;   // (a population laid out for resident units budgets its streaming LDS without them)
    if (!pl.wide)
        for (int j = pl.desc_start[k]; j < pl.desc_start[k + 1]; ++j) lds_need = std::max(lds_need, sweep_unit_lds(g, pl.descs[j]));
    if (lds_need > 150 * 1024) return fail(MFAS_EINVAL, "train-mode forward: this population's units are too wide for the streaming kernels");
    TapGradCall tg;      // (the last thing that can refuse: its work list is uploaded before anything is launched)
    if (dlogits && (ds || dv)) if (int rc = tap_grad_prepare(pl, p->hp, k, ds, dv, tg)) return rc;
    const StepKernel sweep_k = step_build(single_batch_step_key(plan_facts(pl))).fn;
    if (lds_need > pl.lds_step) HIPCHK(set_lds(sweep_k, lds_need));
    auto sweep = [&]() { launch(sweep_k, nsw, lds_need, p->stream, st); };
    if (dlogits) {
        // The gradient lands in the first-moment slot as m <- m + 1 * (g - m): exact only from m = 0 (1 + (1e-9 - 1) cancels to 0),
        // and a stale second moment would turn the zero-step's 0 * (m / denom) into 0 * inf.  Whatever this handle has trained
        // before, candidate k's m and v planes start from zero here (the header documents them as scratch after this call).
        for (int sel = 1; sel <= 2; ++sel)
            HIPCHK(hipMemsetAsync(p->plane.get() + sel * pl.plane_stride + pl.cand_plane_base[k], 0, sizeof(float) * (size_t)pl.cand_plane_size[k], p->stream));
    }
    // 1. forward partial sums of the batch (no update): the sweep's forward half over this candidate's units
    sweep();
    // 2. the chain (running statistics move like in any train-mode forward): stops at the logits, or goes on from the caller's dL/dlogits and leaves dy_i for the sweep
    st.ca = ca;
    launch(chain_build(single_batch_chain_key(plan_facts(pl))).fn, 1u, pl.lds_chain, p->stream, st.ca);
    if (dlogits) {   // 3. dW of every matrix into its m slot (see the header comment); W, v-scaled-by-lr-0 steps leave W as it was
        st.sa.do_update = 1; st.sa.do_forward = 0;
        sweep();
        tap_grad_launch(pl, p->plane.get(), p->stepbuf.get(), k, nrows, tg, p->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MFAS_OK;
}
