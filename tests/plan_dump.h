// plan_dump.h — the WHOLE LayoutPlan of mfas_amd/csrc/plan.hip.h as text, so that tests/test_plan_cpu.py can pin every descriptor,
// offset, work list and budget of plan_layout() without a device.  One section per part of the plan; structs are written field by
// field, by name (never as bytes: padding must not enter).  mode 0: the `scalars` section in clear, of every other section its record
// count and the 64-bit FNV-1a digest of its text; mode 1: every section in clear (what one diffs when a digest moves).
// Plain C++17 like the header it prints: part of the g++ program of tests/plan_header.py, of no library.
#pragma once
#include <stdarg.h>
#include "plan.hip.h"

struct PlanText {
    std::string out, sec, name;
    int mode = 0;
    long long nrec = 0;
    void f(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char tmp[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(tmp, sizeof(tmp), fmt, ap);
        va_end(ap);
        sec += tmp;
    }
    void begin(const std::string& n) { name = n; sec.clear(); nrec = 0; }
    void rec() { sec += "\n"; ++nrec; }
    void end() {
        unsigned long long h = 1469598103934665603ull;
        for (unsigned char ch : sec) { h ^= ch; h *= 1099511628211ull; }
        char head[160];
        snprintf(head, sizeof(head), "[%s] records=%lld fnv=%016llx\n", name.c_str(), nrec, h);
        out += head;
        if (mode == 1 || name == "scalars") out += sec;
    }
};
// one field by its own name: integers (bools, sizes and 64-bit offsets alike), floating point as %.17g
#define PD_I(s, x) t.f(" " #x "=%lld", (long long)(s).x)
#define PD_D(s, x) t.f(" " #x "=%.17g", (double)(s).x)
#define PD_A(s, x, n) do { t.f(" " #x "="); for (int q_ = 0; q_ < (n); ++q_) t.f("%s%lld", q_ ? "," : "", (long long)(s).x[q_]); } while (0)
#define PD_S(s, x) do { PD_I(s, x); t.rec(); } while (0)       // scalars: one per line
#define PD_SD(s, x) do { PD_D(s, x); t.rec(); } while (0)

static void dump_seg(PlanText& t, const SegDesc& d) {
    PD_I(d, cand); PD_I(d, kind); PD_I(d, cell); PD_I(d, tap); PD_I(d, k0); PD_I(d, cc); PD_I(d, rows_p); PD_I(d, width); PD_I(d, w_off);
    PD_I(d, wt_off); PD_I(d, part_idx); PD_I(d, rows); PD_I(d, cols); PD_I(d, src_off); PD_I(d, src_ld); PD_I(d, src_col0); PD_I(d, init_seed);
    PD_D(d, init_bound); PD_I(d, rb0); PD_I(d, seg_nrb); PD_I(d, sub_kb0); PD_I(d, sub_nkb);
    t.rec();
}
static void dump_segs(PlanText& t, const std::string& name, const std::vector<SegDesc>& v) {
    t.begin(name);
    for (const SegDesc& d : v) dump_seg(t, d);
    t.end();
}
template <typename T>
static void dump_ints(PlanText& t, const char* name, const std::vector<T>& v) {
    t.begin(name);
    for (const T& x : v) { t.f(" %lld", (long long)x); t.rec(); }
    t.end();
}

static void dump_scalars(PlanText& t, const LayoutPlan& pl, int K, int n_cus) {
    const Geo& g = pl.g;
    t.begin("scalars");
    t.f(" K=%d", K); t.rec();
    t.f(" n_cus=%d", n_cus); t.rec();
    t.f(" groups=%d", (int)pl.groups.size()); t.rec();
    PD_S(pl, chunk); PD_S(pl, plane_stride); PD_S(pl, wt_size); PD_S(pl, step_total); PD_SD(pl, bytes_per_launch);
    PD_S(pl, persist); PD_S(pl, res_chain); PD_S(pl, res_wide); PD_S(pl, nres); PD_S(pl, res_nu); PD_S(pl, nres_wg); PD_S(pl, res_buf_words);
    PD_S(pl, wide); PD_S(pl, lean_chain); PD_S(pl, same_group); PD_S(pl, chain_split); PD_S(pl, red_in_sweep); PD_S(pl, nontemporal);
    PD_S(pl, defer); PD_S(pl, sb_dy_alt); PD_SD(pl, occ_bytes); PD_S(pl, mbe); PD_S(pl, nrbw); PD_S(pl, yf_in_lds); PD_S(pl, vec_in_lds);
    PD_S(pl, lds_step); PD_S(pl, lds_chain); PD_S(pl, lds_eval); PD_S(pl, fits_lds); PD_S(pl, lds_split); PD_S(pl, lds_president);
    PD_S(g, R); PD_S(g, C); PD_S(g, Rp); PD_S(g, Cp); PD_S(g, nrb); PD_S(g, ncb); PD_S(g, B); PD_S(g, Bp); PD_S(g, MB);
    PD_S(g, bn); PD_S(g, alphas); PD_S(g, multitask); PD_S(g, use_drop); PD_SD(g, drop_scale); PD_SD(g, bn_eps); PD_SD(g, bn_mom); PD_S(g, drop_thr);
    PD_S(g, sb_part); PD_S(g, sb_dy); PD_S(g, sb_xo); PD_S(g, sb_dlog); PD_S(g, sb_sav); PD_S(g, sb_yf); PD_S(g, sb_gsc); PD_S(g, sb_size);
    PD_S(g, vec_cell_stride); PD_S(g, vec_head);
    PD_A(g, sw, MFAS_MAX_TAPS); t.rec();
    PD_A(g, vw, MFAS_MAX_TAPS); t.rec();
    PD_S(g, loss_mode); PD_SD(g, f1_th); PD_S(g, order_stride);
    const PlanFacts pf = plan_facts(pl);      // (in the order of tests/builds_header.py::FIELDS)
    t.f(" facts=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", (int)pf.wide, (int)pf.MB, (int)pf.lean_chain, (int)pf.same_group, (int)pf.chain_split,
        (int)pf.ngroups, (int)pf.nontemporal, (int)pf.persist, (int)pf.res_wide, (int)pf.res_nu, (int)pf.mbe, (int)pf.nrbw, (int)pf.nrb);
    t.rec();
    t.end();
}

static void dump_cands(PlanText& t, const LayoutPlan& pl) {
    t.begin("cands");
    for (const CandDev& c : pl.cands) {
        PD_I(c, L);
        for (int i = 0; i < MFAS_MAX_CELLS; ++i) {
            t.f(" cell%d:", i);
            PD_A(c, conf[i], 3); PD_A(c, seg_off[i], 3); PD_A(c, seg_cc[i], 3); PD_A(c, seg_cols[i], 3);
        }
        PD_I(c, head_off); PD_A(c, outT_off, MFAS_MAX_CELLS); PD_I(c, headT_off); PD_I(c, vec_off);
        PD_A(c, nch_s, MFAS_MAX_CELLS); PD_A(c, nch_v, MFAS_MAX_CELLS); PD_A(c, part_cell_off, MFAS_MAX_CELLS);
        PD_I(c, step_off); PD_I(c, drop_seed); PD_I(c, gidx); PD_I(c, f_alpha);
        PD_A(c, f_W, MFAS_MAX_CELLS); PD_A(c, f_b, MFAS_MAX_CELLS); PD_A(c, f_bn, MFAS_MAX_CELLS); PD_I(c, f_Wc); PD_I(c, f_bc);
        PD_A(c, K_in, MFAS_MAX_CELLS);
        t.rec();
    }
    t.end();
}

static void dump_group(PlanText& t, const GroupPlan& gr, int gi) {
    const std::string p = "group" + std::to_string(gi);
    t.begin(p + ".head");
    PD_I(gr, c0); PD_I(gr, nc); PD_D(gr, alg_state); PD_D(gr, alg_feat);
    t.rec();
    t.end();
    dump_segs(t, p + ".descs", gr.descs);
    t.begin(p + ".taps");
    for (const TapDesc& d : gr.taps) {
        PD_I(d, kind); PD_I(d, tap); PD_I(d, k0); PD_I(d, cc); PD_I(d, rows_p); PD_I(d, width); PD_I(d, nitems);
        PD_A(d, cand, TAP_MAX_ITEMS); PD_A(d, cell, TAP_MAX_ITEMS); PD_A(d, part_idx, TAP_MAX_ITEMS); PD_A(d, w_off, TAP_MAX_ITEMS);
        t.rec();
    }
    t.end();
}

// The plan of (hp, confs, n_cells, drop_seeds, K, chunk_cols) on a device of n_cus compute units, under the switches of the current
// environment (tuning_from_env, as mfas_population_plan), as text into out.
inline int plan_dump(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells, const uint32_t* drop_seeds, int32_t K,
                     int32_t chunk_cols, int32_t n_cus, int32_t allow_persist, int32_t mode, std::string& out) {
    if (mode != 0 && mode != 1) return fail(MFAS_EINVAL, "unknown mode");
    if (int vrc = validate_inputs(hp, confs, n_cells, K)) return vrc;
    LayoutPlan pl;
    if (int prc = plan_layout(hp, confs, n_cells, drop_seeds, K, chunk_cols, n_cus, allow_persist != 0, tuning_from_env(), pl)) return prc;
    PlanText t;
    t.mode = mode;
    dump_scalars(t, pl, K, n_cus);
    dump_cands(t, pl);
    dump_segs(t, "descs", pl.descs);
    dump_ints(t, "desc_start", pl.desc_start);
    dump_ints(t, "nparams", pl.nparams);
    dump_ints(t, "cand_plane_base", pl.cand_plane_base);
    dump_ints(t, "cand_plane_size", pl.cand_plane_size);
    dump_ints(t, "wide_start", pl.wide_start);
    for (size_t gi = 0; gi < pl.groups.size(); ++gi) dump_group(t, pl.groups[gi], (int)gi);
    dump_segs(t, "pdescs", pl.pdescs);
    dump_ints(t, "need", pl.need);
    dump_ints(t, "role", pl.role);
    out.swap(t.out);
    return MFAS_OK;
}
#undef PD_I
#undef PD_D
#undef PD_A
#undef PD_S
#undef PD_SD
