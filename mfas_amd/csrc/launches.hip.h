// launches.hip.h — the launches of ONE launch-per-phase epoch, in order, as data (host only; plain C++17: no HIP include, no engine type).
// Kernel boundaries carry every dependency of a group g: the forward sums of batch t come from the prologue (t = 0) or sweep(g, t-1);
// chain(g, t) needs them and leaves dy for sweep(g, t) in a LATER launch — same-group plan: in the SAME launch, behind per-cell flags.
// Gathered rows (sweep.hip.h, gather_body; two groups): sweep(g, t) stages batches t and t + 1 from the group's gathered copy, parity =
// batch & 1.  The prologue gathers batches 0 and 1; the launch that carries chain(g, t), t >= 1, gathers batch t + 1: it runs BEFORE
// sweep(g, t) and after sweep(g, t-1), the last reader of batch t - 1, whose parity it overwrites.  (A plan that defers stores — below —
// keeps three sets, set = batch mod 3: a double pass sweep(g, t) still reads batch t - 1, and batch t + 1 overwrites batch t - 2.)
#pragma once
#include <stdint.h>
#include <vector>

struct Launch {
    int sweep_g = -1, upd = 0, fwd = 0;     // group whose sweep the launch carries (-1: none); it updates W / m / v with step sweep_t; it
    int64_t sweep_t = 0;                    // produces forward sums: of batch sweep_t + 1 when it updates, of sweep_t when not (the prologue)
    int chain_g = -1;                       // group whose chain the launch carries (-1: none), at step chain_t
    int64_t chain_t = 0;
    int gather_g = -1, gather_n = 0;        // group whose rows it gathers (-1: none): batches gather_b .. gather_b + gather_n - 1 (1 or 2 sets)
    int64_t gather_b = 0;
    int mode = 0;                           // LAUNCH_PLAIN / _VIRTUAL / _DOUBLE: what the sweep's feature units do with W / m / v (mark_deferred)
};

// ngroups: 1 or 2 candidate groups; same_group: chain and sweep of the one group share a launch; T: train steps of this epoch; gather:
// gathered rows are in use.  (The wide path is "one group, not same-group".)  `out` is reused: no allocation once it has held an epoch.
static void epoch_launches(int ngroups, bool same_group, int64_t T, bool gather, std::vector<Launch>& out) {
    out.clear();
    gather = gather && ngroups == 2;
    auto add = [&](int gs, int upd, int fwd, int64_t ts, int gc, int64_t tc) -> Launch& {
        out.push_back(Launch{gs, upd, fwd, ts, gc, tc});
        return out.back();
    };
    auto rows = [&](Launch& l, int g, int64_t b, int n) { if (gather) { l.gather_g = g; l.gather_b = b; l.gather_n = n; } };
    for (int g = 0; g < ngroups; ++g) rows(add(g, 0, 1, 0, -1, 0), g, 0, T > 1 ? 2 : 1);      // prologue: forward sums of batch 0
    if (ngroups == 1 && same_group) {
        for (int64_t t = 0; t < T; ++t) add(0, 1, t + 1 < T, t, 0, t);                       // chain(t) + sweep(t), per-cell flags
    } else if (ngroups == 1) {
        for (int64_t t = 0; t < T; ++t) { add(-1, 0, 0, 0, 0, t); add(0, 1, t + 1 < T, t, -1, 0); }
    } else {
        add(-1, 0, 0, 0, 0, 0);                                                              // chain(A, 0)
        for (int64_t t = 0; t < T; ++t) {
            const int fwd = t + 1 < T;
            Launch& a = add(0, 1, fwd, t, 1, t);                                             // sweep(A, t)  ||  chain(B, t)
            if (t >= 1 && t + 1 < T) rows(a, 1, t + 1, 1);
            Launch& b = add(1, 1, fwd, t, fwd ? 0 : -1, t + 1);                              // sweep(B, t)  ||  chain(A, t + 1)
            if (fwd && t + 2 < T) rows(b, 0, t + 2, 1);
        }
    }
}

// Deferred stores (two groups, launch per phase).  Nothing reads the stored W / m / v of a feature segment between two sweeps of its
// group — the chain needs only the forward sums, which a sweep makes from the updated tile in its registers — so two consecutive updating
// sweeps of a group share ONE store:
//   virtual (step t):     load version t, update t in registers, forward sums of batch t + 1 from W_{t+1}; W / m / v are NOT stored
//   double  (step t + 1): load version t again, replay update t (x_t, dy_t and the step scalars of t are still there), apply update
//                         t + 1, store version t + 2, forward sums of batch t + 2
// OUT / HEAD units update and store every step whatever the mode: the next launch's chain reads them.
enum { LAUNCH_PLAIN = 0, LAUNCH_VIRTUAL = 1, LAUNCH_DOUBLE = 2 };

// Marks the modes on a finished list: per group its updating sweeps in order, paired (virtual, double); an unpaired sweep stays plain, so
// the LAST updating sweep of a list always stores (the dev pass, the best-epoch copy, resume and get_plane read the planes between
// lists).  The groups are staggered — A pairs steps (0, 1), (2, 3) ..., B keeps step 0 plain and pairs (1, 2), (3, 4) ... — so that every
// pair of consecutive launches holds one short and one long sweep.  One-group and same-group lists keep every sweep plain.
static inline void mark_deferred(int ngroups, bool same_group, std::vector<Launch>& list) {
    for (Launch& l : list) l.mode = LAUNCH_PLAIN;
    if (ngroups != 2 || same_group) return;
    for (int g = 0; g < 2; ++g) {
        Launch* open = nullptr;             // an updating sweep that becomes virtual once the group's next one is there to store for it
        int64_t n = 0;
        for (Launch& l : list) {
            if (l.sweep_g != g || !l.upd) continue;
            if (open) { open->mode = LAUNCH_VIRTUAL; l.mode = LAUNCH_DOUBLE; open = nullptr; }
            else if (n >= g) open = &l;
            ++n;
        }
    }
}

// What a double pass replays must still be there.  Gathered rows: sweep(g, t) in double mode reads the batches t - 1, t and t + 1, and
// the launch that carries chain(g, t + 1) gathers batch t + 2 right after it — three row sets, set = batch mod 3 (two, batch & 1,
// where nothing is deferred).  dy: chain(g, t + 1) runs between sweep(g, t) and sweep(g, t + 1) and must not overwrite the dy_t that
// sweep(g, t + 1) replays — two dy areas, area = step & 1 (one where nothing is deferred).
static inline int row_sets(bool deferring) { return deferring ? 3 : 2; }
static inline int row_set_of(int64_t batch, bool deferring) { return (int)(batch % row_sets(deferring)); }
static inline int dy_area_of(int64_t step, bool deferring) { return deferring ? (int)(step & 1) : 0; }
