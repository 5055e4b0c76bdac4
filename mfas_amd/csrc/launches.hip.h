// launches.hip.h — the launches of ONE launch-per-phase epoch, in order, as data (host only; plain C++17: no HIP include, no engine type).
// Kernel boundaries carry every dependency of a group g: the forward sums of batch t come from the prologue (t = 0) or sweep(g, t-1);
// chain(g, t) needs them and leaves dy for sweep(g, t) in a LATER launch — same-group plan: in the SAME launch, behind per-cell flags.
// Gathered rows (sweep.hip.h, gather_body; two groups): sweep(g, t) stages batches t and t + 1 from the group's gathered copy, parity =
// batch & 1.  The prologue gathers batches 0 and 1; the launch that carries chain(g, t), t >= 1, gathers batch t + 1: it runs BEFORE
// sweep(g, t) and after sweep(g, t-1), the last reader of batch t - 1, whose parity it overwrites.
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
