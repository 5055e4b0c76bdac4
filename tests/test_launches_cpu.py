"""The launch list of a launch-per-phase epoch (mfas_amd/csrc/launches.hip.h, plain C++17) on the CPU: compiled with g++ alone, printed,
and held to two independent checks on every case — the previous hand-written loops, launch for launch, and the data dependencies."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (groups, same_group, gather): one group plain, one group same-group, two groups without / with gathered rows
PLANS = [(1, False, False), (1, True, False), (2, False, False), (2, False, True)]
STEPS = [1, 2, 3, 5]          # T = 1: prologue only feeds one step; 2: first step with a forward; 3: first steady-state gather; 5: several
CASES = [(ng, same, T, gather) for ng, same, gather in PLANS for T in STEPS]
FIELDS = ("sweep_g", "upd", "fwd", "sweep_t", "chain_g", "chain_t", "gather_g", "gather_b", "gather_n")

MAIN = r"""
#include <stdio.h>
#include "launches.hip.h"
int main() {
    const int plans[4][3] = {{1, 0, 0}, {1, 1, 0}, {2, 0, 0}, {2, 0, 1}};
    const long long steps[4] = {1, 2, 3, 5};
    std::vector<Launch> out;          // reused across the cases, like the engine reuses it across epochs
    for (const auto& pl : plans)
        for (long long T : steps) {
            epoch_launches(pl[0], pl[1] != 0, T, pl[2] != 0, out);
            printf("case %d %d %lld %d\n", pl[0], pl[1], T, pl[2]);
            for (const Launch& l : out)
                printf("%d %d %d %lld %d %lld %d %lld %d\n", l.sweep_g, l.upd, l.fwd, (long long)l.sweep_t, l.chain_g, (long long)l.chain_t,
                       l.gather_g, (long long)l.gather_b, l.gather_n);
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """{case: [records]} as the header produces them (compiled once for the module)."""
    d = tmp_path_factory.mktemp("launches")
    (d / "main.cpp").write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "mfas_amd", "csrc"), str(d / "main.cpp"), "-o", str(d / "main")])
    got, cur = {}, None
    for line in subprocess.check_output([str(d / "main")], text=True).splitlines():
        w = line.split()
        if w[0] == "case":
            cur = got.setdefault((int(w[1]), bool(int(w[2])), int(w[3]), bool(int(w[4]))), [])
        else:
            cur.append(tuple(int(x) for x in w))
    return got


def parent_launches(ng, same, T, gather):
    """Transcription of the three loops of train_impl and the two gather conditions of step() as they stood before the launch list
    (commit 999ded2, mfas_hip.hip:1112-1130 and :814-826); use_gather needs two groups (:761)."""
    out = []

    def step(gs, upd, fwd, ts, gc, tc):
        gg, gb, gn = -1, 0, 0
        if gather and ng == 2:
            if gs >= 0 and not upd and fwd and ts == 0:                     # prologue of group gs: batches 0 and 1
                gg, gb, gn = gs, 0, (2 if T > 1 else 1)
            elif gc >= 0 and gs >= 0 and tc >= 1 and tc + 1 < T:            # chain(gc, tc) rides with a sweep: batch tc + 1 of group gc
                gg, gb, gn = gc, tc + 1, 1
        out.append((gs, upd, fwd, ts, gc, tc, gg, gb, gn))

    for gi in range(ng):
        step(gi, 0, 1, 0, -1, 0)
    if ng == 1 and same:
        for t in range(T):
            step(0, 1, 1 if t + 1 < T else 0, t, 0, t)
    elif ng == 1:
        for t in range(T):
            step(-1, 0, 0, 0, 0, t)
            step(0, 1, 1 if t + 1 < T else 0, t, -1, 0)
    else:
        step(-1, 0, 0, 0, 0, 0)
        for t in range(T):
            fwd = 1 if t + 1 < T else 0
            step(0, 1, fwd, t, 1, t)
            step(1, 1, fwd, t, 0 if fwd else -1, t + 1)
    return out


def check_dependencies(launches, ng, same, T, gather):
    """What a launch list owes the kernels, from sweep.hip.h (gather_body, SweepArgs::gather) and DESIGN.md §0 / §4 — from neither
    implementation.  Launch i completes before launch i + 1 starts (one stream); inside a launch only the same-group flags order anything."""
    sweep, chain, produced, gathered = {}, {}, {}, {}
    for i, (gs, upd, fwd, ts, gc, tc, gg, gb, gn) in enumerate(launches):
        if gs >= 0:
            assert 0 <= gs < ng and 0 <= ts < T
            if upd:
                assert (gs, ts) not in sweep, "two updating sweeps of one step"
                sweep[(gs, ts)] = i
            assert upd or fwd, "a sweep that does nothing"
            if fwd:
                batch = ts + 1 if upd else ts
                assert (gs, batch) not in produced, "forward sums produced twice"
                produced[(gs, batch)] = i
        if gc >= 0:
            assert 0 <= gc < ng and 0 <= tc < T and (gc, tc) not in chain, "a chain twice, or of a step the epoch does not have"
            chain[(gc, tc)] = i
        if gs >= 0 and gs == gc:     # sweep and chain of one group in one launch: only the same-group launch, and only of the same step
            assert same and upd and ts == tc, "sweep and chain of the same group share a launch"
        if gg >= 0:
            assert gather and 0 <= gg < ng and gn in (1, 2)
            for b in range(gb, gb + gn):
                assert b < T, "rows gathered for a batch the epoch does not have"
                assert (gg, b) not in gathered, "a batch gathered twice"
                gathered[(gg, b)] = i
        else:
            assert gn == 0
    for g in range(ng):
        for t in range(T):
            assert (g, t) in chain and (g, t) in sweep, "every (group, step) has one chain and one updating sweep"
            assert (g, t) in produced and produced[(g, t)] < chain[(g, t)], "forward sums of batch t strictly before chain(g, t)"
            if t >= 1:
                assert produced[(g, t)] == sweep[(g, t - 1)]
            if same:
                assert chain[(g, t)] == sweep[(g, t)], "same-group plan: chain(g, t) and sweep(g, t) share their launch"
            else:
                assert chain[(g, t)] < sweep[(g, t)], "chain(g, t) strictly before sweep(g, t)"
        assert (g, T) not in produced, "the last updating sweep produces no forward sums"
        for b in range(T if gather else 0):
            # sweep(g, b - 1) stages batch b as x_{t+1}; batch 0 is first read by sweep(g, 0)
            assert (g, b) in gathered and gathered[(g, b)] < sweep[(g, max(b - 1, 0))], "rows of batch b gathered strictly before sweep(g, b - 1)"
            if b >= 2:       # batch b overwrites the parity of batch b - 2, last read by sweep(g, b - 2)
                assert gathered[(g, b)] > sweep[(g, b - 2)], "a parity reused before its last reader"
    assert len(sweep) == len(chain) == ng * T and (gather or not gathered)


@pytest.mark.parametrize("case", CASES, ids=["g%d%s%s-T%d" % (ng, "-same" if same else "", "-gather" if gather else "", T) for ng, same, T, gather in CASES])
def test_launch_list(built, case):
    ng, same, T, gather = case
    want = parent_launches(ng, same, T, gather)
    check_dependencies(want, ng, same, T, gather)          # the checker itself is held to the previous loops alone
    got = built[case]
    assert got == want, "\n".join("%s\n%s" % (g, w) for g, w in zip(got, want) if g != w)
    check_dependencies(got, ng, same, T, gather)


def _late_gather(launches):
    """the last steady-state gather moved to the launch after its own"""
    i = max(j for j, r in enumerate(launches) if r[6] >= 0 and r[1] and launches[j + 1][6] < 0)
    out = list(launches)
    out[i], out[i + 1] = launches[i][:6] + (-1, 0, 0), launches[i + 1][:6] + launches[i][6:]
    return out


def _prologue_two_sets(launches):
    return [r[:8] + (2,) if r[6] >= 0 and not r[1] else r for r in launches]


def _last_sweep_forward(launches):
    i = max(j for j, r in enumerate(launches) if r[0] == 0 and r[1])
    return [r[:2] + (1,) + r[3:] if j == i else r for j, r in enumerate(launches)]


MUTATIONS = {
    "gather_one_launch_late": ((2, False, 3, True), _late_gather),
    "prologue_gathers_two_sets_at_T1": ((2, False, 1, True), _prologue_two_sets),
    "last_sweep_produces_forward_sums": ((1, False, 2, False), _last_sweep_forward),
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_launch_list_mutations(built, mut):
    """Each way a launch list goes wrong fails the dependency check; the same list unmutated passes it."""
    case, mutate = MUTATIONS[mut]
    check_dependencies(built[case], *case)
    bad = mutate(built[case])
    assert bad != built[case]
    with pytest.raises(AssertionError):
        check_dependencies(bad, *case)
