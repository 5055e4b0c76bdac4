"""Deferred stores on the CPU (mfas_amd/csrc/launches.hip.h, mark_deferred and the row-set / dy-area rules; plain C++17, g++ alone): the
marked launch lists of the four plans at T = 1 .. 6, held to what a list owes the kernels — every update reaches the stored state once,
a double pass follows its virtual pass, the last updating sweep stores, and what a double pass replays is still there when it runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (groups, same_group, gather), as tests/test_launches_cpu.py
PLANS = [(1, False, False), (1, True, False), (2, False, False), (2, False, True)]
STEPS = [1, 2, 3, 4, 5, 6]
CASES = [(ng, same, T, gather) for ng, same, gather in PLANS for T in STEPS]
PLAIN, VIRTUAL, DOUBLE = 0, 1, 2

MAIN = r"""
#include <stdio.h>
#include "launches.hip.h"
int main() {
    const int plans[4][3] = {{1, 0, 0}, {1, 1, 0}, {2, 0, 0}, {2, 0, 1}};
    std::vector<Launch> out;
    printf("modes %d %d %d\n", (int)LAUNCH_PLAIN, (int)LAUNCH_VIRTUAL, (int)LAUNCH_DOUBLE);
    for (int d = 0; d < 2; ++d) {
        printf("sets %d %d :", d, row_sets(d != 0));
        for (long long b = 0; b < 8; ++b) printf(" %d", row_set_of(b, d != 0));
        printf(" :");
        for (long long t = 0; t < 8; ++t) printf(" %d", dy_area_of(t, d != 0));
        printf("\n");
    }
    for (const auto& pl : plans)
        for (long long T = 1; T <= 6; ++T) {
            epoch_launches(pl[0], pl[1] != 0, T, pl[2] != 0, out);
            for (Launch& l : out) l.mode = 7;          // (a reused list: mark_deferred owes every record its mode)
            mark_deferred(pl[0], pl[1] != 0, out);
            printf("case %d %d %lld %d\n", pl[0], pl[1], T, pl[2]);
            for (const Launch& l : out)
                printf("%d %d %d %lld %d %lld %d %lld %d %d\n", l.sweep_g, l.upd, l.fwd, (long long)l.sweep_t, l.chain_g, (long long)l.chain_t,
                       l.gather_g, (long long)l.gather_b, l.gather_n, l.mode);
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """({case: [records of ten fields]}, {deferring: (row sets, [set of batch 0..7], [dy area of step 0..7])}), compiled once."""
    d = tmp_path_factory.mktemp("defer")
    (d / "main.cpp").write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "mfas_amd", "csrc"), str(d / "main.cpp"), "-o", str(d / "main")])
    got, rules, cur = {}, {}, None
    for line in subprocess.check_output([str(d / "main")], text=True).splitlines():
        w = line.split()
        if w[0] == "modes":
            assert [int(x) for x in w[1:]] == [PLAIN, VIRTUAL, DOUBLE]
        elif w[0] == "sets":
            a, b, c = line.split(":")
            rules[bool(int(a.split()[1]))] = (int(a.split()[2]), [int(x) for x in b.split()], [int(x) for x in c.split()])
        elif w[0] == "case":
            cur = got.setdefault((int(w[1]), bool(int(w[2])), int(w[3]), bool(int(w[4]))), [])
        else:
            cur.append(tuple(int(x) for x in w))
    return got, rules


def check_deferred(launches, ng, same, T, gather, row_set, dy_area):
    """What a marked list owes the kernels (sweep.hip.h: tile_run's modes, sweep_body's staging).  Launch i ends before launch i + 1
    starts.  A feature tile's stored state is a version number: the count of updates applied to it, in step order."""
    nonplain = [r for r in launches if r[9] != PLAIN]
    if ng != 2 or same:
        assert not nonplain, "one-group and same-group lists defer nothing"
        return
    for g in range(ng):
        stored, applied, replayed, pending = 0, {}, {}, None     # stored version; launches that stored step t; that replayed it; open virtual step
        sweeps = [(i, r) for i, r in enumerate(launches) if r[0] == g and r[1]]
        assert [r[3] for _, r in sweeps] == list(range(T))
        for n, (i, r) in enumerate(sweeps):
            t, mode = r[3], r[9]
            assert mode in (PLAIN, VIRTUAL, DOUBLE)
            if mode == DOUBLE:
                assert pending == t - 1 and stored == t - 1, "a double pass directly follows its virtual pass, on the version that pass loaded"
                replayed[t - 1] = replayed.get(t - 1, 0) + 1
                applied[t - 1] = applied.get(t - 1, 0) + 1
                applied[t] = applied.get(t, 0) + 1
                stored, pending = t + 1, None
            else:
                assert pending is None, "a virtual pass followed by anything but its double pass loses an update"
                assert stored == t, "a sweep loads the version its step starts from"
                if mode == VIRTUAL:
                    assert r[2], "a virtual pass exists for its forward sums"
                    pending = t
                else:
                    applied[t] = applied.get(t, 0) + 1
                    stored = t + 1
        assert pending is None and stored == T, "the last updating sweep stores: the planes hold every step of the epoch"
        assert sweeps[-1][1][9] != VIRTUAL
        assert all(applied.get(t, 0) == 1 for t in range(T)), "every update reaches the stored state exactly once"
        assert all(v <= 1 for v in replayed.values())
        if T >= 2 + g:
            assert any(r[9] == VIRTUAL for _, r in sweeps), "a group with a pair to make defers"
    # staggered: the two launches of a step (sweep(A, t), sweep(B, t)) are never two double passes or two virtual passes
    by_step = {(r[0], r[3]): r[9] for r in launches if r[0] >= 0 and r[1]}
    for t in range(T):
        assert by_step[(0, t)] == PLAIN or by_step[(0, t)] != by_step[(1, t)], "a step's two launches of one kind"
    # what a pass reads is what its producer left: row sets (gathered rows) and dy areas, written and read launch by launch
    rows, dys = {}, {}          # (group, set) -> batch it holds; (group, area) -> step whose dy it holds
    for r in launches:
        gs, updf, fwd, ts, gc, tc, gg, gb, gn, mode = r
        # inside a launch the gather / chain blocks belong to the OTHER group than an updating sweep's, so the order inside does not matter
        # (the prologue's forward-only sweep gathers for its own group and reads the table itself)
        assert gs < 0 or not updf or (gs != gc and gs != gg)
        if gs >= 0 and updf:
            need_rows = [ts] + ([ts + 1] if fwd else []) + ([ts - 1] if mode == DOUBLE else [])
            if gather:
                for b in need_rows:
                    assert rows.get((gs, row_set(b))) == b, "rows of batch %d gone when sweep(%d, %d) mode %d reads them" % (b, gs, ts, mode)
            for t in [ts] + ([ts - 1] if mode == DOUBLE else []):
                assert dys.get((gs, dy_area(t))) == t, "dy of step %d gone when sweep(%d, %d) mode %d reads it" % (t, gs, ts, mode)
        if gg >= 0:
            for b in range(gb, gb + gn):
                rows[(gg, row_set(b))] = b
        if gc >= 0:
            dys[(gc, dy_area(tc))] = tc


IDS = ["g%d%s%s-T%d" % (ng, "-same" if same else "", "-gather" if gather else "", T) for ng, same, T, gather in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_marked_list(built, case):
    got, rules = built
    ng, same, T, gather = case
    nsets, sets, areas = rules[True]
    assert nsets == 3 and rules[False][0] == 2 and rules[False][1] == [b & 1 for b in range(8)] and rules[False][2] == [0] * 8
    check_deferred(got[case], ng, same, T, gather, lambda b: sets[b], lambda t: areas[t])


def test_stagger(built):
    """A pairs (0, 1), (2, 3) ...; B keeps step 0 plain and pairs (1, 2), (3, 4) ...; an unpaired sweep stays plain."""
    got, _ = built
    for T in STEPS:
        modes = {g: [r[9] for r in got[(2, False, T, True)] if r[0] == g and r[1]] for g in (0, 1)}
        want_a = [VIRTUAL, DOUBLE] * (T // 2) + [PLAIN] * (T % 2)
        want_b = [PLAIN] + [VIRTUAL, DOUBLE] * ((T - 1) // 2) + [PLAIN] * ((T - 1) % 2)
        assert modes[0] == want_a and modes[1] == want_b[:T], (T, modes)
        assert all(r[9] == PLAIN for r in got[(2, False, T, True)] if not r[1])


def _virtual_last(launches):
    i = max(j for j, r in enumerate(launches) if r[0] == 0 and r[1])
    return [r[:9] + (VIRTUAL,) if j == i else r for j, r in enumerate(launches)]


def test_mutation_virtual_last_sweep(built):
    got, rules = built
    case = (2, False, 3, True)
    _, sets, areas = rules[True]
    check_deferred(got[case], *case, lambda b: sets[b], lambda t: areas[t])
    with pytest.raises(AssertionError):
        check_deferred(_virtual_last(got[case]), *case, lambda b: sets[b], lambda t: areas[t])


def test_mutation_two_row_sets(built):
    """With the two row sets of a plan that defers nothing, batch t + 1's rows overwrite batch t - 1's before the double pass replays them."""
    got, rules = built
    case = (2, False, 4, True)
    _, sets, areas = rules[True]
    check_deferred(got[case], *case, lambda b: sets[b], lambda t: areas[t])
    with pytest.raises(AssertionError, match="rows of batch"):
        check_deferred(got[case], *case, lambda b: rules[False][1][b], lambda t: areas[t])
    with pytest.raises(AssertionError, match="dy of step"):
        check_deferred(got[case], *case, lambda b: sets[b], lambda t: rules[False][2][t])
