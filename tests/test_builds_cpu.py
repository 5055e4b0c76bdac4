"""mfas_amd/csrc/builds.hip.h on the CPU, over its whole domain: compiled with g++ alone (tests/builds_header.py), asked, and held to
the three statements that replace "create sets the LDS limit of everything":

* containment: every key a choice function returns — step_key, chain_key, president_key, eval_key, the two of single_batch — for any
  plan facts and any launch-time inputs is in plan_keys of those facts (create sets the limit of exactly plan_keys);
* every key of any plan_keys has a row in the kernel tables (the row lists the library compiles into them), and no plan_keys names
  a key twice;
* every table row is in some plan_keys: a dead build cannot come back unnoticed (the k_eval argument combinations no accepted
  geometry reaches are not built; builds.hip.h says why at the row list).

The domain: test_step_builds_cpu.plan_states() x {cached, nontemporal} and the resident plans (the lean chain at MB <= 2, one or two
units per workgroup, narrow or wide units), each with the dev-pass facts of every geometry R <= 512, C <= 256 its chain admits
(test_gpu_ref64.eval_facts: the lean chain has one row block, chain_split eight); the launch-time inputs: the launches of an epoch
(test_step_builds_cpu.launch_inputs) under either occupancy verdict, f32 and 16-bit train tables x the three chain variants, the three
table dtypes x the eight settings of the MFAS_EVAL_NO_* switches.

Two mutations of the header's text — plan_keys loses a key; step_key gives a lean chain's launch at MB = 2 the WPE = 2 build, which
has left the tables — fail these checks."""
import pytest

from oracle import np_oracle as O
from tests import builds_header as BH
from tests import ref64_cases as G
from tests import report_cases as RP
from tests import step_build_cases as SB


def eval_geometries():
    """The distinct dev-pass facts (mbe, nrbw, nrb) of the accepted geometries."""
    out = set()
    for R in range(1, 513):
        for C in range(1, 257, 5):
            out.add(tuple(sorted(G.eval_facts(O.Hyper(R=R, C=C, B=16, s_sizes=G.W_A["s"], v_sizes=G.W_A["v"])).items())))
    return [dict(f) for f in sorted(out)]


def domain():
    """[(facts, launches)]: launches = the (sweep, chain, same) of a launch-per-phase epoch, None for a resident plan."""
    geos = eval_geometries()
    assert {g["nrb"] for g in geos} == set(range(1, 33)) and {g["mbe"] for g in geos} == {4, 2, 1}
    out = []
    for st in SB.plan_states():
        for nt in (0, 1):
            for g in geos:
                if (st["lean"] and g["nrb"] != 1) or (st["chain_split"] and g["nrb"] != 8):
                    continue
                out.append((BH.facts(nt=nt, **st, **g), SB.launch_inputs(st)))
    for MB in (1, 2):
        for nu in (1, 2):
            for wide in (0, 1):
                for nt in (0, 1):
                    for g in geos:
                        if g["nrb"] == 1:
                            out.append((BH.facts(persist=1, lean=1, MB=MB, res_nu=nu, res_wide=wide, nt=nt, **g), None))
    return out


def check_header(mutation=None):
    dom = domain()
    queries, owner = [], []
    for i, (f, launches) in enumerate(dom):
        mine = [("plan", f), ("sb_step", f), ("sb_chain", f)]
        mine += [("eval", f, dtype, sw & 1, sw >> 1 & 1, sw >> 2 & 1) for dtype in (0, 1, 2) for sw in range(8)]
        if launches is None:
            mine += [("president", f, x16, plain) for x16 in (0, 1) for plain in (0, 1, 2)]
        else:
            for sweep, chain, same in launches:
                mine += [("step", f, nch * chain, same, over) for nch in (1, 3) for over in (0, 1)] if sweep else [("chain", f)]
        queries += mine
        owner += [i] * len(mine)
    answers = BH.ask(queries + [("tables", None)], mutation)
    table = answers.pop()
    assert len(set(table)) == len(table) == 72, len(table)
    plans, live = {}, set()
    for q, i, a in zip(queries, owner, answers):
        if q[0] == "plan":
            assert len(set(a)) == len(a), ("plan_keys names a key twice", dom[i][0], a)
            assert set(a) <= set(table), ("plan_keys names a build the tables lack", dom[i][0], set(a) - set(table))
            plans[i] = set(a)
            live |= plans[i]
    for q, i, a in zip(queries, owner, answers):
        if q[0] != "plan":
            assert a in plans[i], ("a launch can choose a build whose LDS limit create has not set", q[0], q[2:], dom[i][0], a)
    assert set(table) == live, sorted(set(table) - live)
    return len(queries)


def test_choices_plan_keys_and_tables_agree():
    assert check_header() > 30000          # (the domain is not empty by accident)


def test_president_plain_over_its_inputs():
    """The chain variant of a resident launch: the search default 1, BatchNorm alone 2, anything else — alphas, multitask, the
    multi-label head, MFAS_NO_PLAIN_CHAIN — the general chain."""
    q = [("plain", None, a, m, lm, bn, no) for a in (0, 1) for m in (0, 1) for lm in (0, 1) for bn in (0, 1) for no in (0, 1)]
    for (_, _, a, m, lm, bn, no), got in zip(q, BH.ask(q)):
        assert got == (0 if a or m or lm or no else 2 if bn else 1), (a, m, lm, bn, no, got)


# name: (text of builds.hip.h, what replaces it, the check that must fail)
MUTATIONS = {
    "plan_keys_drops_the_single_batch_chain": ("    add(single_batch_chain_key(f));\n", "", "LDS limit create has not set"),
    "lean_mb2_takes_wpe2": ("(occ || f.lean_chain)", "occ", "a build the tables lack"),
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_header_mutations_fail(mut):
    old, new, message = MUTATIONS[mut]
    with pytest.raises(AssertionError, match=message):
        check_header((old, new))
