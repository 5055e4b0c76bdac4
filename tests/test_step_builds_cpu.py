"""CPU side of tests/test_gpu_step_builds_ref64.py, which holds every launch-per-phase sweep build — k_step, k_step_same,
k_sweep_wide, cached (NT = 0) and nontemporal (NT = 1) — to the float64 reference and asserts each by the name the library's own
launch record gives it (mfas_population_launch_record).  This file holds the inputs of both (shared by import) and checks, without
a device:

* coverage: ALL_BUILDS is the three sweep tables of the library (14 + 6 + 2 instantiations: the key list builds.hip.h compiles into
  them, printed by tests/builds_header.py's program), the launch's choice is the header's own step_key / chain_key, asked over the plan
  states plan_layout can produce (plan_layout: the lean chain has B <= 32 and neither a same-group launch nor chain_split; the
  same-group launch has B <= 32; chain_split has B <= 16), every build the choice can reach appears in SWEEP_FORMS x {cached,
  nontemporal}, and UNREACHABLE — now empty — would list the rest with the reason;
* every row's expected record follows from the row's plan facts through the header's choice and the launch list (launches.hip.h);
* calibration: on every row's own inputs the float32 oracle stays under a quarter of each tau, the train counts lie inside [lo, hi],
  and ref64 alone leaves at most a quarter of a step's rows ambiguous (the rule and the cap of tests/test_axes_cpu.py);
* the sizes of the two natural populations against the thresholds they are sized by (plan_layout's nontemporal and occ_bytes);
* power: a weight tile whose store of m, of v or of W is dropped at step 2, and a tile that is updated twice at step 2, exceed a tau
  at a checked step on one row of each kernel family.

Seeds.  Row i draws parameters, taps and orders from SEED0 + i (+ 100 per further draw), the natural populations from
NATURAL_SEED0 + i.  Nine of the eleven rows and both natural populations meet every condition on the first draw; two BatchNorm rows
leave more than a quarter of a step's rows ambiguous in ref64 on their first two draws and take the third (ROW_DRAW, with what the
earlier draws failed).  The draws were judged by the float32 oracle and ref64 alone, before any engine result existed; no per-row
tau was needed (CASE_TAUS is empty).

Mutations that do not separate: none — each of the four exceeds a tau at step 2 itself on each of the three rows tried, and none
moves step 1.

-s prints the oracle's worst ratios per kernel family: the CPU figures quoted in the GPU file's docstring.
"""
import os

import numpy as np
import pytest

from tests import builds_header as BH
from tests import ref64_cases as G
from tests import train_cases as GT
from tests import wide_cases as GW
from tests.axes_cases import count_spy
from tests.oracle32_runs import oracle_steps
from tests.step_build_cases import (DEV_ROWS, FORM_IDS, FULL, NATURAL, NATURAL_IDS, NATURAL_STEPS, NT_BYTES, STEPS, SWEEP_FORMS, WB65,
                                    case_taus, launch_inputs, named, natural_inputs, natural_sibling, plan_states, plane_floats,
                                    row_dtype, row_inputs, row_order_mode)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        print("\nfloat32 oracle, worst |got - ref64| / (2^-24 M):")
        for g in sorted(WORST):
            print(f"  {g:24s} " + "  ".join(f"{q} {WORST[g][q]:.3g}" for q in ("m", "v", "w", "runstat", "loss")))


def note(group, r):
    w = WORST.setdefault(group, {})
    for q, v in r.items():
        w[q] = max(w.get(q, 0.0), v)


# ------------------------------------------------------------------------------------------------ the kernel tables
# builds.hip.h: BUILDS_STEP_ROWS (MB, WPE, LEAN, NS), BUILDS_SAME_ROWS (MB, NS), each built cached and nontemporal; the wide sweep
STEP_ROWS = [(1, 4, 0, 4), (1, 4, 0, 1), (2, 2, 0, 1), (2, 4, 0, 1), (4, 2, 0, 1), (1, 4, 1, 1), (2, 4, 1, 1)]
SAME_ROWS = [(1, 1), (2, 1), (1, 4)]
# a build's name as the launch record spells it, with N for the NT argument
ALL_FORMS = [f"k_step<{m},N,{w},{f},{s}>" for m, w, f, s in STEP_ROWS] + [f"k_step_same<{m},N,{s}>" for m, s in SAME_ROWS] + ["k_sweep_wide<N>"]


ALL_BUILDS = [named(f, nt) for f in ALL_FORMS for nt in (0, 1)]
# a form no plan reaches, with the reason: none since k_step<2,N,2,1,1> (a lean chain's launch at MB = 2 always takes WPE = 4) left the table
UNREACHABLE = {}


def form_of(cached, nontemporal):
    """The two names the header gives a launch under NT = 0 and NT = 1, as one form: they differ in the NT argument alone."""
    if cached == nontemporal:
        return cached
    d = [i for i, (a, b) in enumerate(zip(cached, nontemporal)) if a != b]
    assert len(cached) == len(nontemporal) and len(d) == 1 and (cached[d[0]], nontemporal[d[0]]) == ("0", "1"), (cached, nontemporal)
    return cached[:d[0]] + "N" + cached[d[0] + 1:]


def launch_forms(st, over_occ):
    """The builds of one epoch's launches for a plan state as builds.hip.h chooses them (step_key, chain_key), chain builds included."""
    plan = {k: st[k] for k in ("wide", "MB", "lean", "same_group", "chain_split", "groups")}
    queries = []
    for nt in (0, 1):
        f = BH.facts(nt=nt, **plan)
        queries += [("step", f, 3 * chain, same, over_occ) if sweep else ("chain", f) for sweep, chain, same in launch_inputs(st)]
    names = BH.ask(queries)
    n = len(names) // 2
    return {form_of(a, b) for a, b in zip(names[:n], names[n:])}


def test_tables_are_the_sources():
    """ALL_BUILDS is what the library's sweep tables hold: 14 + 6 + 2, in the tables' order."""
    rows = [k for k in BH.ask1("tables", None) if k.startswith(("k_step<", "k_step_same<", "k_sweep_wide<"))]
    assert rows == ALL_BUILDS, (rows, ALL_BUILDS)
    assert len(ALL_BUILDS) == 22 and len(set(ALL_BUILDS)) == 22
    assert sum(b.startswith("k_step<") for b in ALL_BUILDS) == 14 and sum(b.startswith("k_step_same<") for b in ALL_BUILDS) == 6


def test_every_reachable_build_has_a_row():
    """The choice over every plan state reaches ALL_FORMS minus UNREACHABLE (nothing: every build is launched by some plan), names
    nothing the tables lack, and SWEEP_FORMS x {cached, nontemporal} names every reachable build."""
    reach = set()
    for st in plan_states():
        for over in (False, True):
            reach |= {f for f in launch_forms(st, over) if not f.startswith("k_chain")}
    assert reach <= set(ALL_FORMS), reach - set(ALL_FORMS)
    assert set(ALL_FORMS) - reach == set(UNREACHABLE), (set(ALL_FORMS) - reach, set(UNREACHABLE))
    assert list(UNREACHABLE) == []
    covered = {named(f, nt) for row in SWEEP_FORMS for f in row["forms"] if not f.startswith("k_chain") for nt in (0, 1)}
    assert covered == {named(f, nt) for f in reach for nt in (0, 1)}, covered ^ {named(f, nt) for f in reach for nt in (0, 1)}
    assert covered == set(ALL_BUILDS) - {named(f, nt) for f in UNREACHABLE for nt in (0, 1)}
    assert any(row["target"] == "k_step<1,N,4,0,1>" for row in SWEEP_FORMS) and NATURAL["natural_nt"]["forms"] >= {"k_step<1,N,4,0,1>"}


MUT_ROWS = ("step-mb1", "same-mb2", "wide")


def test_rows_span_the_design():
    assert STEPS == (1, 2, 3, 5, 6, 7) and FULL == 5
    assert len(set(FORM_IDS)) == len(SWEEP_FORMS) == 11 and set(DEV_ROWS) | set(MUT_ROWS) <= set(FORM_IDS)
    fam = lambda ids: sorted(SWEEP_FORMS[FORM_IDS.index(i)]["family"] for i in ids)  # noqa: E731
    assert fam(DEV_ROWS) == fam(MUT_ROWS) == ["k_step", "k_step_same", "k_sweep_wide"]
    dtypes, modes, depths, nls = set(), set(), set(), set()
    for row in SWEEP_FORMS:
        rid, B = row["id"], row["B"]
        assert row["target"] in row["forms"] and 3 <= len(row["confs"]), rid
        assert 2 <= GT.ragged_rows(B) <= B - 1, rid
        assert not ("bn" in row["flags"] and max(len(c) for c in row["confs"]) > 2), rid
        assert len({len(c) for c in row["confs"]}) >= 2 and len({c[0][2] for c in row["confs"]}) >= 2, rid
        used = {row["widths"]["s"][c[0]] for conf in row["confs"] for c in conf} | {row["widths"]["v"][c[1]] for conf in row["confs"] for c in conf}
        assert 0 not in used and any(u % 16 for u in used), rid
        dtypes.add(row_dtype(rid))
        modes.add(row_order_mode(rid))
        depths |= {len(c) for c in row["confs"]}
        nls |= {c[2] for conf in row["confs"] for c in conf}
    assert dtypes == set(G.DTYPES) and modes == {"shared", "per_candidate"} and depths == {1, 2, 3, 4} and nls == {0, 1, 2}
    # gather_body (two groups and per-candidate orders) under both builds
    assert any(r["facts"]["groups"] == 2 and row_order_mode(r["id"]) == "per_candidate" for r in SWEEP_FORMS)
    assert (WB65[1], WB65[2], WB65[3]) == (16, 60, 65)


@pytest.mark.parametrize("row", SWEEP_FORMS, ids=FORM_IDS)
def test_row_record_follows_from_its_plan_facts(row):
    """The row's expected record is what the header's choice gives for the row's plan facts, and the facts fit the row: batch tiles
    from B, the lean chain's and chain_split's geometry, the switches that force the schedule.  (The GPU test asserts the facts with
    pop.schedule() and the record with the library's own.)"""
    f, env = row["facts"], row["env"]
    assert launch_forms(f, f["over_occ"]) == row["forms"], (row["id"], launch_forms(f, f["over_occ"]))
    assert any({k: f[k] for k in st} == st for st in plan_states()), row["id"]
    MB = -(-row["B"] // 16)
    assert f["MB"] == (4 if MB >= 3 else MB), row["id"]
    nrb, ncb = -(-row["R"] // 16), -(-row["C"] // 16)
    if not f["wide"]:
        assert row["B"] <= 64
        assert f["lean"] == (nrb == 1 and ncb <= 4 and f["MB"] <= 2), row["id"]
        assert (f["chain_split"] == 4) == (not f["lean"] and f["MB"] == 1 and nrb == 8 and ncb <= 4 and (f["same_group"] or f["groups"] == 2)
                                           and env.get("MFAS_CHAIN_SPLIT") != "0"), row["id"]
        assert (f["groups"] == 2) == (env.get("MFAS_GROUPS") == "2") and f["same_group"] == (env.get("MFAS_SAME_GROUP") == "2"), row["id"]
        assert f["over_occ"] == (env.get("MFAS_OCC_BYTES") == "0"), row["id"]
        assert not f["lean"] or env.get("MFAS_PERSIST") == "0", row["id"]          # (else the resident schedule)
    else:
        assert row["B"] > 64
    assert "MFAS_NT" not in env


def test_layout_query_agrees_where_it_can():
    """mfas_population_plan (a pure host function) under each row's switches: launch per phase, the lean chain and the wide path
    where the facts say so."""
    from mfas_amd.engine import plan_population
    for row in SWEEP_FORMS:
        inp = row_inputs(row)
        os.environ.update(row["env"])
        try:
            plan = plan_population(inp["ehp"], inp["confs"], "cuda:0", row["cc"])
        finally:
            for k in row["env"]:
                os.environ.pop(k, None)
        assert not plan["persistent"] and plan["lean_chain"] == row["facts"]["lean"] and plan["wide"] == row["facts"]["wide"], (row["id"], plan)


def state_bytes(R, C, widths, confs):
    """plan.hip.h: GroupPlan::alg_state, 24 bytes per unpadded weight of the candidates' segments."""
    return 24.0 * sum(R * (widths["s"][c[0]] + widths["v"][c[1]] + (R if i else 0)) for conf in confs for i, c in enumerate(conf)) + \
        24.0 * C * R * len(confs)


OCC_BYTES_SMALL_R = 250e6           # plan_layout: occ_bytes below eight row blocks (450e6 from R = 113 on)


def test_natural_populations_sit_at_their_thresholds():
    nt = NATURAL["natural_nt"]
    n = plane_floats(nt["R"], nt["C"], nt["widths"], nt["confs"])
    assert n == 17673984 and 12.0 * n > NT_BYTES, n
    sib = natural_sibling(nt)
    ns = plane_floats(sib["R"], sib["C"], sib["widths"], sib["confs"])
    assert ns == 16869120 and 12.0 * ns <= NT_BYTES and sum(map(len, sib["confs"])) == sum(map(len, nt["confs"])) - 1, ns
    assert len(nt["confs"]) < 8 and state_bytes(nt["R"], nt["C"], nt["widths"], nt["confs"]) > 260e6      # one group, no same-group launch
    oc = NATURAL["natural_occ"]
    assert 17 <= oc["B"] <= 32 and len(oc["confs"]) >= 8 and -(-oc["R"] // 16) < 8
    # plan_layout: the first group is the shortest prefix with half of the padded weight columns
    work = [sum(GW.ceil16(oc["R"]) * (GW.ceil16(oc["widths"]["s"][c[0]]) + GW.ceil16(oc["widths"]["v"][c[1]]) + (GW.ceil16(oc["R"]) if i else 0))
                for i, c in enumerate(conf)) + GW.ceil16(oc["C"]) * GW.ceil16(oc["R"]) for conf in oc["confs"]]
    split = next(k + 1 for k in range(len(work)) if sum(work[:k + 1]) >= sum(work) / 2)
    assert split == 6
    for grp in (oc["confs"][:split], oc["confs"][split:]):
        b = state_bytes(oc["R"], oc["C"], oc["widths"], grp)
        assert b == 24.0 * 10432800 and OCC_BYTES_SMALL_R < b < 1.02 * OCC_BYTES_SMALL_R, b
    n = plane_floats(oc["R"], oc["C"], oc["widths"], oc["confs"])
    assert n == 20941056 and 12.0 * n > NT_BYTES, n
    for row in NATURAL.values():
        assert launch_forms(row["facts"], row["facts"]["over_occ"]) == row["forms"] and not row["env"]


# ------------------------------------------------------------------------------------------------ calibration
def assert_quarter(r, taus, tag):
    for q, tau in taus.items():
        assert r[q] * 4.0 <= tau, (tag, q, r[q], tau)
    assert r["count"] == 0.0, tag


def calibrate(inp, steps, taus, tag, group):
    per = inp["ehp"].order_per_candidate
    for k, conf in enumerate(inp["confs"]):
        with count_spy() as spy:
            r = oracle_steps(conf, inp["hp"], inp["p0s"][k], inp["t"], inp["order"][k] if per else inp["order"], inp["etas"],
                             inp["seeds"][k], steps, taus, f"{tag} cand {k}")
        note(group, r)
        assert_quarter(r, taus, f"{tag} cand {k}")
        spy.check(f"{tag} cand {k}")


@pytest.mark.parametrize("row", SWEEP_FORMS, ids=FORM_IDS)
def test_rows_calibration_margin(row):
    """Every candidate of the row on the row's own table, orders, seeds and steps: the float32 oracle under a quarter of each tau,
    counts inside [lo, hi], at most a quarter of a step's rows ambiguous."""
    calibrate(row_inputs(row), STEPS, case_taus(row["id"]), row["id"], "builds/" + row["family"])


@pytest.mark.parametrize("name", NATURAL_IDS)
def test_natural_populations_calibration_margin(name):
    calibrate(natural_inputs(name), NATURAL_STEPS, GT.TAUS, name, "builds/natural")


# ------------------------------------------------------------------------------------------------ power
TILE_KEY = "fusion_layers.0.0.weight"       # the first cell's feature weights: rows 0..15 x columns 0..15, one 16 x 16 tile (or all there is)
MUTATIONS = ("drop_m", "drop_v", "drop_w", "twice")


def tile_mutation(mut):
    """At step 2: the tile's store of one plane never happens (the plane keeps what step 1 left there), or the tile is updated a
    second time (the same step again from the state the first update left)."""
    def post(j, prev, new, again):
        if j != 2:
            return new
        out = {pl: {k: v.copy() for k, v in new[pl].items()} for pl in ("w", "m", "v")}
        src = again(new) if mut == "twice" else prev
        for pl in ("m", "v", "w") if mut == "twice" else (mut[-1],):
            out[pl][TILE_KEY][:16, :16] = src[pl][TILE_KEY][:16, :16]
        return out
    return post


@pytest.mark.parametrize("mut", MUTATIONS)
def test_tile_mutations_exceed_a_tau(mut):
    """On one row of each kernel family, candidate 0: unmutated the row keeps x4 (test_rows_calibration_margin); with the mutation a
    checked step exceeds a tau."""
    for rid in MUT_ROWS:
        row = SWEEP_FORMS[FORM_IDS.index(rid)]
        inp = row_inputs(row)
        per = inp["ehp"].order_per_candidate
        taus = case_taus(rid)
        hit = {}
        for s in STEPS[:3]:
            bad = oracle_steps(inp["confs"][0], inp["hp"], inp["p0s"][0], inp["t"], inp["order"][0] if per else inp["order"], inp["etas"],
                               inp["seeds"][0], (s,), taus, f"{rid} {mut}", post=tile_mutation(mut))
            hit[s] = {q: bad[q] for q, tau in taus.items() if bad[q] > tau}
        assert not hit[1] and hit[2], (rid, mut, hit)       # step 1 is untouched; the step that drops or repeats the store shows it
