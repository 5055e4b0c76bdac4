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
from tests import test_gpu_ref64 as G
from tests import test_gpu_resident_ref64 as GR
from tests import test_gpu_train_ref64 as GT
from tests import test_gpu_wide_ref64 as GW
from tests.test_axes_cpu import count_spy
from tests.test_gpu_ref64 import W_A, W_C
from tests.test_ref64_cpu import oracle_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = GR.FULL                      # the six-batch train table of test_gpu_resident_ref64.py
STEPS = GR.STEPS                    # (1, 2, 3, 5, 6, 7)
SEED0 = 11000
NATURAL_SEED0 = 11500
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


def named(form, nt):
    return form.replace("N", str(int(nt)))


ALL_BUILDS = [named(f, nt) for f in ALL_FORMS for nt in (0, 1)]
# a form no plan reaches, with the reason: none since k_step<2,N,2,1,1> (a lean chain's launch at MB = 2 always takes WPE = 4) left the table
UNREACHABLE = {}


def plan_states():
    """Every (wide, MB, lean, same_group, chain_split, groups) plan_layout can produce."""
    out = [dict(wide=True, MB=MB, lean=False, same_group=False, chain_split=0, groups=1) for MB in (1, 2, 4)]
    for MB in (1, 2, 4):
        for lean in (False, True):
            for same_group in (False, True):
                for chain_split in (0, 4):
                    for groups in (1, 2):
                        if lean and (MB > 2 or same_group or chain_split):
                            continue
                        if same_group and (MB > 2 or groups == 2):
                            continue
                        if chain_split and (MB != 1 or not (same_group or groups == 2)):
                            continue
                        out.append(dict(wide=False, MB=MB, lean=lean, same_group=same_group, chain_split=chain_split, groups=groups))
    return out


def launch_inputs(st):
    """What the launches of one launch-per-phase epoch hand the choice (launches.hip.h: epoch_launches; train.hip.h: launch_record):
    (has a sweep, has a chain, same-group launch).  The prologue, and a two-group epoch's last launch, are sweeps without a chain; a
    launch without a sweep is the standalone chain."""
    if st["same_group"]:
        return [(1, 0, 0), (1, 1, 1)]
    if st["groups"] == 1:
        return [(1, 0, 0), (0, 1, 0)]
    return [(1, 0, 0), (0, 1, 0), (1, 1, 0)]


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


# ------------------------------------------------------------------------------------------------ the rows
# candidates: different depths and nonlinearities.  BatchNorm populations keep to two cells (a deeper BatchNorm stack leaves most
# rows of a train batch ambiguous in ref64 itself); the others go to four.
POP_BN = [[[3, 3, 0], [1, 2, 1]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1]]]
POP_DEEP = [[[3, 3, 0], [1, 2, 1], [0, 0, 2]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1], [1, 1, 0], [2, 2, 2]]]
WB65 = GW.WIDE_CASES[GW.WIDE_IDS.index("wb65")]          # B = 65: the smallest batch that is wide
POP_WIDE = [GW.POOL[2], GW.POOL[1], [[2, 0, 0], [0, 2, 1]]]


def _row(rid, target, family, R, C, B, widths, confs, flags, env, cc, facts, forms):
    return dict(id=rid, target=target, family=family, R=R, C=C, B=B, widths=widths, confs=confs, flags=flags, env=env, cc=cc,
                facts=facts, forms=set(forms))


def _facts(MB, lean=False, same_group=False, chain_split=0, groups=1, wide=False, over_occ=False):
    return dict(wide=wide, MB=MB, lean=lean, same_group=same_group, chain_split=chain_split, groups=groups, over_occ=over_occ)


# One row per reachable form.  R, C, B and the widths are the smallest at which the form exists (R = 33 / 17 / 11: no multiple of 16;
# R = 113: the first width with eight row blocks, which chain_split needs; B = 7 / 17 / 33 / 65: the first of each batch-tile count with
# a ragged last tile); the same-group rows keep the shapes of test_gpu_ref64.SCHEDULES.  forms: the record the row must leave, chain
# builds included (the prologue, and the last launch of a two-group epoch, are sweeps without a chain: the plain k_step of the MB).
SWEEP_FORMS = [
    _row("step-mb1", "k_step<1,N,4,0,1>", "k_step", 33, 17, 7, W_A, POP_BN, "bn", {"MFAS_GROUPS": "2"}, 0,
         _facts(1, groups=2), ["k_step<1,N,4,0,1>", "k_chain<1,0>"]),
    _row("step-split", "k_step<1,N,4,0,4>", "k_step", 113, 17, 16, W_A, POP_DEEP, "", {"MFAS_GROUPS": "2", "MFAS_SAME_GROUP": "0"}, 0,
         _facts(1, chain_split=4, groups=2), ["k_step<1,N,4,0,4>", "k_step<1,N,4,0,1>", "k_chain<1,0>"]),
    _row("step-mb2-w2", "k_step<2,N,2,0,1>", "k_step", 17, 60, 17, W_A, POP_BN, "bn", {"MFAS_GROUPS": "2"}, 0,
         _facts(2, groups=2), ["k_step<2,N,2,0,1>", "k_step<2,N,4,0,1>", "k_chain<2,0>"]),
    # the same population: every launch with a chain in it now takes the WPE = 4 build, so the WPE = 2 one must be absent
    _row("step-mb2-w4-chain", "k_step<2,N,4,0,1>", "k_step", 17, 60, 17, W_A, POP_BN, "bn", {"MFAS_GROUPS": "2", "MFAS_OCC_BYTES": "0"}, 0,
         _facts(2, groups=2, over_occ=True), ["k_step<2,N,4,0,1>", "k_chain<2,0>"]),
    _row("step-mb4", "k_step<4,N,2,0,1>", "k_step", 17, 17, 33, W_A, POP_DEEP, "", {}, 0,
         _facts(4), ["k_step<4,N,2,0,1>", "k_chain<4,0>"]),
    _row("lean-mb1", "k_step<1,N,4,1,1>", "k_step", 16, 60, 7, W_A, POP_BN, "bn", {"MFAS_PERSIST": "0"}, 0,
         _facts(1, lean=True), ["k_step<1,N,4,1,1>", "k_chain<1,1>"]),
    # two groups: chain_lean runs inside the k_step build (the 128-register one), not only next to it
    _row("lean-mb2", "k_step<2,N,4,1,1>", "k_step", 11, 17, 20, W_A, POP_DEEP, "", {"MFAS_PERSIST": "0", "MFAS_GROUPS": "2"}, 0,
         _facts(2, lean=True, groups=2), ["k_step<2,N,4,1,1>", "k_chain<2,1>"]),
    _row("same-mb1", "k_step_same<1,N,1>", "k_step_same", 128, 60, 16, W_A, POP_BN, "bn", {"MFAS_SAME_GROUP": "2", "MFAS_CHAIN_SPLIT": "0"}, 128,
         _facts(1, same_group=True), ["k_step_same<1,N,1>", "k_step<1,N,4,0,1>"]),
    _row("same-mb2", "k_step_same<2,N,1>", "k_step_same", 65, 17, 20, W_A, POP_DEEP, "", {"MFAS_SAME_GROUP": "2"}, 0,
         _facts(2, same_group=True), ["k_step_same<2,N,1>", "k_step<2,N,4,0,1>"]),
    _row("same-split", "k_step_same<1,N,4>", "k_step_same", 128, 60, 16, W_A, POP_BN, "bn", {"MFAS_SAME_GROUP": "2"}, 128,
         _facts(1, same_group=True, chain_split=4), ["k_step_same<1,N,4>", "k_step<1,N,4,0,1>"]),
    _row("wide", "k_sweep_wide<N>", "k_sweep_wide", WB65[1], WB65[2], WB65[3], WB65[4], POP_WIDE, "bn", {}, 0,
         _facts(4, wide=True), ["k_sweep_wide<N>", "k_chain_wide"]),
]
FORM_IDS = [r["id"] for r in SWEEP_FORMS]
# the rows that also train one epoch with the 83-row dev table under MFAS_NT=1: one per kernel family
DEV_ROWS = ("step-mb2-w2", "same-split", "wide")
MUT_ROWS = ("step-mb1", "same-mb2", "wide")
# Per-row taus where the float32 oracle itself exceeds a quarter of the project's tau on the row's inputs: four times the oracle's
# measured maximum, rounded up.  {id: {quantity: (tau, measured)}}.  None was needed.
CASE_TAUS = {}
# Row i draws from SEED0 + i + 100 * draw.  Draw 0 unless the float32 oracle and ref64 ALONE refuse it (no engine result was looked
# at): the draws listed here are the first on which test_rows_calibration_margin holds, with what the earlier ones failed.
#   step-mb1 (BatchNorm, ragged batch of 3 rows): draws 0 and 1 leave 1 of the 3 rows ambiguous in ref64 (candidate 0)
#   same-mb1 (BatchNorm at R = 128, C = 60):      draw 0 leaves 7 of 16 rows ambiguous, draw 1 3 of the ragged 8 (candidate 0)
ROW_DRAW = {"step-mb1": 2, "same-mb1": 2}


def case_taus(rid):
    taus = dict(GT.TAUS)
    taus.update({q: float(tau) for q, (tau, _) in CASE_TAUS.get(rid, {}).items()})
    return taus


def row_dtype(rid):
    return G.DTYPES[FORM_IDS.index(rid) % 3]


def row_order_mode(rid):
    return ("shared", "per_candidate")[FORM_IDS.index(rid) % 2]


def _inputs(row, seed, dtype, order_mode, full, extra=""):
    """What a row trains, as numpy (no device)."""
    from tests.helpers import engine_hyper
    fl = set(filter(None, row["flags"].split(",")))
    case = lambda cells: (row["id"], row["R"], row["C"], row["B"], row["widths"], cells, "bn" in fl, 0.5, extra)  # noqa: E731
    hp = G.case_hyper(case(row["confs"][0]))
    confs, p0s = [], []
    for k, cells in enumerate(row["confs"]):
        conf, p0 = G.case_params(case(cells), hp, seed + 10 * k)
        confs.append(conf)
        p0s.append(p0)
    K = len(confs)
    ehp = engine_hyper(hp)
    ehp.order_per_candidate = order_mode == "per_candidate"
    N = GT.train_rows(row["B"], full)
    t = G.case_table(case(None), hp, N, seed, dtype)
    order = GT.make_order(N, seed, K if ehp.order_per_candidate else None)
    return dict(hp=hp, ehp=ehp, confs=confs, seeds=[seed + 3 * k for k in range(K)], p0s=p0s, N=N, t=t, dtype=dtype, order=order,
                etas=GT.step_etas(N, row["B"]), seed=seed, case=case(None))


def row_inputs(row, draw=None):
    rid = row["id"]
    draw = ROW_DRAW.get(rid, 0) if draw is None else draw
    return _inputs(row, SEED0 + FORM_IDS.index(rid) + 100 * draw, row_dtype(rid), row_order_mode(rid), FULL)


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


# ------------------------------------------------------------------------------------------------ the natural populations
def plane_floats(R, C, widths, confs):
    """plan.hip.h: plane_stride, the floats of ONE of the three planes W / m / v — per candidate the vector block, per cell the padded
    S, V (and from the second cell on OUT) segments, the head, rounded up to 64."""
    Rp, Cp = GW.ceil16(R), GW.ceil16(C)
    vec = (4 * (5 * Rp + 16) + Cp + 63) // 64 * 64
    tot = 0
    for conf in confs:
        n = vec + Cp * Rp
        for i, c in enumerate(conf):
            n += Rp * (GW.ceil16(widths["s"][c[0]]) + GW.ceil16(widths["v"][c[1]]) + (Rp if i else 0))
        tot += (n + 63) // 64 * 64
    return tot


def state_bytes(R, C, widths, confs):
    """plan.hip.h: GroupPlan::alg_state, 24 bytes per unpadded weight of the candidates' segments."""
    return 24.0 * sum(R * (widths["s"][c[0]] + widths["v"][c[1]] + (R if i else 0)) for conf in confs for i, c in enumerate(conf)) + \
        24.0 * C * R * len(confs)


NT_BYTES = 200.0 * 1024 * 1024      # plan_layout: pl.nontemporal = plane_stride * 12 > 200 MiB
OCC_BYTES_SMALL_R = 250e6           # plan_layout: occ_bytes below eight row blocks (450e6 from R = 113 on)
BIG = [3, 0]                        # W_C's two widest taps: s2048 + v4100 columns per cell


def _big(*nls):
    return [BIG + [nl] for nl in nls]


# natural_nt: R = 128 (the headline's width), B = 16, six candidates of 4, 3, 4, 4, 3 and 4 cells: 17,673,984 floats per plane,
#   212.1 MB of W / m / v against the 209.7 MB (200 MiB) threshold -> nontemporal; one group (fewer than 8 candidates; 423 MB of state
#   is beyond the same-group launch's 260 MB), so the sweep is k_step<1,1,4,0,1>, the headline build, reached by size alone.
#   Its sibling has one cell fewer (the last candidate: 3 cells): 16,869,120 floats, 202.4 MB -> cached.
# natural_occ: R = 80 (five row blocks: occ_bytes = 250 MB; with B in 17..32 the k-split slabs of six or seven row blocks leave the
#   LDS too little room), B = 17, twelve candidates (two groups with no switch from eight on) of 4, 4, 4, 3, 3, 3 | 4, 4, 4, 3, 3, 3 cells:
#   each group 10,432,800 weights = 250.4 MB of state against 250 MB -> the WPE = 4 build also with a chain in the launch; 20,941,056
#   floats per plane, 251.3 MB of planes -> nontemporal: k_step<2,1,4,0,1>, and no k_step<2,1,2,0,1>.
_OCC_GROUP = [(0, 1, 2, 0), (1, 2, 0, 1), (2, 0, 1, 2), (0, 2, 1), (1, 0, 2), (2, 1, 0)]
NATURAL = {
    "natural_nt": dict(_row("natural_nt", "k_step<1,N,4,0,1>", "k_step", 128, 60, 16, W_C,
                            [_big(0, 1, 2, 0), _big(1, 2, 0), _big(2, 0, 1, 2), _big(0, 0, 1, 1), _big(2, 1, 0), _big(1, 2, 2, 0)], "", {}, 0,
                            _facts(1), ["k_step<1,N,4,0,1>", "k_chain<1,0>"]), nt=1, dtype="bfloat16", order_mode="per_candidate"),
    "natural_occ": dict(_row("natural_occ", "k_step<2,N,4,0,1>", "k_step", 80, 17, 17, W_C,
                             [_big(*n) for n in _OCC_GROUP] + [_big(*n[::-1]) for n in _OCC_GROUP], "", {}, 0,
                             _facts(2, groups=2, over_occ=True), ["k_step<2,N,4,0,1>", "k_chain<2,0>"]), nt=1, dtype="float16", order_mode="shared"),
}
NATURAL_IDS = list(NATURAL)
NATURAL_STEPS = (1, 2, 3)


def natural_sibling(row):
    """natural_nt with one cell fewer: the last candidate loses its last cell."""
    return dict(row, confs=row["confs"][:-1] + [row["confs"][-1][:-1]])


def natural_inputs(name, row=None):
    row = row or NATURAL[name]
    return _inputs(row, NATURAL_SEED0 + NATURAL_IDS.index(name), row["dtype"], row["order_mode"], 1)


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
