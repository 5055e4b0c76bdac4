"""CPU checks for tests/test_gpu_resident_ref64.py (which judges the resident step loop's thirty builds and the late steps of the
other train schedules on the GPU):

* coverage: RESIDENT_BUILDS names exactly the thirty (MB, PLAIN, unit form) builds of k_president, every row's hyper-parameters,
  table dtype and plan (the layout query, a pure host function: 256 compute units without a device) give the build its id names
  through the choice of builds.hip.h itself (president_plain, president_key: compiled with g++ by tests/builds_header.py),
  and the table spans what the design asks for (batch sizes, the three ways into the general chain, depths, nonlinearities, widths);
* calibration: on every row's own inputs and on the late steps of the other schedules the float32 oracle stays under a quarter of
  each tau the GPU test applies (-s prints the worst ratios per group, the figures quoted in the GPU file's docstring);
* two errors of a step loop stay within every tau where train tables have two batches and steps (1, 2, 3) are checked, and exceed
  one on steps (5, 6, 7) of a table of six batches."""
import numpy as np
import pytest

from tests import builds_header as BH
from tests import ref64_cases as G
from tests import resident_gpu as GR
from tests import train_cases as GT
from tests import wide_cases as GW
from tests.oracle32_runs import MUT_CE, oracle_steps, oracle_train_steps

WORST = {}          # group -> {quantity: worst ratio of the float32 oracle}


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


# ------------------------------------------------------------------------------------------------ coverage
def parse(rid):
    mb, plain, form = rid.split("-", 2)
    return int(mb[2:]), int(plain[5:]), form


def test_table_names_the_thirty_builds():
    assert len(GR.RESIDENT_BUILDS) == 30 and sorted(GR.BUILD_IDS) == sorted(GR.ALL_BUILDS) and len(set(GR.BUILD_IDS)) == 30
    assert GR.STEPS == (1, 2, 3, 5, 6, 7) and GR.LATE == (5, 6, 7) and GR.FULL == 5
    ways, depths, nls, modes, bsizes, x16 = {}, set(), set(), set(), set(), []
    for row in GR.RESIDENT_BUILDS:
        rid, R, C, B, w, confs, flags, dtype, tap_bits, cc, K = row
        mb, plain, form = parse(rid)
        fl = set(filter(None, flags.split(",")))
        assert fl <= {"bn", "drpt0", "alphas", "multitask", "lm1"}, rid
        assert K == len(confs) >= 2 and R <= 16 and C <= 64, rid
        assert mb == (1 if B <= 16 else 2) and 2 <= B <= 32, rid
        assert 2 <= GT.ragged_rows(B) <= B - 1, rid
        general = fl & {"alphas", "multitask", "lm1"}
        if plain == 0:
            assert len(general) == 1, rid
            ways.setdefault(general.pop(), set()).add(form)
        else:
            assert not general and ("bn" in fl) == (plain == 2), rid
        if plain == 1:
            assert fl == set(), rid                                     # the search default: no BN, CE, drpt 0.5
        assert "bn" in fl or "drpt0" not in fl, rid                     # (drpt 0 without BatchNorm is no legal cell)
        used = {w["s"][c[0]] for conf in confs for c in conf} | {w["v"][c[1]] for conf in confs for c in conf}
        assert 0 not in used and any(u % 16 for u in used), rid
        if form.startswith("f32"):
            assert dtype == "float32" and tap_bits in (0, 32), rid
        else:
            assert dtype in ("bfloat16", "float16"), rid
            x16.append(dtype)
        if form == "x16-wide":
            assert tap_bits == 16 and cc == 1024 and any(513 <= GW.ceil16(u) <= 1024 for u in used), rid
        depths |= {len(conf) for conf in confs}
        nls |= {c[2] for conf in confs for c in conf}
        modes.add(GR.row_order_mode(rid))
        bsizes.add(B)
    assert ways.keys() == {"alphas", "multitask", "lm1"} and all(len(f) >= 3 for f in ways.values()), ways
    assert depths == {1, 2, 3, 4} and nls == {0, 1, 2} and modes == {"shared", "per_candidate"}
    assert bsizes == {7, 16, 20, 32}
    assert all(a != b for a, b in zip(x16, x16[1:])), x16               # bf16 and f16 alternate down the table
    p2 = [set(r[6].split(",")) for r in GR.RESIDENT_BUILDS if parse(r[0])[1] == 2]
    assert any("drpt0" in f for f in p2) and any("drpt0" not in f for f in p2)
    assert sorted(parse(r)[1] for r in GR.DEV_ROWS) == [0, 1, 2] and set(GR.DEV_ROWS) <= set(GR.BUILD_IDS)


def president_queries(hp, dtype, sched):
    """The two questions a resident launch asks builds.hip.h, from the launch's inputs (train.hip.h: persist_epoch_once): the chain
    variant of the hyper-parameters (no test sets MFAS_NO_PLAIN_CHAIN), and the build for the plan's facts — batch tiles, units per
    workgroup, a widest resident unit of more than 512 columns — and a table that is or is not f32.
    hp: the engine's Hyper; sched: pop.schedule() or plan_population()'s answer, with "widest_unit" (GR.resident_schedule)."""
    f = BH.facts(persist=bool(sched["persistent"] and sched["resident_units"] > 0), MB=-(-hp.B // 16), lean=1,
                 res_wide=sched["widest_unit"] > 512, res_nu=sched["units_per_workgroup"])
    return f, ("plain", None, hp.alphas, hp.multitask, hp.loss_mode, hp.bn, 0), dtype != "float32"


def header_president(hp, dtype, sched):
    """The k_president build a train() call of this population launches, by the record's name, as builds.hip.h chooses it."""
    f, plain_q, x16 = president_queries(hp, dtype, sched)
    assert f["persist"], sched
    return BH.ask1("president", f, x16, BH.ask([plain_q])[0])


@pytest.mark.parametrize("row", GR.RESIDENT_BUILDS, ids=GR.BUILD_IDS)
def test_row_plans_as_the_build_its_id_names(row):
    """The layout query at 256 compute units: resident, the id's units per workgroup and unit width; with the row's
    hyper-parameters and table dtype that is the build the id names.  Two units per workgroup are needed, not chosen."""
    from tests.helpers import engine_hyper
    rid, dtype, cc, K = row[0], row[7], row[9], row[10]
    ehp = engine_hyper(G.case_hyper(GR.base_case(row)))
    ehp.tap_bits = row[8]
    confs = [np.array(c) for c in row[5]]
    sched = GR.resident_schedule(ehp, confs, cc)
    if sched["compute_units"] != 256:       # (a device of another size answers for itself: the GPU test asserts the build there)
        return
    assert header_president(ehp, dtype, sched) == GR.president_name(rid), (rid, sched)
    assert sched["resident_workgroups"] == -(-sched["resident_units"] // sched["units_per_workgroup"])
    assert K + sched["resident_workgroups"] <= 256 and K <= 64, sched
    if rid.endswith("nu2"):
        assert K + sched["resident_units"] > 256, sched
    if rid.endswith("wide"):
        assert 512 < sched["widest_unit"] <= 1024, sched
    else:
        assert sched["widest_unit"] <= 512, sched


def test_president_build_restates_the_launch():
    """builds.hip.h's president_key over the launch's inputs: every one of the thirty builds is reachable and nothing else, each is
    among the builds its plan may launch (plan_keys), and a population that is not resident may launch none."""
    from mfas_amd import Hyper
    seen = set()
    for B in (16, 20):
        for kw in (dict(), dict(bn=True), dict(alphas=True), dict(multitask=True, bn=True), dict(loss_mode=1)):
            hp = Hyper(R=16, B=B, **kw)
            for dtype in G.DTYPES:
                for nu in (1, 2):
                    for widest in (256, 1008):
                        s = dict(persistent=1, resident_units=9, units_per_workgroup=nu, widest_unit=widest)
                        name = header_president(hp, dtype, s)
                        f = president_queries(hp, dtype, s)[0]
                        assert name in BH.ask1("plan", f), (name, f)
                        seen.add(name)
                        for off in (dict(s, persistent=0), dict(s, resident_units=0)):
                            assert not any(k.startswith("k_president") for k in BH.ask1("plan", president_queries(hp, dtype, off)[0])), off
    assert seen == {GR.president_name(b) for b in GR.ALL_BUILDS} and len(seen) == 30, seen ^ {GR.president_name(b) for b in GR.ALL_BUILDS}


# ------------------------------------------------------------------------------------------------ calibration
def assert_quarter(r, taus, tag):
    for q, tau in taus.items():
        assert r[q] * 4.0 <= tau, (tag, q, r[q], tau)
    assert r["count"] == 0.0, tag


@pytest.mark.parametrize("row", GR.RESIDENT_BUILDS, ids=GR.BUILD_IDS)
def test_resident_rows_calibration_margin(row):
    """Every candidate of the row on the row's own table, orders, seeds and steps: the float32 oracle under a quarter of each tau."""
    rid = row[0]
    inp = GR.build_inputs(row)
    per = inp["ehp"].order_per_candidate
    taus = GR.case_taus(rid)
    for k, conf in enumerate(inp["confs"]):
        r = oracle_steps(conf, inp["hp"], inp["p0s"][k], inp["t"], inp["order"][k] if per else inp["order"], inp["etas"],
                         inp["seeds"][k], GR.STEPS, taus, f"{rid} cand {k}")
        note("resident/" + rid[4:], r)
        assert_quarter(r, taus, f"{rid} cand {k}")


@pytest.mark.parametrize("name,order_mode", GR.LATE_PARAMS, ids=[f"{n}-{m}" for n, m in GR.LATE_PARAMS])
def test_late_steps_calibration_margin(name, order_mode):
    """The late steps of the other schedules and of the two wide cases, on the inputs the GPU test trains."""
    if name in GR.LATE_WIDE:
        case = GW.WIDE_CASES[GW.WIDE_IDS.index(name)]
        hp, ehp, seed, confs, p0s, seeds = GW.case_inputs(case, order_mode)
        N, t, order, etas = GW.train_inputs(case, hp, ehp, seed, GR.FULL)
        taus, group = GW.case_taus(name)[1], "late/wide"
    else:
        inp = GT.schedule_inputs(name, order_mode, GR.FULL)
        hp, ehp, confs, p0s, seeds, t, order, etas = (inp[q] for q in ("hp", "ehp", "confs", "p0s", "seeds", "t", "order", "etas"))
        taus, group = GT.TAUS, "late/schedules"
    for k, conf in enumerate(confs):
        r = oracle_steps(conf, hp, p0s[k], t, order[k] if ehp.order_per_candidate else order, etas, seeds[k], GR.LATE, taus,
                         f"{name} {order_mode} cand {k}")
        note(group, r)
        assert_quarter(r, taus, f"{name} {order_mode} cand {k}")


# ------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize("mut", ["stage_lag2", "order_wrap2"])
def test_step_loop_mutations_show_only_on_late_steps(mut):
    """stage_lag2: from the third batch of a launch on, a step reads the rows of batch t - 2 (the staging buffer that was not
    refilled); order_wrap2: batch bi gathers from offset (bi % 2) * B of its order row.  With two batches per epoch and steps
    (1, 2, 3) neither moves anything; with six batches, steps (5, 6, 7) exceed a tau.  The same setups unmutated keep x4."""
    B = MUT_CE[3]
    early = dict(N=GT.train_rows(B), steps=(1, 2, 3))
    late = dict(N=GT.train_rows(B, GR.FULL), steps=GR.LATE)
    for kw in (early, late):
        assert_quarter(oracle_train_steps(MUT_CE, "bfloat16", seed=9, **kw), GT.TAUS, (mut, "unmutated", kw))
    ok = oracle_train_steps(MUT_CE, "bfloat16", mut=mut, seed=9, **early)
    assert all(ok[q] <= tau for q, tau in GT.TAUS.items()) and ok["count"] == 0.0, (mut, ok)
    bad = oracle_train_steps(MUT_CE, "bfloat16", mut=mut, seed=9, **late)
    assert {q: bad[q] for q, tau in GT.TAUS.items() if bad[q] > tau}, (mut, bad)
    for s in GR.LATE[:2]:       # each of the two steps the errors touch (step 7 is batch 0 again) exceeds a tau on its own
        one = oracle_train_steps(MUT_CE, "bfloat16", mut=mut, seed=9, N=late["N"], steps=(s,))
        assert any(one[q] > tau for q, tau in GT.TAUS.items()), (mut, s, one)
