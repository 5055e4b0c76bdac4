"""Every launch-per-phase sweep build — k_step, k_step_same, k_sweep_wide, each cached (NT = 0) and nontemporal (NT = 1) — against
the float64 reference (tests/ref64.py), one step at a time and element by element, and each asserted by the name the LIBRARY gives
it: Population.launch_record() (mfas_population_launch_record) is filled where the launches are made, from the same template
instantiation the function pointer comes from, so a wrong row in a kernel table or a wrong choice in step_key (builds.hip.h) shows.

Which of the two builds of a form runs is decided by population size (plan.hip.h: planes above 200 MiB stream nontemporally), which
no other elementwise test reaches: they all run the cached builds.  Here every row of SWEEP_FORMS (tests/test_step_builds_cpu.py:
one row per reachable form, the smallest shapes at which it exists) trains the same inputs twice, under MFAS_NT=0 and MFAS_NT=1, on
the six-batch table of test_gpu_resident_ref64.py, steps (1, 2, 3, 5, 6, 7), and the test asserts
  * the record of every call: exactly the row's builds (chain builds included) with the run's NT, every count > 0;
  * bit identity of the two runs after every call: W, m, v, BatchNorm running statistics, the statistics array, status — one
    arithmetic under -ffp-contract=off, two ways of streaming it;
  * ref64 (test_gpu_train_ref64's check, its taus unchanged: m 20, v 1, w 20, runstat 4, loss 1) for every candidate on the
    nontemporal run; if the two runs differ, on both, so that the message says which side left the reference;
  * for one row per kernel family, one epoch with the 83-row dev table under MFAS_NT=1: the dev pass reads what nontemporal stores wrote.
Two more tests reach the thresholds with NO switch set (populations sized by the threshold: W_C's 2048 + 4100 columns per cell):
natural_nt, 17.7 M floats per plane = 212 MB > 200 MiB, whose record must name k_step<1,1,4,0,1> — the headline build — while the
same population with one cell fewer (202 MB) names k_step<1,0,4,0,1>; natural_occ, B = 17, twelve candidates in two groups of 250.4 MB
of state each (> occ_bytes = 250 MB), whose record must name k_step<2,1,4,0,1> with a chain in the launch and no WPE = 2 build.

tests/test_step_builds_cpu.py holds the inputs, the coverage argument (all 22 instantiations are reachable), the float32 oracle's
calibration on exactly these inputs and the mutations (a tile's dropped store of m / v / W, a tile
updated twice).

Worst ratio over all steps, candidates and elements of a family (-s prints the run's table; the CPU column is the float32 oracle on
the same inputs, tests/test_step_builds_cpu.py -s):

  family         float32 oracle on the CPU: m (20) / v (1) / w (20) / runstat (4) / loss (1)     MI355X, nontemporal run
  k_step         0.89 / 0.178 / 3.34 / 0.826 / 0.014                                              0.77 / 0.180 / 3.76 / 0.826 / 0.017
  k_step_same    0.84 / 0.181 / 3.59 / 0.833 / 0.006                                              0.92 / 0.182 / 3.91 / 0.833 / 0.009
  k_sweep_wide   0.52 / 0.171 / 3.33 / 0.793 / 0.001                                              0.52 / 0.166 / 3.94 / 0.793 / 0.002
  natural        0.99 / 0.183 / 4.62 / -     / 0.005                                              0.99 / 0.183 / 4.55 / -     / 0.007
  dev pass of the three dev rows (fraction of ref64's bound used)                                 0.009

Every figure is below a quarter of its tau.  Worst engine / oracle ratio per quantity over the families: m 1.09 (k_step_same),
v 1.01, w 1.18 (k_sweep_wide), runstat 1.00, loss 1.5 (0.002 against 0.001 of a bound of 1).  All eleven cached / nontemporal pairs
are bit-identical and every record names the builds its row lists, so the cached runs have the same figures.  Nothing had to change
in a kernel or in the dispatch.

test_resident_record_names_the_president_build does the same for the resident loop: the library's record of a two-step call of each
of test_gpu_resident_ref64.py's thirty populations must name that k_president build and nothing else.

Measured on an MI355X (43 tests, 8.4 s for the file on its own, 1.4 s of it the first test's device start-up): a SWEEP_FORMS row
0.04 - 0.52 s (two populations x eight train calls, then ref64 for three candidates x six steps on the CPU), natural_nt 1.8 s,
natural_occ 2.5 s (21 M weights in three planes read back after each of four calls, ref64 on the CPU), a resident row 0.01 - 0.07 s.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_step_builds_ref64.py -m gpu -x -q -s
"""
import pytest

from oracle import np_oracle as O
from tests import gpu_support as G
from tests import resident_cases as GR
from tests import train_cases as GT
from tests import step_build_cases as SB
from tests.gpu_support import dev  # noqa: F401
from tests.step_build_gpu import assert_record, check_ref64, make_pop, train_states

pytestmark = pytest.mark.gpu


def first_difference(a, b):
    """Where two runs' (S, ST) differ byte for byte: (call, candidate, plane, key) or (call, 'statistics'), else None."""
    (Sa, STa), (Sb, STb) = a, b
    for j in sorted(Sa):
        for k in range(len(Sa[j])):
            for pl in ("w", "m", "v"):
                for key, v in Sa[j][k][pl].items():
                    if v.tobytes() != Sb[j][k][pl][key].tobytes():
                        return (f"{j}-step call", f"candidate {k}", pl, key)
        if STa[j].tobytes() != STb[j].tobytes():
            return (f"{j}-step call", "statistics")
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("row", SB.SWEEP_FORMS, ids=SB.FORM_IDS)
def test_sweep_builds_cached_and_nontemporal_vs_ref64(dev, row):
    """One reachable sweep form, both of its builds asserted by the library's record: bit-identical runs, every candidate's steps
    1, 2, 3, 5, 6 and 7 of the nontemporal run against ref64."""
    rid = row["id"]
    inp = SB.row_inputs(row)
    hp = inp["hp"]
    taus = SB.case_taus(rid)
    runs, stats = {}, None
    for nt in (0, 1):
        S, ST, pop, tab = train_states(dev, row, inp, nt, SB.STEPS)
        try:
            if nt == 1 and rid in SB.DEV_ROWS:
                for k, p0 in enumerate(inp["p0s"]):
                    pop.set_state_dict(k, p0)
                tdv = G.case_table(inp["case"], hp, G.N_EVAL, inp["seed"] + 2, inp["dtype"])
                stats, status = pop.train(tab, G.gpu_table(tdv, inp["dtype"], dev), 1, O.eta_sequence(1e-3, 1e-6, 1, 2, inp["N"] / hp.B, SB.FULL + 1))
                assert not status.any(), (rid, status)
                assert_record(row, 1, SB.FULL + 1, pop.launch_record())
                after = [G.state_np(pop, k) for k in range(len(inp["confs"]))]
        finally:
            pop.close()
        runs[nt] = (S, ST)
    diff = first_difference(runs[0], runs[1])
    if diff is not None:
        verdict = {}
        for nt in (0, 1):
            try:
                check_ref64(row, inp, *runs[nt], SB.STEPS, taus, f"NT={nt}")
                verdict[nt] = "stays within ref64"
            except AssertionError as e:
                verdict[nt] = f"leaves ref64: {e}"
        pytest.fail(f"{rid}: the cached and the nontemporal run differ at {diff}; cached {verdict[0]}; nontemporal {verdict[1]}")
    check_ref64(row, inp, *runs[1], SB.STEPS, taus, "NT=1")
    if stats is not None:
        for k, c in enumerate(inp["confs"]):
            G.check_dev(stats[k:k + 1], after[k], c, hp, tdv, f"{rid} NT=1 cand {k} train E=1")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SB.NATURAL_IDS)
def test_natural_thresholds_vs_ref64(dev, name):
    """A population sized by the threshold, no switch set: the record names the nontemporal build (natural_occ: the WPE = 4 build with
    a chain in the launch, and no WPE = 2 build); steps 1..3 of every candidate against ref64.  natural_nt's sibling with one cell
    fewer names the cached build after a one-step call."""
    torch = G._torch()
    row = SB.NATURAL[name]
    inp = SB.natural_inputs(name)
    assert row["nt"] == 1 and not row["env"]
    S, ST, pop, tab = train_states(dev, row, inp, None, SB.NATURAL_STEPS)
    pop.close()
    check_ref64(row, inp, S, ST, SB.NATURAL_STEPS, dict(GT.TAUS), "no switch", "builds/natural")
    if name == "natural_nt":
        sib = SB.natural_sibling(row)
        sinp = dict(inp, confs=inp["confs"][:-1] + [inp["confs"][-1][:-1]])
        pop = make_pop(sib, sinp, dev, None)
        try:
            pop.init(list(range(1, len(sinp["confs"]) + 1)))
            _, status = pop.train(tab, None, GT.EPOCHS, inp["etas"], order=torch.from_numpy(inp["order"]).to(dev), max_steps=1)
            assert not status.any(), status
            assert_record(sib, 0, 1, pop.launch_record())
        finally:
            pop.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", GR.RESIDENT_BUILDS, ids=GR.BUILD_IDS)
def test_resident_record_names_the_president_build(dev, row):
    """The library's own record of a two-step call of each of test_gpu_resident_ref64.py's thirty populations names the build the
    row's id spells and nothing else."""
    torch = G._torch()
    from mfas_amd import Population
    rid, cc = row[0], row[9]
    inp = GR.build_inputs(row)
    pop = Population(inp["ehp"], inp["confs"], dev, drop_seeds=inp["seeds"], chunk_cols=cc)
    try:
        if inp["hp"].loss_mode == 1:
            pop.set_pos_weight(G.pos_weight(inp["hp"]))
        for k, p0 in enumerate(inp["p0s"]):
            pop.set_state_dict(k, p0)
        _, status = pop.train(G.gpu_table(inp["t"], inp["dtype"], dev), None, GT.EPOCHS, inp["etas"],
                              order=torch.from_numpy(inp["order"]).to(dev), max_steps=2)
        rec = pop.launch_record()
        assert not status.any() and pop.schedule()["persistent"] == 1, (rid, status)
    finally:
        pop.close()
    assert set(rec) == {GR.president_name(rid)} and all(n > 0 for n in rec.values()), (rid, rec)
