"""Every build of the resident step loop (k_president, persist.hip.h) and the late steps of every other train schedule against the
float64 reference (tests/ref64.py), one step at a time and element by element (test_gpu_train_ref64.py's check and taus).

The resident loop is the schedule the search runs (R <= 16, B = 20, 6-16 candidates per GPU).  It keeps W / m / v in registers for a
whole launch, stages the rows of batch t + 2 right after step t and stores the state back only at the launch's end; its kernel is
built thirty times: MB in {1, 2} x PLAIN in {0 general chain, 1 search default, 2 BatchNorm alone} x five unit forms (f32 staging
with one or two units per workgroup, 16-bit staging with one or two, one 16-bit WIDE unit of up to 1024 columns).  RESIDENT_BUILDS
has one row per build; every test asserts that the library's own launch record (Population.launch_record()) names the build its id
spells (president_name) and nothing else after it has trained, and that the population still runs the resident schedule afterwards (a
launch whose grid was not resident at once would have handed the population to launch-per-phase).  tests/test_resident_cpu.py holds
the same ids to the choice of builds.hip.h (president_key) without a device.

The train table has N = 5 B + r rows (nb = 6 batches) and steps (1, 2, 3, 5, 6, 7) are checked: 1..3 as in the sibling files
(batch 0, batch 1, batch 2 — the first whose rows were staged inside the step loop), step 5 the fifth full batch of one launch (rows
staged at step 3, state four steps in registers), step 6 the ragged last batch, step 7 batch 0 of epoch 1's launch, read from
what epoch 0's launch stored back.  The same N and steps (5, 6, 7) go to the nine launch-per-phase schedules and two wide cases.

tests/test_resident_cpu.py holds the float32 oracle under a quarter of every tau on exactly these inputs, checks that the table
covers the thirty builds, and makes two errors of a step loop (a staging buffer that is not refilled, an order offset that wraps
after two batches) pass on steps (1, 2, 3) and fail on (5, 6, 7).

Worst ratio over all steps, candidates and elements of a group (-s prints the table of the run; test_resident_cpu.py prints the
float32 oracle's on the same inputs on the CPU).  The MI355X column, the test count and the wall time are NOT recorded yet: this
file has not run on a device yet; the CPU column is measured.

  group                     float32 oracle on the CPU: m (20) / v (1) / w (20) / runstat (4) / loss (1)      MI355X
  plain0  f32-nu1           0.68 / 0.17 / 3.65 / 0.81 / 0.0006                                               -
  plain0  f32-nu2           0.96 / 0.18 / 3.91 / 0.80 / 0.010                                                -
  plain0  x16-nu1           0.85 / 0.18 / 3.34 / 0.78 / 0.003                                                -
  plain0  x16-nu2           0.88 / 0.18 / 3.76 / 0.78 / 0.010                                                -
  plain0  x16-wide          0.72 / 0.17 / 3.74 / 0.72 / 0.001                                                -
  plain1  f32-nu1           0.87 / 0.18 / 3.58 / -    / 0.024                                                -
  plain1  f32-nu2           0.88 / 0.18 / 3.66 / -    / 0.016                                                -
  plain1  x16-nu1           0.83 / 0.18 / 3.41 / -    / 0.016                                                -
  plain1  x16-nu2           0.95 / 0.18 / 3.62 / -    / 0.023                                                -
  plain1  x16-wide          0.80 / 0.18 / 3.18 / -    / 0.017                                                -
  plain2  f32-nu1           0.57 / 0.18 / 3.26 / 0.69 / 0.0009                                               -
  plain2  f32-nu2           0.90 / 0.18 / 4.46 / 0.81 / 0.003                                                -
  plain2  x16-nu1           0.73 / 0.18 / 3.80 / 0.85 / 0.001                                                -
  plain2  x16-nu2           0.84 / 0.18 / 3.65 / 0.81 / 0.0008                                               -
  plain2  x16-wide          0.67 / 0.18 / 3.57 / 0.77 / 0.0007                                               -
  late steps, 9 schedules   0.80 / 0.18 / 2.99 / 0.84 / 0.003                                                -
  late steps, wb65 / w177   0.65 / 0.18 / 3.07 / 0.76 / 0.002                                                -

Run on its own, with a time limit:  python -m pytest tests/test_gpu_resident_ref64.py -m gpu -x -q -s
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import gpu_support as G
from tests import train_gpu as GT
from tests import wide_gpu as GW
from tests.gpu_support import dev  # noqa: F401
from tests.resident_cases import (BUILD_IDS, DEV_ROWS, FULL, LATE, LATE_PARAMS, LATE_WIDE, RESIDENT_BUILDS, STEPS,
                                  assert_president_record, base_case, build_inputs, case_taus)

pytestmark = pytest.mark.gpu


@pytest.mark.gpu
@pytest.mark.parametrize("row", RESIDENT_BUILDS, ids=BUILD_IDS)
def test_resident_builds_steps_vs_ref64(dev, row):
    """One k_president build, asserted by name: K >= 2 candidates, steps 1, 2, 3, 5, 6 and 7 of every candidate against ref64."""
    torch = G._torch()
    from unittest import mock
    from mfas_amd import Population
    rid, cc = row[0], row[9]
    inp = build_inputs(row)
    hp, ehp, confs, p0s, t, dtype = inp["hp"], inp["ehp"], inp["confs"], inp["p0s"], inp["t"], inp["dtype"]
    pop = Population(ehp, confs, dev, drop_seeds=inp["seeds"], chunk_cols=cc)
    try:
        if hp.loss_mode == 1:
            pop.set_pos_weight(G.pos_weight(hp))
        tab = G.gpu_table(t, dtype, dev)
        S, ST = GT.engine_states(pop, tab, p0s, inp["etas"], torch.from_numpy(inp["order"]).to(dev), STEPS)
        assert_president_record(pop, [rid], rid)
        stats = None
        if rid in DEV_ROWS:
            for k, p0 in enumerate(p0s):
                pop.set_state_dict(k, p0)
            tdv = G.case_table(base_case(row), hp, G.N_EVAL, inp["seed"] + 2, dtype)
            stats, status = pop.train(tab, G.gpu_table(tdv, dtype, dev), 1, O.eta_sequence(1e-3, 1e-6, 1, 2, inp["N"] / hp.B, FULL + 1))
            assert not status.any(), (rid, status)
            assert_president_record(pop, [rid], rid)
            after = [G.state_np(pop, k) for k in range(len(confs))]
        assert pop.schedule()["persistent"] == 1, (rid, "a resident launch was given up: the steps ran launch per phase")
    finally:
        pop.close()
    per = ehp.order_per_candidate
    plain_form = rid[4:]
    with mock.patch.dict(GT.TAUS, case_taus(rid)):      # (test_gpu_train_ref64's check reads its module's taus)
        for k, c in enumerate(confs):
            GT.check_candidate(S, ST, k, c, hp, p0s[k], t, inp["order"][k] if per else inp["order"], inp["seeds"][k], inp["etas"],
                               f"{rid} cand {k}", f"resident/{plain_form}", STEPS)
    if stats is not None:
        for k, c in enumerate(confs):
            G.check_dev(stats[k:k + 1], after[k], c, hp, tdv, f"{rid} cand {k} train E=1")


@pytest.mark.gpu
@pytest.mark.parametrize("name,order_mode", LATE_PARAMS, ids=[f"{n}-{m}" for n, m in LATE_PARAMS])
def test_late_steps_vs_ref64(dev, name, order_mode):
    """The train schedules of test_gpu_train_ref64.py and two wide cases on a table of six batches: the fifth full batch, the
    ragged sixth and the first of epoch 1 against ref64 (steps 1..3 are held by those files)."""
    if name in LATE_WIDE:
        GW.run_train_steps(dev, GW.WIDE_CASES[GW.WIDE_IDS.index(name)], order_mode, FULL, LATE, "late/wide")
    else:
        GT.run_schedule(dev, name, order_mode, FULL, LATE, "late/schedules")
