"""Three axes of the C ABI that every other ref64 file holds at one value, against the float64 reference (tests/ref64.py):

* tap slots 4..7 (MFAS_MAX_TAPS is 8 per modality; everything else selects slots 0..3 of four-wide tables): 8 + 8 slots with
  unused ones between used ones, AV-MNIST's 5 + 3 and a 2 + 6 set — gather_tap_off and gather_body's mask of used taps
  (the two-group population with per-candidate orders, the only one whose rows are gathered: it has the 8 + 8 set), plan_layout's grouping by (kind, tap) (tap_major), the tab.s[d.tap] / tab.v[d.tap] reads of the streaming,
  the per-tap, the resident and the wide sweep and of k_eval;
* plain cells (allow_plain_cell, bn = 0, drpt = 0: a cell is [Linear, nl]) on every chain family: lean, resident, the general
  chain at 1 / 2 / 4 m-blocks, same-group, chain_split, two-group, wide — and every dev-pass build of their geometries;
* the hyper-parameter scalars (wd, beta1, beta2, adam_eps, bn_eps, bn_momentum, f1_threshold, the learning rates), four sets with
  every field off its default, among them wd = 0, beta1 = 0, bn_momentum = 1, learning rates of exactly 0 (w must come back
  bit-identical while m and v move) and eta_max = 3e-2, on every train schedule, a wide population and the multi-label head's dev
  pass.  The steps of the 3e-2 set's populations alone are judged with ref64's batch_sum_term (test_axes_cpu.spec_flag).

tests/test_axes_cpu.py holds the designs, the seeds and the inputs (shared by import) and keeps the float32 oracle under a quarter
of every tau on exactly these inputs.  Same rule, same taus as the sibling files: |got - ref64| <= tau 2^-24 M elementwise
(logits 6, gradients 20, running statistics 4; train steps: m 20, v 1, w 20, runstat 4, loss 1); every population's schedule is
asserted by name with pop.schedule(), the resident one's k_president build with the library's launch record.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_axes_ref64.py -m gpu -x -q -s

Observed on the MI355X (131 tests; the run prints the table with -s): worst ratio per quantity, the engine's figure / the float32
oracle's on the same inputs on the CPU (tests/test_axes_cpu.py prints its own with -s).  No kernel or host code had to change.

  group              forward      fwd_train    backward     run_stats    train m      train v      train w      runstat      loss
  (tau)              6            6            20           4            20           1            20           4            1
  tap cases          0.45 / 0.40  0.33 / 0.49  3.91 / 3.72  0.84 / 0.85  0.92 / 0.93  0.18 / 0.18  4.00 / 4.37  0.84 / 0.85  0.014 / 0.014
  tap populations    -            -            -            -            0.88 / 0.87  0.18 / 0.18  3.92 / 4.08  0.84 / 0.87  0.055 / 0.018
  plain populations  0.58 / 0.41  0.31 / 0.38  3.00 / 3.12  -            0.78 / 0.82  0.18 / 0.18  3.84 / 4.14  -            0.028 / 0.018
  scalars sa         0.20 / 0.13  0.005/ 0.008 1.30 / 1.30  0.33 / 0.43  0.40 / 0.40  0.17 / 0.17  3.70 / 3.97  0.58 / 0.79  0.003 / 0.002
  scalars sb         0.14 / 0.14  0.006/ 0.008 1.30 / 1.30  0.36 / 0.44  0.85 / 0.83  0.20 / 0.20  3.56 / 3.76  0.59 / 0.69  0.004 / 0.004
  scalars sc         0.16 / 0.16  0.006/ 0.009 1.30 / 1.30  0.84 / 0.84  1.02 / 1.13  0.18 / 0.18  0 / 0        0.95 / 0.95  0.002 / 0.002
  scalars sd *       0.12 / 0.14  0.005/ 0.006 1.30 / 1.30  0.64 / 0.65  0.88 / 0.89  0.19 / 0.19  3.97 / 4.03  0.80 / 0.80  0.002 / 0.001
  (* the population columns, train m .. loss, with batch_sum_term; the four entry-point columns without)
  (the first four columns of a scalar set are its SCALAR_EVAL_CASES, the others its populations; the eval forward's engine figure
   covers every MFAS_EVAL_NO_* build and row range, the oracle's one pass over the 83 rows)
  dev_loss_sum of the one-epoch calls: 0.013 (CE), 0.050 (multi-label) of its bound.
Every train count lay inside ref64's interval; under set 'sc' (learning rates exactly 0) w came back bit-identical at every step.
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import axes_cases as AX
from tests import gpu_support as G
from tests import resident_cases as GR
from tests import train_gpu as GT
from tests.gpu_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def run_entry_points(dev, case, hp, dtype, seed, rec, steps):
    """The blocks of test_gpu_ref64.py::test_entry_points_vs_ref64 on one candidate — the eval forward over the ragged row ranges
    in every dev-pass build, forward_train + running statistics, backward of arbitrary dlogits, one epoch of train() with a dev
    table — and, with `steps`, steps 1..3 of train() as test_gpu_train_ref64.py checks them."""
    torch = G._torch()
    conf, p0 = G.case_params(case, hp, seed)
    t = G.case_table(case, hp, G.N_EVAL, seed, dtype)
    tab = G.gpu_table(t, dtype, dev)
    tag = f"{case[0]} R{hp.R} C{hp.C} B{hp.B} {dtype} {rec}"
    pop = G.make_pop(hp, conf, dev, seed)
    try:
        assert pop.schedule()["wide"] == (1 if hp.B > 64 else 0), (tag, pop.schedule())
        pop.set_state_dict(0, p0)
        for env in G.eval_envs(hp):
            ep = pop if not env else G.make_pop(hp, conf, dev, seed, env=env)
            try:
                if env:
                    ep.set_state_dict(0, p0)
                G.check_eval_forward(ep, hp, conf, p0, t, tab, tag, rec, env)
            finally:
                if env:
                    ep.close()
        G.check_train_passes(pop, dev, hp, conf, p0, t, tab, seed, tag, rec)
        pop.set_state_dict(0, p0)
        ntr = G.dev_epoch_rows(hp.B)
        ttr = G.case_table(case, hp, ntr, seed + 1, dtype)
        etas = O.eta_sequence(hp.eta_max, hp.eta_min, 1, 2, ntr / hp.B, -(-ntr // hp.B))
        stats, status = pop.train(G.gpu_table(ttr, dtype, dev), tab, 1, etas)
        assert not status.any(), (tag, status)
        G.check_dev(stats, G.state_np(pop), conf, hp, t, f"{tag} train E=1")
        if steps:
            N = GT.train_rows(hp.B)
            ts = G.case_table(case, hp, N, seed, dtype)
            order = GT.make_order(N, seed)
            etas = GT.step_etas(N, hp.B)
            S, ST = GT.engine_states(pop, G.gpu_table(ts, dtype, dev), [p0], etas, torch.from_numpy(order).to(dev))
    finally:
        pop.close()
    if steps:
        GT.check_candidate(S, ST, 0, conf, hp, p0, ts, order, seed, etas, tag, rec)


@pytest.mark.parametrize("dtype", G.DTYPES)
@pytest.mark.parametrize("case", AX.TAP_CASES, ids=AX.TAP_IDS)
def test_tap_slots_entry_points_vs_ref64(dev, case, dtype):
    """Every tap slot 0..7 of both modalities, in cell 0 and in a later cell, over f32 / bf16 / f16 tables: the entry points, the
    one-epoch dev statistics and steps 1..3 of one candidate (t8w: on the wide path)."""
    run_entry_points(dev, case, G.case_hyper(case), dtype, AX.case_seed(case[0]), f"tap/{dtype}", True)


@pytest.mark.parametrize("dtype", G.DTYPES)
@pytest.mark.parametrize("sid", list(AX.SCALAR_SETS))
@pytest.mark.parametrize("case", AX.SCALAR_EVAL_CASES, ids=[c[0] for c in AX.SCALAR_EVAL_CASES])
def test_scalars_in_the_dev_pass_vs_ref64(dev, case, sid, dtype):
    """k_eval's bn_eps and f1_threshold under the multi-label head: the eval forward with its F1 count on every dev-pass build,
    forward_train (bn_eps, bn_momentum in the running statistics), backward, and the dev statistics of one epoch."""
    run_entry_points(dev, case, AX.scalar_case_hyper(case, sid), dtype, AX.AXES_SEED0 + 100 + AX.SCALAR_EVAL_CASES.index(case),
                     f"scalar_eval/{sid}", False)


def check_population_entry_points(dev, pop, inp, tag, rec):
    """Every candidate of a population: the eval forward over the ragged row ranges, forward_train and backward on the 83-row
    table of test_axes_cpu.pop_eval_table; candidate 0 on every other dev-pass build of the geometry; then one epoch with that
    table as the dev table, every candidate's dev statistics."""
    hp, confs, p0s, dtype = inp["hp"], inp["confs"], inp["p0s"], inp["dtype"]
    tdv = AX.pop_eval_table(inp)
    dtab = G.gpu_table(tdv, dtype, dev)
    for k, p0 in enumerate(p0s):
        pop.set_state_dict(k, p0)
    for k, conf in enumerate(confs):
        G.check_eval_forward(pop, hp, conf, p0s[k], tdv, dtab, f"{tag} cand {k}", rec, k=k)
        G.check_train_passes(pop, dev, hp, conf, p0s[k], tdv, dtab, AX.POP_DL_SEED + k, f"{tag} cand {k}", rec, k=k,
                             drop_seed=inp["seeds"][k])
    for env in G.eval_envs(hp)[1:]:
        ep = G.make_pop(hp, confs[0], dev, inp["seeds"][0], env=env)
        try:
            ep.set_state_dict(0, p0s[0])
            G.check_eval_forward(ep, hp, confs[0], p0s[0], tdv, dtab, f"{tag} cand 0", rec, env)
        finally:
            ep.close()
    for k, p0 in enumerate(p0s):
        pop.set_state_dict(k, p0)
    N = inp["N"]
    stats, status = pop.train(G.gpu_table(inp["t"], dtype, dev), dtab, 1, O.eta_sequence(hp.eta_max, hp.eta_min, 1, 2, N / hp.B, -(-N // hp.B)))
    assert not status.any(), (tag, status)
    for k, conf in enumerate(confs):
        G.check_dev(stats[k:k + 1], G.state_np(pop, k), conf, hp, tdv, f"{tag} cand {k} train E=1")


@pytest.mark.parametrize("spec", AX.POPS, ids=AX.POP_IDS)
def test_population_steps_vs_ref64(dev, spec):
    """One population of axes_cases.POPS (a train schedule or the wide path, asserted by name; K >= 3 candidates of different
    depth and nonlinearity): steps 1..3 of every candidate against ref64.  Plain-cell populations also run the entry points and
    the dev pass; a set whose learning rates are exactly 0 leaves w bit-identical while m and v move."""
    torch = G._torch()
    pid, name, mode, axis, key = spec
    inp = AX.pop_inputs(spec)
    entry = AX.pop_entry(name)
    hp, ehp, confs, p0s = inp["hp"], inp["ehp"], inp["confs"], inp["p0s"]
    rec = key if axis == "scalar" else axis
    pop = GT.schedule_pop(name, inp, dev, entry=entry)          # (asserts the schedule with pop.schedule())
    try:
        S, ST = GT.engine_states(pop, G.gpu_table(inp["t"], inp["dtype"], dev), p0s, inp["etas"], torch.from_numpy(inp["order"]).to(dev))
        if name == "persistent":
            GR.assert_president_record(pop, [f"mb2-plain{2 if hp.bn else 1}-{form}" for form in GR.FORMS if form.startswith("x16")], pid)
        if axis == "plain":
            check_population_entry_points(dev, pop, inp, pid, rec)
        if name == "persistent":
            assert pop.schedule()["persistent"] == 1, (pid, "a resident launch was given up: the steps ran launch per phase")
    finally:
        pop.close()
    per = ehp.order_per_candidate
    for k, c in enumerate(confs):
        GT.check_candidate(S, ST, k, c, hp, p0s[k], inp["t"], inp["order"][k] if per else inp["order"], inp["seeds"][k], inp["etas"],
                           f"{pid} cand {k}", rec, batch_sum_term=AX.spec_flag(spec))
    if not inp["etas"].any():
        for k, c in enumerate(confs):
            for j in (1, 2, 3):
                for q in O.trainable_keys(c, hp):
                    assert S[j][k]["w"][q].tobytes() == p0s[k][q].tobytes(), (pid, k, j, q, "w moved at a learning rate of 0")
                assert all(S[j][k][pl]["central_classifier.weight"].tobytes() != S[j - 1][k][pl]["central_classifier.weight"].tobytes()
                           for pl in ("m", "v")), (pid, k, j, "m or v did not move")


def test_plain_cells_are_refused_without_the_flag(dev):
    import dataclasses
    inp = AX.pop_inputs(AX.PLAIN_POPS[0])
    hp = dataclasses.replace(inp["hp"], allow_plain_cell=False)
    with pytest.raises(RuntimeError, match="illegal cell variant"):
        G.make_pop(hp, inp["confs"][0], dev, 1)
