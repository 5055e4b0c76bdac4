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
from tests import test_gpu_ref64 as G
from tests import test_gpu_train_ref64 as GT
from tests import test_gpu_wide_ref64 as GW
from tests.test_gpu_ref64 import dev  # noqa: F401

pytestmark = pytest.mark.gpu

FULL = 5                            # full batches of the train table: nb = 6
STEPS = (1, 2, 3, 5, 6, 7)
LATE = (5, 6, 7)
# parameters, taps and orders of row i are drawn from SEED0 + i: a base on which test_resident_cpu.py's calibration holds for every
# row (TAU_RUNSTAT's margin is narrow, see SEED0 in test_gpu_train_ref64.py)
SEED0 = 7000

# tap widths: 9 / 17 / 65 are no multiple of 16; 600, 1000 and 3000 pad to 608 = 16 * 38, 1008 = 16 * 63 and 3008 = 16 * 188, which cut into
# odd chunks (at 256 columns: 19 units of 32, 7 of 144, 47 of 64); 1008 is the WIDE unit at a chunk of 1024
W_R = dict(s=(9, 600, 2048, 1000), v=(17, 65, 1000, 3000))
# populations: mixed depths 1..4, all three nonlinearities
POP_A = [[[0, 1, 0], [2, 0, 1]], [[3, 2, 2]], [[1, 1, 1], [0, 2, 0], [2, 1, 2], [3, 0, 1]]]
POP_B = [[[1, 2, 2], [3, 1, 0], [0, 0, 1]], [[2, 2, 0]]]
POP_W = [[[3, 2, 0], [0, 0, 1]], [[2, 1, 2]], [[1, 3, 1], [3, 0, 0], [0, 2, 2], [2, 2, 1]]]
# more than 256 - K units at 256 columns, at most twice that: two units per workgroup (each 3000-wide tap is 47 units)
POP_N = [[[2, 3, 0], [1, 3, 1]], [[3, 3, 2]], [[0, 3, 1], [2, 2, 0], [3, 3, 2]], [[1, 3, 0]]]
POP_M = [[[1, 3, 2]], [[0, 3, 0], [3, 3, 1], [2, 0, 2], [1, 3, 0]], [[2, 3, 1], [0, 1, 0]], [[3, 3, 0], [1, 2, 2], [1, 3, 1]], [[0, 0, 2]]]

# (id, R, C, B, widths, confs, hyper flags, table dtype, tap_bits, chunk_cols, K)
# flags: bn / drpt0 / alphas / multitask / lm1 (loss_mode 1 with pos_weight); drpt is 0.5 unless drpt0
RESIDENT_BUILDS = [
    ("mb1-plain0-f32-nu1", 16, 60, 16, W_R, POP_A, "alphas,bn", "float32", 0, 0, 3),
    ("mb1-plain0-f32-nu2", 11, 23, 7, W_R, POP_N, "multitask,bn", "float32", 32, 0, 4),
    ("mb1-plain0-x16-nu1", 16, 64, 7, W_R, POP_B, "lm1", "bfloat16", 16, 512, 2),
    ("mb1-plain0-x16-nu2", 8, 5, 16, W_R, POP_M, "alphas", "float16", 0, 0, 5),
    ("mb1-plain0-x16-wide", 16, 17, 16, W_R, POP_W, "multitask,bn,drpt0", "bfloat16", 16, 1024, 3),
    ("mb1-plain1-f32-nu1", 16, 60, 7, W_R, POP_B, "", "float32", 32, 128, 2),
    ("mb1-plain1-f32-nu2", 16, 23, 16, W_R, POP_M, "", "float32", 0, 0, 5),
    ("mb1-plain1-x16-nu1", 11, 64, 16, W_R, POP_A, "", "float16", 16, 0, 3),
    ("mb1-plain1-x16-nu2", 16, 5, 7, W_R, POP_N, "", "bfloat16", 16, 0, 4),
    ("mb1-plain1-x16-wide", 8, 17, 7, W_R, POP_W, "", "float16", 16, 1024, 3),
    ("mb1-plain2-f32-nu1", 8, 60, 16, W_R, POP_A, "bn,drpt0", "float32", 0, 512, 3),
    ("mb1-plain2-f32-nu2", 16, 23, 7, W_R, POP_N, "bn", "float32", 32, 0, 4),
    ("mb1-plain2-x16-nu1", 16, 64, 7, W_R, POP_B, "bn", "bfloat16", 0, 0, 2),
    ("mb1-plain2-x16-nu2", 11, 5, 16, W_R, POP_M, "bn,drpt0", "float16", 16, 0, 5),
    ("mb1-plain2-x16-wide", 16, 17, 16, W_R, POP_W, "bn", "bfloat16", 16, 1024, 3),
    ("mb2-plain0-f32-nu1", 16, 60, 20, W_R, POP_B, "multitask,bn,drpt0", "float32", 32, 0, 2),
    ("mb2-plain0-f32-nu2", 16, 23, 32, W_R, POP_M, "lm1", "float32", 0, 0, 5),
    ("mb2-plain0-x16-nu1", 11, 64, 32, W_R, POP_A, "alphas,bn,drpt0", "float16", 16, 0, 3),
    ("mb2-plain0-x16-nu2", 16, 5, 20, W_R, POP_N, "multitask,bn", "bfloat16", 16, 0, 4),
    ("mb2-plain0-x16-wide", 16, 17, 20, W_R, POP_W, "lm1,bn", "float16", 16, 1024, 3),
    ("mb2-plain1-f32-nu1", 16, 60, 20, W_R, POP_A, "", "float32", 0, 512, 3),
    ("mb2-plain1-f32-nu2", 8, 23, 32, W_R, POP_N, "", "float32", 32, 0, 4),
    ("mb2-plain1-x16-nu1", 16, 64, 32, W_R, POP_B, "", "bfloat16", 0, 128, 2),
    ("mb2-plain1-x16-nu2", 16, 60, 20, W_R, POP_M, "", "float16", 16, 0, 5),
    ("mb2-plain1-x16-wide", 11, 17, 32, W_R, POP_W, "", "bfloat16", 16, 1024, 3),
    ("mb2-plain2-f32-nu1", 11, 60, 32, W_R, POP_B, "bn", "float32", 32, 0, 2),
    ("mb2-plain2-f32-nu2", 16, 23, 20, W_R, POP_M, "bn,drpt0", "float32", 0, 0, 5),
    ("mb2-plain2-x16-nu1", 16, 64, 20, W_R, POP_A, "bn", "float16", 16, 512, 3),
    ("mb2-plain2-x16-nu2", 8, 5, 32, W_R, POP_N, "bn", "bfloat16", 0, 0, 4),
    ("mb2-plain2-x16-wide", 16, 17, 20, W_R, POP_W, "bn,drpt0", "float16", 16, 1024, 3),
]
BUILD_IDS = [r[0] for r in RESIDENT_BUILDS]
FORMS = ("f32-nu1", "f32-nu2", "x16-nu1", "x16-nu2", "x16-wide")
ALL_BUILDS = [f"mb{mb}-plain{plain}-{form}" for mb in (1, 2) for plain in (0, 1, 2) for form in FORMS]
# the rows that also train one epoch with the 83-row dev table (the dev pass reads what the resident launch stored): one per PLAIN
DEV_ROWS = ("mb2-plain0-x16-nu2", "mb2-plain1-x16-nu1", "mb1-plain2-f32-nu2")
# Per-case taus where the float32 oracle itself exceeds a quarter of the project's tau on the case's inputs
# (tests/test_resident_cpu.py): four times the oracle's measured maximum, rounded up.  {id: {quantity: (tau, measured)}}
CASE_TAUS = {}


def case_taus(rid):
    taus = dict(GT.TAUS)
    taus.update({q: float(tau) for q, (tau, _) in CASE_TAUS.get(rid, {}).items()})
    return taus


def base_case(row, cells=None):
    """The 9-tuple test_gpu_ref64's helpers take: (id, R, C, B, widths, cells, bn, drpt, extra)."""
    rid, R, C, B, w, confs, flags = row[:7]
    fl = set(filter(None, flags.split(",")))
    extra = ",".join(sorted(fl & {"alphas", "multitask", "lm1"}))
    return (rid, R, C, B, w, confs[0] if cells is None else cells, "bn" in fl, 0.0 if "drpt0" in fl else 0.5, extra)


def row_order_mode(rid):
    return ("shared", "per_candidate")[BUILD_IDS.index(rid) % 2]


def president_name(rid):
    """The launch record's name of a RESIDENT_BUILDS row: k_president<MB, tiles per wave, 16-bit staging, units per workgroup, PLAIN> —
    four tiles per wave (PERSIST_NTR), eight for the wide unit (PERSIST_NTR16)."""
    mb, plain, form = rid.split("-", 2)
    ntr, x16, nu = {"f32-nu1": (4, 0, 1), "f32-nu2": (4, 0, 2), "x16-nu1": (4, 1, 1), "x16-nu2": (4, 1, 2), "x16-wide": (8, 1, 1)}[form]
    return f"k_president<{mb[2:]},{ntr},{x16},{nu},{plain[5:]}>"


def assert_president_record(pop, rids, tag):
    """The library's record of the population's last train call: one of the builds `rids` name, launched, and nothing else."""
    rec = pop.launch_record()
    assert len(rec) == 1 and set(rec) <= {president_name(r) for r in rids} and all(n > 0 for n in rec.values()), (tag, rec)


def resident_schedule(hp, confs, chunk_cols, sched=None, device="cuda:0"):
    """pop.schedule() (or, without a population, the plan query's answer) with the chunk the plan cut the feature segments with and
    the widest unit that gives: a tap of padded width w is cut into units of the largest multiple of 16 that divides w and does
    not exceed the chunk (plan.hip.h: pick_chunk)."""
    from mfas_amd.engine import plan_population
    plan = plan_population(hp, confs, device, chunk_cols)
    out = dict(plan if sched is None else sched)
    out["chunk_cols"] = plan["chunk_cols"]
    used = {GW.ceil16(hp.s_sizes[c[0]]) for conf in confs for c in conf} | {GW.ceil16(hp.v_sizes[c[1]]) for conf in confs for c in conf}
    out["widest_unit"] = max(GW.pick_chunk(w, plan["chunk_cols"]) for w in used)
    out["compute_units"] = plan["compute_units"]
    return out


def build_inputs(row):
    """What a RESIDENT_BUILDS row trains, as numpy (no device)."""
    from tests.helpers import engine_hyper
    rid, R, C, B, w, cells, flags, dtype, tap_bits, cc, K = row
    seed = SEED0 + BUILD_IDS.index(rid)
    hp = G.case_hyper(base_case(row))
    confs, p0s = [], []
    for k, c in enumerate(cells):
        conf, p0 = G.case_params(base_case(row, c), hp, seed + 10 * k)
        confs.append(conf)
        p0s.append(p0)
    ehp = engine_hyper(hp)
    ehp.tap_bits = tap_bits
    ehp.order_per_candidate = row_order_mode(rid) == "per_candidate"
    N = GT.train_rows(B, FULL)
    t = G.case_table(base_case(row), hp, N, seed, dtype)
    order = GT.make_order(N, seed, K if ehp.order_per_candidate else None)
    return dict(hp=hp, ehp=ehp, confs=confs, seeds=[seed + 3 * k for k in range(K)], p0s=p0s, N=N, t=t, dtype=dtype, order=order,
                etas=GT.step_etas(N, B), seed=seed)


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


LATE_WIDE = ("wb65", "w177")
LATE_PARAMS = [(name, mode) for name in GT.TRAIN_SCHEDULES for mode in ("shared", "per_candidate")] + \
              [(cid, "per_candidate" if cid in GW.PER_CANDIDATE else "shared") for cid in LATE_WIDE]


@pytest.mark.gpu
@pytest.mark.parametrize("name,order_mode", LATE_PARAMS, ids=[f"{n}-{m}" for n, m in LATE_PARAMS])
def test_late_steps_vs_ref64(dev, name, order_mode):
    """The train schedules of test_gpu_train_ref64.py and two wide cases on a table of six batches: the fifth full batch, the
    ragged sixth and the first of epoch 1 against ref64 (steps 1..3 are held by those files)."""
    if name in LATE_WIDE:
        GW.run_train_steps(dev, GW.WIDE_CASES[GW.WIDE_IDS.index(name)], order_mode, FULL, LATE, "late/wide")
    else:
        GT.run_schedule(dev, name, order_mode, FULL, LATE, "late/schedules")
