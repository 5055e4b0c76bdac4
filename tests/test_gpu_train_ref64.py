"""train() against the float64 reference (tests/ref64.py), one step at a time and element by element.

train() zeroes both Adam moments at entry and the engine is deterministic, so train(max_steps=j) for j = 0..3 from the same
initial parameters gives the states S0..S3 (parameters, both moments, BN running statistics).  For every step j >= 1 ref64 takes
the engine's own float32 state S(j-1) as exact inputs, runs ONE train step in float64 (ref64.train_step64: the rows the sample
order selects, dropout at global step j-1, the loss gradient of the head, backward, Adam with L2 weight decay at eta_j) and S(j) is
compared with it: m_j and v_j elementwise, w_j against the Adam formula evaluated on the engine's own m_j and v_j, the running
statistics, the step's train_loss_sum and train_corrects (differences of the j- and (j-1)-step calls' statistics), and status.
Free-running parameters are never compared, so Adam's sign-like first steps cannot produce a false failure.

The train table has N = B + r rows (r = max(2, B // 2)): step 1 is a full batch gathered from scattered rows, step 2 the ragged
final batch (B = 2 admits none: two full batches), which also consumes the forward sums step 1's sweep produced with the updated
W, and step 3 the first step of epoch 1 (its own order row, the eta index and the global dropout step across the epoch boundary).

tau per quantity (units of 2^-24 M; test_ref64_cpu.py holds the float32 oracle under a quarter of each on every case shape
and makes every mutation exceed it):
  * TAU_M = TAU_GRAD: m bounds the same gradient as backward does;
  * TAU_V = TAU_GRAD enters the allowance of v through the gradient's error delta (ref64.adam_step64); v is compared with tau 1
    against that allowance;
  * TAU_W = 14: seven float32 roundings lie between (m_j, v_j, w_{j-1}) and w_j (sqrt, / bc2s, the float32 eps, + eps,
    m / denom, * ss, the subtraction), each at most one 2^-24 of a quantity M_w = |w| + |dw| bounds — the kernel's sqrt and
    divisions are correctly rounded, so 7 is the worst case — taken twice: the float32 oracle reaches 3.2 of them over the case
    shapes and must stay under a quarter of tau;
  * TAU_RUNSTAT and TAU_LOGITS as in test_gpu_ref64.py; the loss is compared with tau 1 against dev_stats' bound.

Observed on the MI355X, worst ratio over all steps, candidates and elements (the run prints the table with -s; 49 tests, 6 s):

  quantity (tau)        cases f32 / bf16 / f16      nine schedules x two order modes
  train_m       (20)    0.90 / 0.91 / 0.99          0.59 .. 0.74
  train_v        (1)    0.18 / 0.18 / 0.18          0.15 .. 0.18
  train_w       (20)    3.95 / 3.85 / 4.17          2.82 .. 3.63
  train_runstat  (4)    0.85 / 0.76 / 0.82          0.62 .. 0.84
  train_loss     (1)    0.006 / 0.010 / 0.006       0.0002 .. 0.002

Every one is below half of its tau and equal, to the second digit, to what the float32 oracle gives on the same inputs on the CPU
(m 0.98, v 0.18, w 4.24, runstat 0.85): the train path computes what the oracle computes, no kernel had to change.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_train_ref64.py -m gpu -x -q -s
"""
import pytest

from tests import gpu_support as G
from tests.gpu_support import CASES, CASE_IDS, case_hyper, case_params, case_table, dev, gpu_table  # noqa: F401
from tests.train_cases import SEED0, TRAIN_SCHEDULES, case_dtype, make_order, ragged_rows, step_etas
from tests.train_gpu import check_candidate, engine_states, run_schedule

pytestmark = pytest.mark.gpu

STEPS = 3      # the steps the tests of this file check: (1, 2, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_train_steps_vs_ref64(dev, case):
    """Every case of the shape envelope, one candidate, one table dtype: steps 1..3 of train() against ref64."""
    torch = G._torch()
    cid = case[0]
    hp = case_hyper(case)
    dtype = case_dtype(cid)
    seed = SEED0 + CASE_IDS.index(cid)
    conf, p0 = case_params(case, hp, seed)
    N = hp.B + ragged_rows(hp.B)
    t = case_table(case, hp, N, seed, dtype)
    order = make_order(N, seed)
    etas = step_etas(N, hp.B)
    pop = G.make_pop(hp, conf, dev, seed)
    try:
        S, ST = engine_states(pop, gpu_table(t, dtype, dev), [p0], etas, torch.from_numpy(order).to(dev))
    finally:
        pop.close()
    check_candidate(S, ST, 0, conf, hp, p0, t, order, seed, etas, f"{cid} R{hp.R} C{hp.C} B{hp.B} {dtype}", dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("order_mode", ["shared", "per_candidate"])
@pytest.mark.parametrize("name", list(TRAIN_SCHEDULES))
def test_train_schedules_steps_vs_ref64(dev, name, order_mode):
    """Every train schedule, asserted with pop.schedule(), K >= 3 candidates of different depth and nonlinearity with their own
    dropout seeds, a shared or a per-candidate sample order: every candidate's steps 1..3 against ref64."""
    run_schedule(dev, name, order_mode, 1, (1, 2, 3), f"{name}/{order_mode}")
