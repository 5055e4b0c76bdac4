"""The single-pass entry points, the dev pass and a few train steps against the float64 reference (tests/ref64.py) across the
shape envelope the library accepts (R 1..512, C 1..128, B 2..64, tap widths 0..4100, f32 / bf16 / f16 tables).

Every comparison is elementwise, |got - ref64| <= tau * 2^-24 * M (ref64.assert_close64), with M the element's own magnitude:
a wrong padded row, ragged tail or small-gradient tile cannot hide under the tensor's maximum.  CASES is a covering design,
not a product: every value of every axis appears in at least two cases, paired differently
(tests/test_ref64_cpu.py::test_gpu_cases_cover_every_axis_value_twice checks that, and calibrates the taus on these shapes).

Run on its own, with a time limit:  python -m pytest tests/test_gpu_ref64.py -m gpu -x -q
"""
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests.gpu_support import check_dev, check_eval_forward, check_train_passes, dev, gpu_table, make_pop, state_np  # noqa: F401
from tests.ref64_cases import (B3_CASES, CASES, CASE_IDS, DTYPES, N_EVAL, SCHEDULES, TAU_LOGITS, TAU_ONE_LAYER, W_A, W_B, case_hyper,
                               case_params, case_table, dev_epoch_rows, eval_envs, feats_of, one_layer_setup)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_entry_points_vs_ref64(dev, case, dtype):
    """forward (eval) over ragged row ranges, forward_train + running statistics, backward of arbitrary dlogits, and one epoch of
    train() with a dev table, against ref64; then (f32, single-label) three train steps against the float32 oracle."""
    cid = case[0]
    hp = case_hyper(case)
    seed = 1000 + CASE_IDS.index(cid)
    conf, p0 = case_params(case, hp, seed)
    t = case_table(case, hp, N_EVAL, seed, dtype)
    tab = gpu_table(t, dtype, dev)
    pop = make_pop(hp, conf, dev, seed)
    pop.set_state_dict(0, p0)
    tag = f"{cid} R{hp.R} C{hp.C} B{hp.B} {dtype}"
    # 1. eval forward: every row range, every dev-pass build the switches select
    for env in eval_envs(hp):
        ep = pop if not env else make_pop(hp, conf, dev, seed, env=env)
        if env:
            ep.set_state_dict(0, p0)
        check_eval_forward(ep, hp, conf, p0, t, tab, tag, dtype, env)
        if env:
            ep.close()
    # 2. forward_train (+ running statistics) and backward of an arbitrary dL/dlogits
    check_train_passes(pop, dev, hp, conf, p0, t, tab, seed, tag, dtype)
    # 3. one epoch of train() with a dev table: the dev statistics on the engine's parameters after the call
    pop.set_state_dict(0, p0)
    ntr = dev_epoch_rows(hp.B)
    ttr = case_table(case, hp, ntr, seed + 1, dtype)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, -(-ntr // hp.B))
    stats, status = pop.train(gpu_table(ttr, dtype, dev), tab, 1, etas)
    assert not status.any(), (tag, status)
    check_dev(stats, state_np(pop), conf, hp, t, f"{tag} train E=1")
    pop.close()
    # 4. f32 tables, single-label head, no BatchNorm: three train steps against the float32 oracle (check_state).  (Under BN the
    #    batch mean removes the fusion bias's gradient: it is round-off sized, and Adam's first steps move such an element by +-lr
    #    whichever sign the round-off has — ref64 pins those gradients above, elementwise.)
    if dtype == "float32" and hp.loss_mode == 0 and not hp.bn:
        from tests.helpers import oracle_steps
        from tests.parity_gpu import check_state
        pop = make_pop(hp, conf, dev, seed)
        pop.set_state_dict(0, p0)
        stats, status = pop.train(gpu_table(ttr, dtype, dev), None, 2, O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, 2 * -(-ntr // hp.B)),
                                  max_steps=3)
        assert not status.any(), (tag, status)
        params, st, _ = oracle_steps(conf, hp, {k: v.copy() for k, v in p0.items()}, ttr, 3, seed=seed)
        check_state(pop, 0, params, st, 3, tag=f"{tag} train steps")
        pop.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("R,cells", B3_CASES)
def test_one_layer_eval_products_vs_ref64(dev, R, cells, dtype):
    """The dev pass's feature products at the scale of one product (identity head), weights with all 24 significand bits: the
    default build (bf16 x 3 over bf16 tables) and the f32-product build both against ref64.  A product build that dropped the
    low 8 weight bits sits 35..180 x 2^-24 M away (test_ref64_cpu.py::test_mutation_b3_without_lo_term)."""
    hp, conf, p, t = one_layer_setup(R, cells, 77, dtype)
    tab = gpu_table(t, dtype, dev)
    lg, Ml, _ = R64.forward(p, conf, hp, feats_of(t), False)
    for env in ({}, {"MFAS_EVAL_NO_B3": "1"}):
        pop = make_pop(hp, conf, dev, 3, env=env)
        pop.set_state_dict(0, p)
        R64.assert_close64(pop.forward(0, tab).cpu().numpy(), lg, Ml, TAU_ONE_LAYER, f"one-layer R{R} {dtype} {env}",
                           record=f"forward_one_layer/{dtype}")
        pop.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_train_schedules_dev_stats_vs_ref64(dev, name):
    """Each train schedule (lean chain, general chain at 1 / 2 / 4 m-blocks, the same-group launch, chain_split), asserted with
    pop.schedule(): one epoch with a dev table, every candidate's dev statistics against ref64 on its parameters after the call."""
    R, C, B, env, cc, K, check = SCHEDULES[name]
    hp = O.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, s_sizes=W_A["s"], v_sizes=W_A["v"], epochs=1)
    confs = [np.array(c) for c in ([[3, 3, 0], [1, 2, 1]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1], [1, 1, 0]])[:K]]
    from mfas_amd import Population
    from tests.helpers import engine_hyper
    os.environ.update(env)
    try:
        pop = Population(engine_hyper(hp), confs, dev, drop_seeds=list(range(5, 5 + K)), chunk_cols=cc)
    finally:
        for k in env:
            os.environ.pop(k, None)
    sched = pop.schedule()
    assert check(sched), (name, sched)
    for k, c in enumerate(confs):
        pop.set_state_dict(k, O.init_params(c, hp, 40 + k, perturb_bn=True))
    case = (name, R, C, B, W_A, None, True, 0.5, "")
    ntr = 5 * B + 3
    ttr, tdv = case_table(case, hp, ntr, 61, "bfloat16"), case_table(case, hp, N_EVAL, 62, "bfloat16")
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / B, -(-ntr // B))
    stats, status = pop.train(gpu_table(ttr, "bfloat16", dev), gpu_table(tdv, "bfloat16", dev), 1, etas)
    assert not status.any(), (name, status)
    for k, c in enumerate(confs):
        check_dev(stats[k:k + 1], state_np(pop, k), c, hp, tdv, f"{name} cand {k}")
    pop.close()


@pytest.mark.gpu
def test_width0_tap_slot(dev):
    """A width-0 tap is an unused slot: a configuration that selects it is refused at create; one that does not trains and
    evaluates with the empty tap present in the table (no pointer is needed for it)."""
    hp = O.Hyper(R=16, C=17, B=16, bn=True, drpt=0.5, s_sizes=W_B["s"], v_sizes=W_B["v"], epochs=1)
    with pytest.raises(RuntimeError, match="unused tap slot"):
        make_pop(hp, np.array([[3, 0, 0]]), dev, 1)
    case = ("w0", 16, 17, 16, W_B, [[2, 1, 0]], True, 0.5, "")
    conf, p0 = case_params(case, hp, 5)
    t = case_table(case, hp, N_EVAL, 5, "float32")
    assert t["s3"].shape == (N_EVAL, 0)
    tab = gpu_table(t, "float32", dev)
    pop = make_pop(hp, conf, dev, 5)
    pop.set_state_dict(0, p0)
    lg, Ml, _ = R64.forward(p0, conf, hp, feats_of(t), False)
    R64.assert_close64(pop.forward(0, tab).cpu().numpy(), lg, Ml, TAU_LOGITS, "width-0 slot forward")
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N_EVAL / 16, 6)
    stats, status = pop.train(tab, tab, 1, etas)
    assert not status.any()
    check_dev(stats, state_np(pop), conf, hp, t, "width-0 slot train")
    pop.close()
