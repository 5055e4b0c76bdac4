"""Device plumbing of the train ref64 tests: the engine's states, the scheduled populations and the per-candidate check.  Re-exports
tests/train_cases.py."""
import os

import numpy as np

from tests.train_cases import *  # noqa: F401,F403  (one alias serves a consumer for the cases and the plumbing)
from oracle import np_oracle as O
from tests import gpu_support as G
from tests import ref64 as R64
from tests.gpu_support import gpu_table, pos_weight, state_np


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
