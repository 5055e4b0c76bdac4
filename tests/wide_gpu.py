"""Device plumbing of the wide ref64 tests: population setup and the stepped train runs.  Re-exports tests/wide_cases.py."""
from tests.wide_cases import *  # noqa: F401,F403  (one alias serves a consumer for the cases and the plumbing)
from tests import gpu_support as G
from tests import train_gpu as GT


def setup(case, dev, order_mode="shared"):
    from mfas_amd import Population
    hp, ehp, seed, confs, p0s, seeds = case_inputs(case, order_mode)
    pop = Population(ehp, confs, dev, drop_seeds=seeds)
    if hp.loss_mode == 1:
        pop.set_pos_weight(G.pos_weight(hp))
    return hp, ehp, seed, confs, p0s, seeds, pop


def run_train_steps(dev, case, order_mode, full, steps, rec=None, edit=None, batch_sum_term=False):
    """train(max_steps = j) of the case's K = 3 candidates, `steps` against ref64 (test_gpu_train_ref64's check) under the case's taus.
    edit: the inputs changed before the engine and ref64 see them (tests/test_gpu_inputs_ref64.py); batch_sum_term: ref64's."""
    torch = G._torch()
    cid, dtype = case[0], case[9]
    hp, ehp, seed, confs, p0s, seeds, pop = setup(case, dev, order_mode)
    try:
        assert pop.schedule()["wide"] == 1
        N, t, order, etas = train_inputs(case, hp, ehp, seed, full)
        p0s, t = edit_inputs(edit, hp, confs, p0s, t, dtype)
        S, ST = GT.engine_states(pop, G.gpu_table(t, dtype, dev), p0s, etas, torch.from_numpy(order).to(dev), steps)
    finally:
        pop.close()
    from unittest import mock
    with mock.patch.dict(GT.TAUS, case_taus(cid)[1]):      # (test_gpu_train_ref64's check reads its module's taus)
        for k in range(K):
            GT.check_candidate(S, ST, k, confs[k], hp, p0s[k], t, order[k] if ehp.order_per_candidate else order, seeds[k], etas,
                               f"{cid} {order_mode} cand {k}", rec or f"wide/{dtype}", steps, batch_sum_term=batch_sum_term)
