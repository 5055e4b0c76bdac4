"""The wide path (wide.hip.h: k_chain_wide + k_sweep_wide) against the float64 reference, on shapes the engine refused before it
existed: batch sizes above 64, steps whose LDS need is over 150 KiB, heads with more classes than the batch-resident softmax takes.

Same rule and same taus as test_gpu_ref64.py / test_gpu_train_ref64.py: |got - ref64| <= tau * 2^-24 * M elementwise (logits 6,
gradients 20, running statistics 4; train steps: m 20, v 1, w 20, loss 1).  tests/test_wide_cpu.py holds the float32 oracle under
a quarter of each on these shapes and makes three wide-specific mutations exceed them.

WIDE_CASES is a covering design: the smallest shape at which each refusal reason and each loop edge of the two kernels appears
(16-row tiles staged two at a time, batch slices of 64 rows, row-block groups of 8, k-block groups of 8).  legacy_refusal() restates
the three rules by which mfas_population_create refused a geometry, so the file says why each case is wide.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_wide_ref64.py -m gpu -x -q -s
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import gpu_support as G
from tests import train_cases as GT
from tests.gpu_support import W_A, W_B, W_C, dev  # noqa: F401
from tests.wide_cases import K, PER_CANDIDATE, WIDE_CASES, WIDE_IDS, base_case, case_confs, case_taus, legacy_refusal
from tests.wide_gpu import run_train_steps, setup

pytestmark = pytest.mark.gpu

F32 = np.float32


def test_cases_were_refused_before():
    """Every case meets one of the three old refusal rules, and each rule is met by some case."""
    why = {c[0]: legacy_refusal(c, case_confs(c)) for c in WIDE_CASES}
    assert all(why.values()), why
    assert set(why.values()) == {"B>64", "C_padded", "lds"}, why
    assert why["wc"] == why["w512b"] == "C_padded" and all(why[c] == "lds" for c in ("w65", "w80", "w177", "w256", "w512a")), why


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_CASES, ids=WIDE_IDS)
def test_wide_entry_points_vs_ref64(dev, case):
    """forward (the dev pass) over ragged row ranges, forward_train + running statistics and backward of arbitrary dlogits for
    every candidate, then one epoch of train() with the 83-row dev table: the dev statistics on the parameters it leaves."""
    torch = G._torch()
    from mfas_amd.engine import flat_layout
    cid, dtype = case[0], case[9]
    hp, ehp, seed, confs, p0s, seeds, pop = setup(case, dev)
    taus, _ = case_taus(cid)
    try:
        sched = pop.schedule()
        assert sched["wide"] == 1 and sched["groups"] == 1 and sched["persistent"] == 0 and sched["lean_chain"] == 0, sched
        bc = base_case(case)
        t = G.case_table(bc, hp, G.N_EVAL, seed, dtype)
        tab = G.gpu_table(t, dtype, dev)
        ME = G.eval_me(hp)
        # train-mode single batches: a table with at least one full batch
        tb = t if hp.B <= G.N_EVAL else G.case_table(bc, hp, hp.B, seed + 5, dtype)
        tbab = tab if tb is t else G.gpu_table(tb, dtype, dev)
        for k in range(K):
            pop.set_state_dict(k, p0s[k])
        for k in range(K):
            conf, p0 = confs[k], p0s[k]
            tag = f"{cid} cand {k} R{hp.R} C{hp.C} B{hp.B} {dtype}"
            for row0, nrows in ((0, G.N_EVAL), (5, ME + 1), (5, 1)) if k == 0 else ((0, G.N_EVAL),):
                got, corr = pop.forward(k, tab, row0=row0, nrows=nrows, count=True)
                f = G.feats_of(t, row0, nrows)
                lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
                R64.assert_close64(got.cpu().numpy(), lg, Ml, G.TAU_LOGITS, f"{tag} forward rows {row0}+{nrows}", record=f"wide_forward/{dtype}")
                if hp.loss_mode == 0:
                    _, _, lo, hi = R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, labels=t["label"][row0:row0 + nrows],
                                                 vlogit=f.get("vlogit"), slogit=f.get("slogit"))
                    assert lo <= corr <= hi, f"{tag} forward count: {corr} not in [{lo}, {hi}]"
            step = 3
            for nb in (hp.B, hp.B - 3):       # a full batch and a ragged one
                pop.set_state_dict(k, p0)
                f = G.feats_of(tb, 0, nb)
                got = pop.forward_train(k, tbab, 0, nb, step=step).cpu().numpy()
                lg, Ml, cache = R64.forward(p0, conf, hp, f, True, seed=seeds[k], step=step)
                R64.assert_close64(got, lg, Ml, G.TAU_LOGITS, f"{tag} forward_train {nb}", record=f"wide_forward_train/{dtype}")
                if hp.bn:
                    rs, Mrs = R64.running_stats(p0, hp, cache)
                    sd = G.state_np(pop, k)
                    for key in rs:
                        R64.assert_close64(sd[key], rs[key], Mrs[key], taus["running_stats"], f"{tag} forward_train {nb} {key}",
                                           record=f"wide_running_stats/{dtype}")
                pop.set_state_dict(k, p0)
                rng = np.random.default_rng(seed + k)
                dl = (rng.standard_normal((nb, hp.C)) / nb).astype(F32)
                dl[rng.random((nb, hp.C)) < 0.1] *= F32(1e-3)
                flat = pop.backward(k, tbab, torch.from_numpy(dl).to(dev), 0, nb, step=step).cpu().numpy()
                G64, MG = R64.backward(p0, hp, cache, dl)
                layout, _ = flat_layout(conf, hp)
                for key, shape, off in layout:
                    if key in G64:
                        R64.assert_close64(flat[off:off + int(np.prod(shape))].reshape(shape), G64[key], MG[key], G.TAU_GRAD,
                                           f"{tag} backward {nb} {key}", record=f"wide_backward/{dtype}")
        for k in range(K):
            pop.set_state_dict(k, p0s[k])
        ntr = hp.B + GT.ragged_rows(hp.B)
        ttr = G.case_table(bc, hp, ntr, seed + 1, dtype)
        stats, status = pop.train(G.gpu_table(ttr, dtype, dev), tab, 1, O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, 2))
        assert not status.any(), (cid, status)
        for k in range(K):
            G.check_dev(stats[k:k + 1], G.state_np(pop, k), confs[k], hp, t, f"{cid} cand {k} train E=1")
    finally:
        pop.close()


TRAIN_PARAMS = [(c, "shared") for c in WIDE_CASES] + [(c, "per_candidate") for c in WIDE_CASES if c[0] in PER_CANDIDATE]


@pytest.mark.gpu
@pytest.mark.parametrize("case,order_mode", TRAIN_PARAMS, ids=[f"{c[0]}-{m}" for c, m in TRAIN_PARAMS])
def test_wide_train_steps_vs_ref64(dev, case, order_mode):
    """train(max_steps = 0..3) of K = 3 candidates of different depth, step by step against ref64 (test_gpu_train_ref64's check):
    N = B + ragged rows, so step 1 is a full batch through the sample order, step 2 the ragged last batch, step 3 crosses the epoch."""
    run_train_steps(dev, case, order_mode, 1, (1, 2, 3))


@pytest.mark.gpu
def test_wide_train_is_deterministic_and_restarts_adam(dev):
    """Two identical train() calls give identical bits (W / m / v, statistics, status); a further call on the same handle starts
    from zeroed moments; a last batch of one row with BatchNorm is refused."""
    torch = G._torch()
    case = WIDE_CASES[WIDE_IDS.index("wb100")]
    dtype = case[9]
    hp, ehp, seed, confs, p0s, seeds, pop = setup(case, dev)
    try:
        N = hp.B + GT.ragged_rows(hp.B)
        t = G.case_table(base_case(case), hp, N, seed, dtype)
        tdv = G.case_table(base_case(case), hp, G.N_EVAL, seed + 2, dtype)
        tab, dtab = G.gpu_table(t, dtype, dev), G.gpu_table(tdv, dtype, dev)
        order = torch.from_numpy(GT.make_order(N, seed)).to(dev)
        etas = GT.step_etas(N, hp.B)
        runs = []
        for _ in range(2):
            for k in range(K):
                pop.set_state_dict(k, p0s[k])
            stats, status = pop.train(tab, dtab, GT.EPOCHS, etas, order=order)
            runs.append((stats.copy(), status.copy(), [[G.state_np(pop, k, pl) for pl in range(3)] for k in range(K)]))
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and np.array_equal(runs[0][1], runs[1][1])
        for k in range(K):
            for pl in range(3):
                for key, a in runs[0][2][k][pl].items():
                    assert a.tobytes() == runs[1][2][k][pl][key].tobytes(), (k, pl, key)
            assert any(v.any() for v in runs[0][2][k][1].values())          # the moments are live after a call
        stats, status = pop.train(tab, None, GT.EPOCHS, etas, order=order, max_steps=0)
        for k in range(K):
            for pl in (1, 2):
                assert all(not v.any() for key, v in G.state_np(pop, k, pl).items() if key in O.trainable_keys(confs[k], hp)), (k, pl)
        t1 = G.case_table(base_case(case), hp, hp.B + 1, seed, dtype)
        with pytest.raises(RuntimeError, match="size 1"):
            pop.train(G.gpu_table(t1, dtype, dev), None, 1, O.eta_sequence(1e-3, 1e-6, 1, 2, (hp.B + 1) / hp.B, 2), max_steps=2)
    finally:
        pop.close()
