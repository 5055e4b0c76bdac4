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
from tests import test_gpu_ref64 as G
from tests import test_gpu_train_ref64 as GT
from tests.test_gpu_ref64 import W_A, W_B, W_C, dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = np.float32

# (id, R, C, B, widths, cells of candidate 0, bn, drpt, extra, table dtype)
WIDE_CASES = [
    ("w65", 65, 17, 64, W_A, [[0, 3, 0], [2, 1, 1]], True, 0.5, "", "float32"),
    ("w80", 80, 60, 33, W_B, [[1, 2, 0], [0, 1, 2]], False, 0.5, "lm1", "bfloat16"),
    # (R = 128 at B = 64 was accepted — eight row blocks need no k-split slabs; R = 177 is the smallest width from there on whose
    #  OUT unit, 64 * (3 * 192 + 36) * 4 = 156,672 B, no longer fits: the refused neighbour of the headline width)
    ("w177", 177, 60, 64, W_C, [[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 0, 0]], True, 0.5, "multitask", "float16"),
    ("w256", 256, 60, 64, W_A, [[3, 0, 0], [1, 3, 2]], False, 0.5, "alphas,sig1", "float32"),
    ("w512a", 512, 2, 20, W_B, [[2, 0, 0]], True, 0.0, "", "bfloat16"),
    ("w512b", 512, 128, 64, W_C, [[1, 2, 0], [3, 1, 1]], True, 0.5, "", "float16"),
    ("wc", 33, 256, 64, W_A, [[2, 3, 0], [0, 1, 1]], False, 0.5, "lm1", "float32"),
    ("wb65", 16, 60, 65, W_B, [[0, 1, 0], [1, 3, 1], [2, 2, 2]], True, 0.5, "", "bfloat16"),
    ("wb100", 17, 65, 100, W_C, [[3, 2, 1], [0, 0, 0]], True, 0.9, "", "float16"),
    ("wb128", 129, 64, 128, W_A, [[1, 1, 0]], True, 0.5, "multitask", "bfloat16"),
]
WIDE_IDS = [c[0] for c in WIDE_CASES]
PER_CANDIDATE = ("w177", "wb100")        # the cases that also run with per-candidate sample orders
# candidates 1 and 2: other cell counts (tap slots 0..2 only: every width set has them)
POOL = {1: [[0, 1, 2]], 2: [[2, 1, 1], [1, 2, 0]], 3: [[1, 0, 0], [2, 2, 1], [0, 1, 0]], 4: [[0, 0, 1], [1, 1, 0], [2, 2, 2], [0, 2, 0]]}
K = 3
SEED0 = 5000
# Per-case taus where the float32 oracle itself exceeds a quarter of the project's tau on the case's shape
# (tests/test_wide_cpu.py::test_wide_float32_oracle_calibration_margin): four times the oracle's measured maximum, rounded up.
# {case: {quantity: (tau, measured)}}; quantities: forward / forward_train / backward / running_stats, train steps m / v / w / runstat / loss
CASE_TAUS = {
    "w512a": {"train_runstat": (6, 1.313)},
    "wb128": {"running_stats": (5, 1.239), "train_runstat": (5, 1.005)},
}


def case_taus(cid):
    """(taus of the single passes, taus of the train steps) for a case."""
    single = {"forward": G.TAU_LOGITS, "forward_train": G.TAU_LOGITS, "backward": G.TAU_GRAD, "running_stats": G.TAU_RUNSTAT}
    train = dict(GT.TAUS)
    for q, (tau, _) in CASE_TAUS.get(cid, {}).items():
        if q.startswith("train_"):
            train[q[len("train_"):]] = float(tau)
        else:
            single[q] = float(tau)
    return single, train


def base_case(case, cells=None):
    """The 9-tuple test_gpu_ref64's helpers take."""
    return case[:5] + (case[5] if cells is None else cells,) + case[6:9]


def case_confs(case):
    others = [n for n in (1, 2, 3, 4) if n != len(case[5])][:K - 1]
    return [case[5]] + [POOL[n] for n in others]


def ceil16(x):
    return -(-x // 16) * 16


def pick_chunk(cols_p, target):
    return max([c for c in range(16, min(cols_p, target) + 1, 16) if cols_p % c == 0] or [16])


def legacy_refusal(case, confs):
    """Why mfas_population_create refused this geometry before the wide path: 'B>64', 'C_padded' or 'lds' (the LDS need of the
    step, the streaming sweep units and the general chain, over 150 KiB), else None.  A restatement of the validator's two rules and
    of plan_layout's lds_step for the launch-per-phase schedule with the general chain (none of the cases has a lean chain)."""
    _, R, C, B, w, _, bn, drpt, extra, _ = case
    Rp, Cp = ceil16(R), ceil16(C)
    MB = -(-B // 16)
    MB = 4 if MB == 3 else MB
    Bp, nrb = 16 * MB, Rp // 16
    if B > 64:
        return "B>64"
    if Cp > 8 * min(16, 512 // Bp):
        return "C_padded"
    assert not (nrb == 1 and Cp <= 64 and MB <= 2), "lean chain: not restated here"
    cols = [(ceil16(w["s"][c[0]]), ceil16(w["v"][c[1]])) for conf in confs for c in conf]
    tot_cols = sum(a + b for a, b in cols)
    lds_max = 64
    while Bp * (8 * lds_max + 20) * 4 <= 72 * 1024 and lds_max < 1024:
        lds_max *= 2
    target = 64
    while target * nrb < 64 * 16 and target < lds_max:
        target *= 2
    while target > 64 and tot_cols / target < 320.0:
        target //= 2
    if nrb >= 8:
        target = min(target, 64 if len(confs) >= 28 else 256)
    ls = 0
    for a, b in cols:                                   # feature units (k-split reduction slabs below eight row blocks)
        for cp in (a, b):
            cc = pick_chunk(cp, target)
            ls = max(ls, Bp * (cc + 16) + Bp * (cc + 4) + Bp * (Rp + 16) + (8 * nrb * MB * 256 if nrb < 8 else 0))
    if any(len(conf) > 1 for conf in confs):            # OUT units: the whole Rp x Rp block
        ls = max(ls, Bp * (Rp + 16) + Bp * (Rp + 4) + Bp * (Rp + 16))
    ls = max(ls, Bp * (Rp + 16) + Bp * (Rp + 4) + Bp * (Cp + 16))     # HEAD
    ls *= 4
    base = (2 * Bp * (Rp + 4) + Bp * (Cp + 4) + 4 * Rp + 3 * Bp + 16) * 4
    yf = (2 if "alphas" in extra else 1) * 4 * nrb * MB * 256 * 4
    lds_step = max(ls, base + (yf if base + yf <= max(ls, 64 * 1024) else 0))
    return "lds" if lds_step > 150 * 1024 else None


def test_cases_were_refused_before():
    """Every case meets one of the three old refusal rules, and each rule is met by some case."""
    why = {c[0]: legacy_refusal(c, case_confs(c)) for c in WIDE_CASES}
    assert all(why.values()), why
    assert set(why.values()) == {"B>64", "C_padded", "lds"}, why
    assert why["wc"] == why["w512b"] == "C_padded" and all(why[c] == "lds" for c in ("w65", "w80", "w177", "w256", "w512a")), why


def case_inputs(case, order_mode="shared"):
    """What a wide case trains, as numpy (no device): hyper-parameters, the K candidates with their initial parameters and seeds."""
    from tests.helpers import engine_hyper
    hp = G.case_hyper(base_case(case))
    seed = SEED0 + WIDE_IDS.index(case[0])
    confs, p0s = [], []
    for k, cells in enumerate(case_confs(case)):
        conf, p0 = G.case_params(base_case(case, cells), hp, seed + 10 * k)
        confs.append(conf)
        p0s.append(p0)
    ehp = engine_hyper(hp)
    ehp.order_per_candidate = order_mode == "per_candidate"
    seeds = [seed + 3 * k for k in range(K)]
    return hp, ehp, seed, confs, p0s, seeds


def train_inputs(case, hp, ehp, seed, full=1):
    """The train table of `full` full batches and a ragged one, the sample order and the learning rates of a wide case."""
    N = GT.train_rows(hp.B, full)
    assert 2 <= N - full * hp.B <= hp.B - 1
    t = G.case_table(base_case(case), hp, N, seed, case[9])
    return N, t, GT.make_order(N, seed, K if ehp.order_per_candidate else None), GT.step_etas(N, hp.B)


def setup(case, dev, order_mode="shared"):
    from mfas_amd import Population
    hp, ehp, seed, confs, p0s, seeds = case_inputs(case, order_mode)
    pop = Population(ehp, confs, dev, drop_seeds=seeds)
    if hp.loss_mode == 1:
        pop.set_pos_weight(G.pos_weight(hp))
    return hp, ehp, seed, confs, p0s, seeds, pop


def edit_inputs(edit, hp, confs, p0s, t, dtype):
    """Every candidate's parameters and the shared table passed through edit(conf, hp, p0, t, dtype) -> (p0, t) (the table as
    candidate 0's call returns it); edit None: unchanged."""
    if edit is None:
        return p0s, t
    out = [edit(confs[k], hp, p0s[k], t, dtype) for k in range(len(confs))]
    return [p for p, _ in out], out[0][1]


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
