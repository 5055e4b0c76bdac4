"""The kernels against the float64 reference on degenerate and extreme input VALUES (tests/input_edges.py), where every other
ref64 file varies the shapes and draws the values from one distribution.

Each entry of input_cases.INPUT_CASES (base case, transform, table dtype) runs the four blocks of
test_gpu_ref64.py::test_entry_points_vs_ref64 on the transformed inputs — the eval forward over the ragged row ranges in every
dev-pass build, forward_train + running statistics, backward of arbitrary dlogits, one epoch of train() with a dev table — and
steps 1, 2 and 3 of train() as test_gpu_train_ref64.py checks them.  Same rule, same taus: |got - ref64| <= tau 2^-24 M
elementwise (logits 6, gradients 20, running statistics 4; steps: m 20, v 1, w 20, runstat 4, loss 1).  On top of that:

* status is 0 and every reported loss finite: these inputs are finite in the reference's float32 formula;
* 'onelabel': a count equals ref64's lo whenever lo == hi;
* 'dup' / 'dead' / 'deadrelu' with BatchNorm: a named column has batch variance 0 in ref64's own forward (so the case cannot
  silently stop being degenerate; 'deadrelu': a column of the FIRST cell, a ReLU, exactly 0 on every row); its running variance moves
  by exactly the momentum step towards 0, which the elementwise check holds;
* 'bigmean' and the wide 'dup' (input_cases.FLAGGED) are judged with ref64's batch_sum_term — the rounding of the two batch sums
  themselves added to M_mu and M_var (tests/ref64.py::forward) — in forward_train, backward and the train steps; every other entry,
  'deadrelu' included, without it.  The taus are the same;
* POP_CASES: one candidate of a population transformed ('dead', 'bighead', 'deadrelu'), on the resident schedule, on chain_split, on
  the same-group launch and on launch per phase: the neighbours bit-identical to the run where nobody is transformed, the
  transformed one held to ref64 (without the term).

tests/test_inputs_cpu.py holds the float32 oracle under a quarter of each tau on exactly these inputs.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_inputs_ref64.py -m gpu -x -q -s

Observed on the MI355X (54 tests, 8 s; the run prints the table with -s): worst ratio per quantity and transform, the engine's
figure / the float32 oracle's on the same inputs on the CPU (tests/test_inputs_cpu.py).  No kernel had to change.

  transform   forward      fwd_train    backward     run_stats    train m      train v      train w      runstat      loss
  (tau)       6            6            20           4            20           1            20           4            1
  scaled      0.27 / 0.14  0.07 / 0.18  2.85 / 3.66  0.31 / 0.54  0.81 / 0.81  0.18 / 0.18  4.15 / 4.04  0.80 / 0.80  0.001 / 0.001
  tiny        0.81 / 0.81  0.77 / 0.77  3.38 / 3.15  0.79 / 0.79  0.94 / 0.98  0.17 / 0.17  4.23 / 4.23  0.79 / 0.79  0.017 / 0.010
  sparse      0.23 / 0.08  0.16 / 0.16  2.57 / 2.57  0.83 / 0.83  0.89 / 0.89  0.18 / 0.18  3.70 / 4.08  0.78 / 0.78  0.016 / 0.008
  offset      0.20 / 0.08  0.05 / 0.10  2.04 / 2.04  0.74 / 0.74  0.87 / 0.87  0.17 / 0.16  3.48 / 3.56  0.77 / 0.77  0.002 / 0.001
  dup         0.14 / 0.05  0.07 / 0.15  2.30 / 2.30  0.80 / 0.80  0.92 / 0.92  0.18 / 0.18  3.75 / 4.16  0.83 / 0.82  0.004 / 0.002
  onelabel    0.19 / 0.19  0.07 / 0.12  2.91 / 2.91  0.81 / 0.81  0.71 / 0.71  0.17 / 0.17  3.83 / 3.83  0.88 / 0.82  0.004 / 0.003
  dead        0.53 / 0.51  0.59 / 0.74  3.02 / 3.02  0.77 / 0.77  0.79 / 0.79  0.18 / 0.17  3.49 / 3.66  0.81 / 0.81  0.010 / 0.004
  bighead     0.24 / 0.17  0.09 / 0.14  2.49 / 3.46  0.80 / 0.80  0.86 / 0.86  0.18 / 0.18  3.96 / 4.13  0.76 / 0.76  0.002 / 0.002
  mlrows      0.31 / 0.17  0.27 / 0.32  2.05 / 2.50  0.60 / 0.60  0.92 / 0.92  0.18 / 0.18  4.12 / 4.12  0.79 / 0.79  0.006 / 0.002
  deadrelu    0.11 / 0.05  0.000/ 0.000 2.20 / 2.20  0.80 / 0.80  0.85 / 0.87  0.17 / 0.17  3.42 / 3.92  0.83 / 0.82  <0.001/ <0.001
  bigmean *   0.63 / 0.58  0.004/ 0.008 1.45 / 1.45  0.81 / 0.81  0.73 / 0.73  0.17 / 0.17  3.92 / 3.65  0.82 / 0.82  <0.001/ <0.001
  (* with batch_sum_term.  The two rows are the four narrow entries each; the wide w65 entries, engine (candidate 0's single passes,
   all three candidates' steps) / oracle (all three candidates):
   w65 deadrelu   0.02 / 0.05  0.000/ 0.009 0.57 / 1.58  0.78 / 0.78  0.77 / 0.77  0.15 / 0.16  3.17 / 3.41  0.82 / 0.80  <0.001/ <0.001
   w65 bigmean *  0.02 / 0.62  0.000/ 0.023 0.57 / 1.58  0.78 / 0.78  0.51 / 0.51  0.16 / 0.16  2.70 / 2.85  0.81 / 0.78  <0.001/ <0.001
   w65 dup *      0.04 / 0.11  0.001/ 0.111 0.57 / 1.58  0.74 / 0.74  0.78 / 0.79  0.16 / 0.17  3.04 / 2.90  0.82 / 0.80  <0.001/ <0.001)
  (the wide case, w256 'bighead', is inside the 'bighead' row of the oracle's column; the engine's own: forward 0.03, fwd_train
   0.02, backward 1.65, m 0.82, v 0.17, w 3.85, loss 0.002; it has no BatchNorm)
  one transformed candidate (dead / bighead / deadrelu): m 0.0001 / 0.73 / 0.83, v 0.00004 / 0.17 / 0.17, w 0.98 / 3.20 / 3.20,
  runstat 0.82 / 0.76 / 0.79, loss < 0.001
  dev_loss_sum of the one-epoch calls: 0.013 (CE), 0.003 (multi-label) of its bound.
The eval forward's engine figure covers every MFAS_EVAL_NO_* build and row range, the oracle's one pass over the 83 rows.
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import input_edges as IE
from tests import ref64 as R64
from tests import gpu_support as G
from tests import train_gpu as GT
from tests import wide_gpu as GW
from tests import input_cases as TI
from tests.gpu_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = np.float32


def zero_variance_column(how, conf, hp, cache):
    """(cell, column) that `how` leaves without batch variance, asserted on ref64's own forward."""
    if how == "dup":
        cell, col = 0, 0
    elif how == "deadrelu":     # the FIRST cell, a ReLU: exactly 0 on every row
        assert int(conf[0][2]) == 0, conf
        cell, col = 0, int(IE.dead_columns(conf, hp, 0)[0])
        assert cache["cells"][0]["var"][col] == 0.0 and not cache["cells"][0]["a"][:, col].any()
    else:
        cell = next(i for i in range(len(conf)) if int(conf[i][2]) in (0, 1))
        col = int(IE.dead_columns(conf, hp, cell)[0])
    c = cache["cells"][cell]
    assert c["var"][col] <= 1e-24 * max(1.0, c["mu"][col] ** 2), (how, cell, col, c["var"][col])
    return cell, col


def check_zero_variance(how, conf, hp, p0, cache, state, tag):
    cell, col = zero_variance_column(how, conf, hp, cache)
    key = f"fusion_layers.{cell}.2.running_var"
    want = (1.0 - hp.bn_momentum) * float(p0[key][col])
    assert abs(float(state[key][col]) - want) <= 4 * R64.U * abs(float(p0[key][col])), (tag, key, col, state[key][col], want)


def check_losses(stats, status, tag):
    assert not np.asarray(status).any(), (tag, status)
    for name in stats.dtype.names:
        if "loss" in name:
            assert np.isfinite(stats[name]).all(), (tag, name, stats[name])


def check_onelabel_counts(pop, hp, conf, p0, t, tab, tag):
    """Every label is C - 1: where ref64 leaves no row ambiguous the count is exactly its lo."""
    got, corr = pop.forward(0, tab, count=True)
    f = G.feats_of(t)
    lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
    _, _, lo, hi = R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, labels=t["label"], vlogit=f.get("vlogit"), slogit=f.get("slogit"))
    assert (t["label"] == hp.C - 1).all()
    if lo == hi:
        assert corr == lo, (tag, corr, lo)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [j for j, e in enumerate(TI.INPUT_CASES) if not TI.is_wide(e[0])],
                         ids=[n for n, e in zip(TI.INPUT_IDS, TI.INPUT_CASES) if not TI.is_wide(e[0])])
def test_input_values_vs_ref64(dev, i):
    torch = G._torch()
    cid, how, dtype = TI.INPUT_CASES[i]
    case = TI.base_case(cid)
    edit = TI.make_edit(how)
    flag = TI.entry_flag(i)         # ref64's batch-sum term, for the entries that declare it
    hp = G.case_hyper(case)
    seed = TI.entry_seed(i)
    conf, p00 = G.case_params(case, hp, seed)
    p0, t = edit(conf, hp, p00, G.case_table(case, hp, G.N_EVAL, seed, dtype), dtype)
    tab = G.gpu_table(t, dtype, dev)
    tag = f"{TI.INPUT_IDS[i]} R{hp.R} C{hp.C} B{hp.B}"
    pop = G.make_pop(hp, conf, dev, seed)
    try:
        pop.set_state_dict(0, p0)
        # 1. eval forward: every row range, every dev-pass build
        for env in G.eval_envs(hp):
            ep = pop if not env else G.make_pop(hp, conf, dev, seed, env=env)
            try:
                if env:
                    ep.set_state_dict(0, p0)
                G.check_eval_forward(ep, hp, conf, p0, t, tab, tag, how, env)
            finally:
                if env:
                    ep.close()
        if how == "onelabel":
            check_onelabel_counts(pop, hp, conf, p0, t, tab, tag)
        # 2. forward_train + running statistics, backward
        pop.set_state_dict(0, p0)
        got_state = None
        if hp.bn and how in ("dup", "dead", "deadrelu"):
            pop.forward_train(0, tab, 0, hp.B, step=3)
            got_state = G.state_np(pop)
            pop.set_state_dict(0, p0)
        cache = G.check_train_passes(pop, dev, hp, conf, p0, t, tab, seed, tag, how, batch_sum_term=flag)
        if got_state is not None:
            check_zero_variance(how, conf, hp, p0, cache, got_state, tag)
        # 3. one epoch of train() with a dev table
        pop.set_state_dict(0, p0)
        ntr = G.dev_epoch_rows(hp.B)
        _, ttr = edit(conf, hp, p00, G.case_table(case, hp, ntr, seed + 1, dtype), dtype)
        etas = O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, -(-ntr // hp.B))
        stats, status = pop.train(G.gpu_table(ttr, dtype, dev), tab, 1, etas)
        check_losses(stats, status, tag)
        G.check_dev(stats, G.state_np(pop), conf, hp, t, f"{tag} train E=1")
        if how == "onelabel":
            P = G.state_np(pop)
            lg, Ml, _ = R64.forward(P, conf, hp, G.feats_of(t), False)
            f = G.feats_of(t)
            _, _, lo, hi = R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, labels=t["label"], vlogit=f.get("vlogit"), slogit=f.get("slogit"))
            if lo == hi:
                assert int(stats["dev_corrects"].ravel()[0]) == lo, (tag, stats["dev_corrects"], lo)
        # 4. steps 1, 2, 3 of train(): a full batch, the ragged one, the next epoch's first
        N = GT.train_rows(hp.B)
        _, ts = edit(conf, hp, p00, G.case_table(case, hp, N, seed, dtype), dtype)
        order = GT.make_order(N, seed)
        etas = GT.step_etas(N, hp.B)
        S, ST = GT.engine_states(pop, G.gpu_table(ts, dtype, dev), [p0], etas, torch.from_numpy(order).to(dev))
    finally:
        pop.close()
    for j in ST:
        for name in ST[j].dtype.names:
            if "loss" in name:
                assert np.isfinite(ST[j][name]).all(), (tag, j, name)
    GT.check_candidate(S, ST, 0, conf, hp, p0, ts, order, seed, etas, tag, how, batch_sum_term=flag)
    if how == "onelabel" and hp.loss_mode == 0:
        for j in (1, 2, 3):
            batch, ep = GT.batch_of(ts, order, hp.B, j)
            exp = R64.train_step64(S[j - 1][0], conf, hp, batch, seed, j - 1, etas[j - 1], j, G.TAU_LOGITS, GT.TAU_V)
            lo, hi = exp["count"]
            if lo == hi:
                assert int(ST[j][0]["train_corrects"][ep] - ST[j - 1][0]["train_corrects"][ep]) == lo, (tag, j, lo)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [j for j, e in enumerate(TI.INPUT_CASES) if TI.is_wide(e[0])],
                         ids=[n for n, e in zip(TI.INPUT_IDS, TI.INPUT_CASES) if TI.is_wide(e[0])])
def test_wide_input_values_vs_ref64(dev, i):
    """A wide-path case (K = 3 candidates, all transformed): candidate 0's eval forward, forward_train and backward, one epoch with
    the dev table for all, then steps 1..3 of all through test_gpu_wide_ref64.run_train_steps."""
    cid, how, dtype = TI.INPUT_CASES[i]
    case = TI.base_case(cid, dtype)
    edit = TI.make_edit(how)
    flag = TI.entry_flag(i)
    hp, ehp, seed, confs, p0s, seeds, pop = GW.setup(case, dev)
    tag = f"{TI.INPUT_IDS[i]} R{hp.R} C{hp.C} B{hp.B}"
    bc = GW.base_case(case)
    try:
        assert pop.schedule()["wide"] == 1
        p0e, t = GW.edit_inputs(edit, hp, confs, p0s, G.case_table(bc, hp, G.N_EVAL, seed, dtype), dtype)
        tab = G.gpu_table(t, dtype, dev)
        for k in range(GW.K):
            pop.set_state_dict(k, p0e[k])
        G.check_eval_forward(pop, hp, confs[0], p0e[0], t, tab, tag, f"wide_{how}")
        got_state = None
        if hp.bn and how in ("dup", "deadrelu"):
            pop.forward_train(0, tab, 0, hp.B, step=3)
            got_state = G.state_np(pop, 0)
            pop.set_state_dict(0, p0e[0])
        cache = G.check_train_passes(pop, dev, hp, confs[0], p0e[0], t, tab, seed, tag, f"wide_{how}", drop_seed=seeds[0],
                                     batch_sum_term=flag)
        if got_state is not None:
            check_zero_variance(how, confs[0], hp, p0e[0], cache, got_state, tag)
        for k in range(GW.K):
            pop.set_state_dict(k, p0e[k])
        ntr = GT.train_rows(hp.B)
        _, ttr = GW.edit_inputs(edit, hp, confs, p0s, G.case_table(bc, hp, ntr, seed + 1, dtype), dtype)
        stats, status = pop.train(G.gpu_table(ttr, dtype, dev), tab, 1, O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, 2))
        check_losses(stats, status, tag)
        for k in range(GW.K):
            G.check_dev(stats[k:k + 1], G.state_np(pop, k), confs[k], hp, t, f"{tag} cand {k} train E=1")
    finally:
        pop.close()
    GW.run_train_steps(dev, case, "shared", 1, (1, 2, 3), rec=f"wide_{how}", edit=edit, batch_sum_term=flag)


# ------------------------------------------------------------------------------------------------ one transformed candidate among normal ones
def run_population(dev, name, how, k_edit):
    """TRAIN_SCHEDULES[name] with candidate k_edit's parameters transformed (how None: nobody's): states and statistics of the
    0..3-step calls, and the inputs."""
    torch = G._torch()
    inp = GT.schedule_inputs(name, "shared")
    if how is not None:
        inp["p0s"][k_edit] = IE.edge_params(inp["p0s"][k_edit], inp["hp"], inp["confs"][k_edit], how)
    pop = GT.schedule_pop(name, inp, dev)          # (asserts the schedule with pop.schedule())
    try:
        S, ST = GT.engine_states(pop, G.gpu_table(inp["t"], inp["dtype"], dev), inp["p0s"], inp["etas"], torch.from_numpy(inp["order"]).to(dev))
    finally:
        pop.close()
    return inp, S, ST


@pytest.mark.gpu
@pytest.mark.parametrize("name,how,k_edit", TI.POP_CASES, ids=[f"{n}-{h}" for n, h, _ in TI.POP_CASES])
def test_one_transformed_candidate_among_normal_ones(dev, name, how, k_edit):
    """The isolation property of the status tests without a NaN: the neighbours of a candidate with dead units or a big head are
    bit-identical (parameters, moments, running statistics, statistics, at every step count) to the run where all are normal; the
    transformed candidate is held to ref64 step by step and is not flagged (engine_states asserts status 0)."""
    _, S0, ST0 = run_population(dev, name, None, k_edit)
    inp, S1, ST1 = run_population(dev, name, how, k_edit)
    K = len(inp["confs"])
    assert K >= 3
    for j in S0:
        for k in range(K):
            if k == k_edit:
                continue
            assert ST0[j][k].tobytes() == ST1[j][k].tobytes(), (name, how, j, k, "statistics")
            for pl in ("w", "m", "v"):
                for key, a in S0[j][k][pl].items():
                    assert a.tobytes() == S1[j][k][pl][key].tobytes(), (name, how, j, k, pl, key)
        assert np.isfinite(ST1[j]["train_loss_sum"]).all(), (name, how, j)
    assert any(S0[3][k_edit]["w"][key].tobytes() != S1[3][k_edit]["w"][key].tobytes() for key in S0[3][k_edit]["w"])
    GT.check_candidate(S1, ST1, k_edit, inp["confs"][k_edit], inp["hp"], inp["p0s"][k_edit], inp["t"], inp["order"], inp["seeds"][k_edit],
                       inp["etas"], f"{name} {how} cand {k_edit}", f"pop_{how}")
