"""What train() reports to the search controller, against the float64 reference (tests/ref64.py): the per-epoch dev statistics
of a POPULATION call, the parameters snapshot_best leaves, and the status word.

(a) Population dev pass.  REPORT_CASES names every k_eval build the dev pass's choice can reach (builds.hip.h: eval_key, held to each
    case's build by tests/test_report_cpu.py; the argument combinations no accepted geometry reaches are not built, builds.hip.h
    says why) with K >= 9 heterogeneous candidates, so that the bf16 x 3 build's 1-D grid takes its interleaved branch (full groups of
    eight candidates) and its remainder branch.
    E = 2 as two segments; column e of segment e of every candidate through check_dev against ref64 on that candidate's own
    parameters after that epoch.  The candidates' ref64 loss intervals are pairwise disjoint (asserted), so a slot or tile mix-up
    cannot pass.  tests/test_report_cpu.py checks the same conditions with oracle-trained parameters and makes five mutations of
    the per-candidate report fail.
(b) Best epoch.  best_epoch_rule() states the rule; plane 0 after a snapshot_best schedule is bit-identical to the state the rule
    names, for a threshold below, between and above the metrics; forward, backward and one further train step on the restored
    handle against ref64 (stale transposed OUT / HEAD tiles would show there).
(c) Status.  Every site that flags a non-finite train loss, by a NaN weight (CE) and by a saturated sigmoid (multi-label loss),
    with the neighbours' results bit-identical to a clean run and a control that must not be flagged.

Observed on the MI355X (the run prints the table with -s; 32 tests, 5 s), worst ratio per quantity:

  dev_loss_sum, fraction of ref64's bound, per case     0.0013 (r512_f16) .. 0.010 (r128_f32); multi-label 0.0018 / 0.0046
  after the restore: forward (6) / backward (20)        0.38 / 1.22
  the step after the restore: m (20) / v (1) / w (20) / running statistics (4) / loss (1)
                                                        0.54 / 0.036 / 3.6 / 0.74 / 0.0016
  control's first train loss, fraction of the bound     0.005 .. 0.019 (the float32 oracle on the CPU: 0.005 .. 0.019)

No kernel had to change: every candidate's statistics land in its own slot on every build, plane 0 is the state the rule names
for all three thresholds, and all flagging sites raise status 1 for the poisoned candidate alone.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_report_ref64.py -m gpu -x -q -s
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import gpu_support as G
from tests import train_cases as GT
from tests.gpu_support import W_A, W_B, dev  # noqa: F401
from tests.report_cases import (CONTROL_BIAS, E_REPORT, E_STATUS, F32, N_DEV, POISON_BIAS, REPORT_CASES, REPORT_IDS, STATUS_LM1,
                                STATUS_SCHEDULES, best_epoch_rule, check_conditions, dev_ref, first_batch_loss32, poisoned,
                                report_inputs, status_inputs)
from tests.report_gpu import make_population, plane_bytes

pytestmark = pytest.mark.gpu


def record(key, value):
    R64.RATIOS[key] = max(R64.RATIOS.get(key, 0.0), float(value))


# ------------------------------------------------------------------------------------------------ (a) the population dev pass
@pytest.mark.gpu
@pytest.mark.parametrize("case", REPORT_CASES, ids=REPORT_IDS)
def test_population_dev_pass_vs_ref64(dev, case):
    """Two epochs as two segments: every candidate's dev statistics of epoch e against ref64 on its own parameters after epoch e,
    the other column zero, and the conditions that make a slot or tile mix-up visible.  (The build the case was written for: the
    record does not cover the dev pass, tests/test_report_cpu.py holds it without a device.)"""
    from tests.helpers import engine_hyper
    cid, R, C, B, dtype, K, extra, build = case
    inp = report_inputs(case)
    hp = inp["hp"]
    pop = make_population(engine_hyper(hp), inp["confs"], dev, inp["seeds"], pos_weight=G.pos_weight(hp) if hp.loss_mode else None)
    try:
        for k, p in enumerate(inp["p0s"]):
            pop.set_state_dict(k, p)
        ttr, tdv = G.gpu_table(inp["ttr"], dtype, dev), G.gpu_table(inp["tdv"], dtype, dev)
        seg, states = [], []
        for e in range(E_REPORT):
            stats, status = pop.train(ttr, tdv, E_REPORT, inp["etas"], first_epoch=e, last_epoch=e + 1)
            assert not status.any(), (cid, e, status)
            seg.append(stats.copy())
            states.append([G.state_np(pop, k) for k in range(K)])
    finally:
        pop.close()
    for e in range(E_REPORT):
        refs = [dev_ref(states[e][k], inp["confs"][k], hp, inp["tdv"]) for k in range(K)]
        check_conditions(refs, hp, N_DEV, f"{cid} epoch {e}")
        for k in range(K):
            other = seg[e][k][1 - e]
            assert other.tobytes() == bytes(other.nbytes), (cid, e, k, other)
            G.check_dev(seg[e][k:k + 1, e:e + 1], states[e][k], inp["confs"][k], hp, inp["tdv"], f"{cid} cand {k} epoch {e}")
            loss, lb, lo, hi = refs[k]
            record(f"report_dev_loss/{cid}", abs(float(seg[e]["dev_loss_sum"][k, e]) - loss) / lb)
            assert np.isfinite(seg[e]["train_loss_sum"][k, e]) and seg[e]["train_loss_sum"][k, e] != 0.0, (cid, e, k)


# ------------------------------------------------------------------------------------------------ (b) the best epoch
E_BEST = 3
BEST_SCHEDULES = {
    # name: (R, C, B, env, chunk_cols, K, tap_bits, check)
    "resident": (16, 60, 20, {}, 0, 6, 0, lambda s: s["persistent"] == 1 and s["lean_chain"] == 1),
    "chain_split": (128, 60, 16, {"MFAS_SAME_GROUP": "2"}, 128, 2, 0, lambda s: s["groups"] == -1 and s["chain_cus"] == 4),
}


def best_inputs(name):
    from tests.helpers import engine_hyper
    R, C, B, env, cc, K, tap_bits, check = BEST_SCHEDULES[name]
    hp = O.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, s_sizes=W_A["s"], v_sizes=W_A["v"], epochs=E_BEST)
    confs = [np.array(GT.SCHED_CONFS[k % len(GT.SCHED_CONFS)]) for k in range(K)]
    tup = (name, R, C, B, W_A, None, True, 0.5, "")
    ntr = 2 * B + 3
    return dict(hp=hp, ehp=engine_hyper(hp), confs=confs, seeds=[11 + 3 * k for k in range(K)], env=env, cc=cc, check=check,
                p0s=[O.init_params(c, hp, 140 + k, perturb_bn=True) for k, c in enumerate(confs)],
                ttr=G.case_table(tup, hp, ntr, 161, "bfloat16"), tdv=G.case_table(tup, hp, G.N_EVAL, 162, "bfloat16"),
                etas=O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / B, E_BEST * -(-ntr // B)))


def best_pop(inp, dev):
    pop = make_population(inp["ehp"], inp["confs"], dev, inp["seeds"], env=inp["env"], chunk_cols=inp["cc"])
    try:
        assert inp["check"](pop.schedule()), pop.schedule()
        for k, p in enumerate(inp["p0s"]):
            pop.set_state_dict(k, p)
    except BaseException:
        pop.close()
        raise
    return pop


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BEST_SCHEDULES))
def test_snapshot_best_leaves_the_epoch_the_rule_names(dev, name):
    torch = G._torch()
    inp = best_inputs(name)
    hp, confs, K = inp["hp"], inp["confs"], len(inp["confs"])
    ttr, tdv = G.gpu_table(inp["ttr"], "bfloat16", dev), G.gpu_table(inp["tdv"], "bfloat16", dev)
    # 1. segments without snapshot_best: plane 0 after every epoch, the initial bytes, the metrics
    pop = best_pop(inp, dev)
    try:
        kept = [[plane_bytes(pop, k) for k in range(K)]]
        metrics = np.zeros((K, E_BEST))
        for e in range(E_BEST):
            stats, status = pop.train(ttr, tdv, E_BEST, inp["etas"], first_epoch=e, last_epoch=e + 1)
            assert not status.any(), (name, e, status)
            kept.append([plane_bytes(pop, k) for k in range(K)])
            metrics[:, e] = stats["dev_corrects"][:, e].astype(np.float64) / float(G.N_EVAL)
    finally:
        pop.close()
    assert all(len({kept[e][k] for e in range(E_BEST + 1)}) == E_BEST + 1 for k in range(K)), "every epoch moves every candidate"
    tops = sorted(set(metrics.max(1).tolist()))
    assert len(tops) >= 2, (name, metrics)         # (else no threshold separates the candidates)
    thresholds = {"below": -1.0, "between": 0.5 * (tops[0] + tops[1]), "above": 2.0}
    single, train_taus = {"forward": G.TAU_LOGITS, "backward": G.TAU_GRAD}, dict(GT.TAUS)
    nb_rows = hp.B
    rng = np.random.default_rng(9)
    dl = (rng.standard_normal((nb_rows, hp.C)) / nb_rows).astype(F32)
    from mfas_amd.engine import flat_layout
    for tname, thr in thresholds.items():
        rule = [best_epoch_rule(metrics[k], thr) for k in range(K)]
        if tname == "between":
            assert any(ep < 0 for ep, _ in rule) and any(ep >= 0 for ep, _ in rule), (name, thr, metrics)
        if tname == "above":
            assert all(ep < 0 for ep, _ in rule)
        # 2. the whole schedule in one call with snapshot_best
        pop = best_pop(inp, dev)
        try:
            pop.set_best_threshold(thr)
            stats, status = pop.train(ttr, tdv, E_BEST, inp["etas"], snapshot_best=True, first_epoch=0, last_epoch=E_BEST)
            assert not status.any(), (name, tname, status)
            assert np.array_equal(stats["dev_corrects"].astype(np.float64) / float(G.N_EVAL), metrics), (name, tname)
            for k in range(K):
                ep, best = rule[k]
                got = plane_bytes(pop, k)     # 3. bit-identical to the state the rule names (a tie keeps the earlier epoch)
                match = [e - 1 for e in range(E_BEST + 1) if kept[e][k] == got]
                assert match == [ep], f"{name} {tname} cand {k}: plane 0 is the state after epoch {match} (-1: initial), the rule names {ep}; metrics {metrics[k]}, threshold {thr}"
                assert pop.get_progress(k)["best_metric"] == best, (name, tname, k, pop.get_progress(k), best)       # 4.
            # 5. forward and backward on the restored handle (nothing re-packed in between)
            for k in range(K):
                P = G.state_np(pop, k)
                lg, Ml, _ = R64.forward(P, confs[k], hp, G.feats_of(inp["tdv"]), False)
                R64.assert_close64(pop.forward(k, tdv).cpu().numpy(), lg, Ml, single["forward"], f"{name} {tname} cand {k} forward after restore",
                                   record=f"restored_forward/{name}")
                flat = pop.backward(k, ttr, torch.from_numpy(dl).to(dev), 0, nb_rows, step=2).cpu().numpy()
                _, _, cache = R64.forward(P, confs[k], hp, G.feats_of(inp["ttr"], 0, nb_rows), True, seed=inp["seeds"][k], step=2)
                Gr, MG = R64.backward(P, hp, cache, dl)
                for key, shape, off in flat_layout(confs[k], hp)[0]:
                    if key in Gr:
                        R64.assert_close64(flat[off:off + int(np.prod(shape))].reshape(shape), Gr[key], MG[key], single["backward"],
                                           f"{name} {tname} cand {k} backward after restore {key}", record=f"restored_backward/{name}")
            # 6. one further train step from what the handle holds now (backward moved the running statistics; W is the restored W)
            prev = [{"w": G.state_np(pop, k)} for k in range(K)]
            for k in range(K):
                zero = {key: np.zeros_like(v) for key, v in prev[k]["w"].items()}
                prev[k].update(m=zero, v=zero)
            st1, status = pop.train(ttr, None, 1, inp["etas"], max_steps=1)
            assert not status.any(), (name, tname, status)
            batch = {key: v[:hp.B] for key, v in inp["ttr"].items()}
            for k in range(K):
                cur = {"w": G.state_np(pop, k, 0), "m": G.state_np(pop, k, 1), "v": G.state_np(pop, k, 2)}
                exp = R64.train_step64(prev[k], confs[k], hp, batch, inp["seeds"][k], 0, inp["etas"][0], 1, G.TAU_LOGITS, GT.TAU_V, observed=cur)
                R64.check_train_step(exp, cur, st1["train_loss_sum"][k, 0], int(st1["train_corrects"][k, 0]), train_taus,
                                     f"{name} {tname} cand {k} step after restore", rec=f"restored/{name}")
        finally:
            pop.close()


STATUS_SEGMENTED = "general_mb1"


def status_run(inp, dev, how, segments=False, max_steps=-1):
    """One schedule with candidate 1 poisoned `how` (None: clean): statistics, status, planes 0..2 of every candidate."""
    hp, K = inp["hp"], len(inp["confs"])
    pop = make_population(inp["ehp"], inp["confs"], dev, inp["seeds"], env=inp["env"], chunk_cols=inp["cc"],
                          pos_weight=G.pos_weight(hp) if hp.loss_mode else None)
    try:
        assert inp["check"](pop.schedule()), pop.schedule()
        for k, p in enumerate(inp["p0s"]):
            pop.set_state_dict(k, poisoned(p, how) if k == 1 else p)
        ttr, tdv = G.gpu_table(inp["ttr"], "bfloat16", dev), G.gpu_table(inp["tdv"], "bfloat16", dev)
        if segments:
            out = [pop.train(ttr, tdv, E_STATUS, inp["etas"], first_epoch=e, last_epoch=e + 1) for e in range(E_STATUS)]
            stats, status = out[-1][0], [s.copy() for _, s in out]
        elif max_steps >= 0:
            stats, status = pop.train(ttr, None, E_STATUS, inp["etas"], max_steps=max_steps)
        else:
            stats, status = pop.train(ttr, tdv, E_STATUS, inp["etas"])       # (returns without error: a lost dependency would raise)
        planes = [[plane_bytes(pop, k, pl) for pl in range(3)] for k in range(K)]
        final = [G.state_np(pop, k) for k in range(K)]
    finally:
        pop.close()
    return stats, status, planes, final


def assert_isolated(clean, bad, K, tag):
    (cs, cst, cpl, _), (bs, bst, bpl, _) = clean, bad
    assert cst.tolist() == [0] * K, (tag, cst)
    assert bst.tolist() == [0, 1] + [0] * (K - 2), (tag, bst)
    for k in range(K):
        if k != 1:
            assert cs[k].tobytes() == bs[k].tobytes(), (tag, k, cs[k], bs[k])
            assert cpl[k] == bpl[k], (tag, k, "planes 0-2 differ from the clean run")
    assert not np.isfinite(bs["train_loss_sum"][1]).any(), (tag, bs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STATUS_SCHEDULES))
def test_nan_weight_is_flagged_and_isolated(dev, name):
    """CE: one fusion weight of candidate 1 is the canonical quiet NaN.  Status [0, 1, 0, ...], the neighbours bit-identical to the
    clean run, the poisoned candidate's train loss non-finite from epoch 0; on one schedule also as two segments (sticky status)."""
    inp = status_inputs(name, False)
    K = len(inp["confs"])
    clean, bad = status_run(inp, dev, None), status_run(inp, dev, "nan")
    assert_isolated(clean, bad, K, name)
    if name == STATUS_SEGMENTED:
        stats, statuses, planes, _ = status_run(inp, dev, "nan", segments=True)
        assert [s.tolist() for s in statuses] == [[0, 1] + [0] * (K - 2)] * E_STATUS, (name, statuses)
        assert planes == bad[2], (name, "segments differ from the one call")


@pytest.mark.gpu
@pytest.mark.parametrize("name", STATUS_LM1)
def test_saturated_sigmoid_is_flagged_and_isolated(dev, name):
    """Multi-label loss: one class of candidate 1's head bias is +40, so sigmoid rounds to 1 and -log(1 - s) is inf (or 0 * inf), as
    in the reference's WeightedCrossEntropyWithLogits.  The control's bias keeps the float32 logits below 16: no flag, and its loss
    is finite and inside ref64's bound."""
    inp = status_inputs(name, True)
    hp, K = inp["hp"], len(inp["confs"])
    loss32, _ = first_batch_loss32(inp, 1, poisoned(inp["p0s"][1], POISON_BIAS))
    assert not np.isfinite(loss32), loss32                           # the reference's formula, float32: non-finite on this batch
    ctl32, top = first_batch_loss32(inp, 1, poisoned(inp["p0s"][1], CONTROL_BIAS))
    assert np.isfinite(ctl32) and top < 16.0, (ctl32, top)
    clean, bad = status_run(inp, dev, None), status_run(inp, dev, POISON_BIAS)
    assert_isolated(clean, bad, K, name)
    # control: not flagged, every loss finite, the dev statistics of the last epoch and the first step's train loss inside ref64's bound
    cs, cst, _, final = status_run(inp, dev, CONTROL_BIAS)
    assert cst.tolist() == [0] * K, (name, cst)
    assert np.isfinite(cs["train_loss_sum"]).all() and np.isfinite(cs["dev_loss_sum"]).all(), (name, cs)
    G.check_dev(cs[1:2, E_STATUS - 1:E_STATUS], final[1], inp["confs"][1], hp, inp["tdv"], f"{name} control")
    s1, st1, _, _ = status_run(inp, dev, CONTROL_BIAS, max_steps=1)
    assert st1.tolist() == [0] * K, (name, st1)
    p1 = poisoned(inp["p0s"][1], CONTROL_BIAS)
    zero = {key: np.zeros_like(v) for key, v in p1.items()}
    exp = R64.train_step64({"w": p1, "m": zero, "v": zero}, inp["confs"][1], hp, {key: v[:hp.B] for key, v in inp["ttr"].items()},
                           inp["seeds"][1], 0, inp["etas"][0], 1, G.TAU_LOGITS, GT.TAU_V, pos_weight=G.pos_weight(hp))
    ref_loss, lb = exp["loss"]
    got = float(s1["train_loss_sum"][1, 0])
    record(f"control_train_loss/{name}", abs(got - ref_loss) / lb)
    assert abs(got - ref_loss) <= lb, f"{name} control train loss: got {got!r}, ref64 {ref_loss!r}, bound {lb:.3g}"
