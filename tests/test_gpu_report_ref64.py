"""What train() reports to the search controller, against the float64 reference (tests/ref64.py): the per-epoch dev statistics
of a POPULATION call, the parameters snapshot_best leaves, and the status word.

(a) Population dev pass.  REPORT_CASES names every k_eval build the dev pass's choice can reach (builds.hip.h: eval_key, held to each
    case's build by tests/test_report_cpu.py; the builds no accepted geometry reaches are listed in UNREACHABLE_BUILDS with the
    reason) with K >= 9 heterogeneous candidates, so that the bf16 x 3 build's 1-D grid takes its interleaved branch (full groups of
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
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import test_gpu_ref64 as G
from tests import test_gpu_train_ref64 as GT
from tests.test_gpu_ref64 import W_A, W_B, dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = np.float32
N_DEV = 147          # three 64-row tiles, the last ragged (19 rows); five 32-row tiles; ten 16-row tiles
E_REPORT = 2
MAX_AMBIGUOUS = 3    # rows of N_DEV whose decision ref64 leaves open, per candidate and epoch
MAX_UNBOUNDED_CELLS = 2      # (one above R = 256)
# Every draw (configurations, initial parameters, tables) of case i comes from the seed 7000 + 100 i + shift.  The shift is the first
# of 0, 1, 2, ... for which the REFERENCE ALONE (float32-oracle-trained parameters, ref64 intervals) meets check_conditions with
# margin 2 and one open row to spare (tests/test_report_cpu.py::test_report_cases_calibration_and_conditions); no engine result
# entered the choice.
SEED_SHIFT = {"b3_k11": 1, "b3_k16_mt": 2, "b3_me32_k9": 1, "b3_lm1_k9": 6, "r16_bf16": 1, "r512_f16": 13}

# (id, R, C, B, table dtype, K, extra, build = (MBE, NRBW, split, 16-bit rows, B3))
REPORT_CASES = [
    # the bf16 x 3 build's 1-D grid: one interleaved group of eight and a remainder of three; two full groups; five row blocks (a
    # wave's second row block clamped), a remainder of one, sigma(alpha) = 1 in one cell; 32-row tiles (the wide path's C = 256)
    ("b3_k11", 128, 60, 16, "bfloat16", 11, "", (4, 2, 0, True, True)),
    ("b3_k16_mt", 128, 60, 16, "bfloat16", 16, "multitask", (4, 2, 0, True, True)),
    ("b3_r72_k9", 72, 60, 16, "bfloat16", 9, "alphas,sig1", (4, 2, 0, True, True)),
    ("b3_me32_k9", 128, 256, 16, "bfloat16", 9, "", (2, 2, 0, True, True)),
    ("b3_lm1_k9", 100, 23, 16, "bfloat16", 9, "lm1", (4, 2, 0, True, True)),
    # the 2-D grid builds
    ("r16_bf16", 16, 60, 20, "bfloat16", 9, "", (4, 1, 1, True, False)),
    ("r16_f32_lm1", 16, 23, 20, "float32", 9, "lm1", (4, 1, 1, False, False)),
    ("r24_bf16", 24, 17, 16, "bfloat16", 9, "", (4, 1, 2, True, False)),
    ("r32_f16", 32, 60, 16, "float16", 9, "", (4, 1, 2, False, False)),
    ("r64_f32", 64, 60, 16, "float32", 9, "", (4, 1, 0, False, False)),
    ("r64_c256", 64, 256, 16, "float16", 9, "", (2, 1, 0, False, False)),
    ("r128_f32", 128, 60, 16, "float32", 9, "", (4, 2, 0, False, False)),
    ("r128_c256", 128, 256, 16, "float32", 9, "", (2, 2, 0, False, False)),
    ("r160_f16", 160, 17, 16, "float16", 9, "", (4, 4, 0, False, False)),
    ("r256_bf16", 256, 60, 16, "bfloat16", 9, "", (2, 4, 0, False, False)),
    ("r300_f32", 300, 17, 16, "float32", 9, "", (2, 8, 0, False, False)),
    ("r512_f16", 512, 60, 16, "float16", 9, "", (1, 8, 0, False, False)),
]
REPORT_IDS = [c[0] for c in REPORT_CASES]

# Every k_eval instantiation of the table (builds.hip.h: BUILDS_EVAL_ROWS): the split builds, the three bf16 x 3 builds, the plain ones.
ALL_BUILDS = ([(m, 1, s, x, False) for m in (4, 2, 1) for s in (1, 2) for x in (False, True)] + [(m, 2, 0, True, True) for m in (4, 2, 1)] +
              [(m, n, 0, False, False) for m in (4, 2, 1) for n in (1, 2, 4, 8)])
# The tile is 64 rows unless (64 * (max(136, Cp + 4) + Rp + 8)) * 4 exceeds 80 KiB, i.e. Rp + max(136, Cp + 4) > 312, and 32 rows
# unless Rp + max(136, Cp + 4) > 632; Cp <= 256 (C <= 256), so max(136, Cp + 4) <= 260.
_SPLIT = "one or two row blocks: Rp <= 32, and 32 + 260 = 292 is not over 312, so the tile is always 64 rows"
_ME16 = "a 16-row tile needs Rp + 260 > 632, Rp > 372: only with eight row blocks per wave"
UNREACHABLE_BUILDS = {
    **{(m, 1, s, x, False): _SPLIT for m in (2, 1) for s in (1, 2) for x in (False, True)},
    (1, 2, 0, True, True): _ME16, (1, 1, 0, False, False): _ME16, (1, 2, 0, False, False): _ME16, (1, 4, 0, False, False): _ME16,
    (4, 8, 0, False, False): "eight row blocks per wave: Rp >= 272, and 272 + 136 = 408 is over 312, so the tile is never 64 rows",
}

POISON_BIAS = 40.0       # sigmoid(40 + x) rounds to 1 in float32
# the control: the float32 oracle's logits stay below 16 (1 - sigmoid is still a float32 above 0).  The largest of 12, 10, 8, ... at
# which the float32 oracle's loss of the first batch uses under a quarter of ref64's bound on all four schedules' inputs (measured
# 0.008, 0.019, 0.005, 0.006; at 12: 0.31 on general_mb2) — tests/test_report_cpu.py::test_control_bias_calibration_margin
CONTROL_BIAS = 10.0


# ------------------------------------------------------------------------------------------------ pure helpers (no device)
def best_epoch_rule(metrics, threshold):
    """train_searchable/ntu.py:17-18,82-86 as a pure function: (epoch, best) — the FIRST epoch whose dev metric strictly exceeds
    every earlier one and the threshold, -1 (the initial parameters) if none does; best is that metric, else the threshold."""
    best, epoch = float(threshold), -1
    for e, m in enumerate(metrics):
        if float(m) > best:
            best, epoch = float(m), e
    return epoch, best


def report_hyper(case):
    _, R, C, B, dtype, K, extra, build = case
    return O.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, alphas="alphas" in extra, multitask="multitask" in extra,
                   loss_mode=1 if "lm1" in extra else 0, s_sizes=W_A["s"], v_sizes=W_A["v"], epochs=E_REPORT)


def report_inputs(case):
    """What a REPORT_CASES entry trains, as numpy: K candidates of 1..4 cells with mixed taps and non-linearities, each with its
    own init seed (perturb_bn) and dropout seed, a train table of 2 B + 3 rows, a dev table of N_DEV rows, the learning rates."""
    cid, R, C, B, dtype, K, extra, build = case
    hp = report_hyper(case)
    base = 7000 + 100 * REPORT_IDS.index(cid) + SEED_SHIFT.get(cid, 0)
    rng = np.random.default_rng(base)
    confs = [np.array([[rng.integers(4), rng.integers(4), rng.integers(3)] for _ in range(1 + (k + 2) % 4)]) for k in range(K)]
    for c in confs:     # at most MAX_UNBOUNDED_CELLS ReLU / LeakyReLU cells per candidate: each multiplies the error scale M by ~ sqrt(R) / 2,
        while (c[:, 2] != 1).sum() > (MAX_UNBOUNDED_CELLS if R <= 256 else 1):       # and ref64 would leave too many dev rows open (check_conditions)
            c[rng.choice(np.flatnonzero(c[:, 2] != 1)), 2] = 1
    p0s = [O.init_params(c, hp, base + 1 + k, perturb_bn=True) for k, c in enumerate(confs)]
    for p in p0s:       # a head bias of its own per candidate: untrained candidates would else report nearly the same loss (and, under
        p["central_classifier.bias"] = rng.standard_normal(C).astype(F32)      # the multi-label head, the very same F1 sum)
    if "sig1" in extra:
        p0s[0]["alphas.0.alpha_x"] = np.array([40.0], F32)
    tup = (cid, R, C, B, W_A, None, True, 0.5, extra)
    ntr = 2 * B + 3
    ttr, tdv = G.case_table(tup, hp, ntr, base + 50, dtype), G.case_table(tup, hp, N_DEV, base + 51, dtype)
    nb = -(-ntr // B)
    return dict(hp=hp, confs=confs, p0s=p0s, seeds=[base + 20 + k for k in range(K)], ttr=ttr, tdv=tdv, dtype=dtype,
                etas=O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / B, E_REPORT * nb))


def oracle_epochs(conf, hp, p0, ttr, seed, etas, epochs):
    """The float32 oracle's parameters after each epoch (sequential sample order) and its train loss sums."""
    params = {k: v.copy() for k, v in p0.items()}
    keys, st = O.trainable_keys(conf, hp), O.AdamState()
    N = len(ttr["label"])
    states, losses, g = [], [], 0
    for _ in range(epochs):
        run = 0.0
        for r0 in range(0, N, hp.B):
            batch = {k: v[r0:r0 + hp.B] for k, v in ttr.items()}
            feats = {k: v for k, v in batch.items() if k not in ("label", "multilabel")}
            logits, cache = O.forward(params, conf, hp, feats, True, seed=seed, step=g)
            if hp.loss_mode == 1:
                loss, dl = O.bce_loss(logits, batch["multilabel"], G.pos_weight(hp))
            else:
                loss, dl, _ = O.ce_loss(logits, batch["label"])
            grads = O.backward(params, hp, cache, dl)
            O.bn_update_running(params, hp, cache)
            O.adam_step(params, grads, st, float(etas[g]), hp, keys)
            run += float(loss) * len(batch["label"])
            g += 1
        states.append({k: v.copy() for k, v in params.items()})
        losses.append(run)
    return states, losses


def dev_ref(P, conf, hp, t, rows=None):
    """ref64's (loss_sum, bound, count_lo, count_hi) of a dev pass over `rows` (all) of table t with parameters P."""
    sl = slice(None) if rows is None else rows
    f = {k: v[sl] for k, v in G.feats_of(t).items()}
    lg, Ml, _ = R64.forward(P, conf, hp, f, False)
    return R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, labels=t["label"][sl], vlogit=f.get("vlogit"), slogit=f.get("slogit"),
                         z=t["multilabel"][sl] if "multilabel" in t else None, pos_weight=G.pos_weight(hp))


def ambiguous_rows(ref, hp, n):
    _, _, lo, hi = ref
    return int(round((hi - lo - 2 * n) / float(1 << 32))) if hp.loss_mode == 1 else hi - lo


def check_conditions(refs, hp, n, tag, margin=1.0, spare=0):
    """What keeps the comparison from hiding a failure; refs[k] = dev_ref of candidate k for one epoch.  Every pair of candidates
    has disjoint loss intervals; at most MAX_AMBIGUOUS rows per candidate are open; multi-label: every candidate's count window is
    smaller than the gap between any two candidates' windows.  margin / spare: the CPU check on oracle-trained parameters asks for
    intervals `margin` times as wide and `spare` open rows fewer, so that the engine's own parameters (a float32 trajectory of
    their own) still meet the conditions as stated."""
    K = len(refs)
    for k in range(K):
        assert ambiguous_rows(refs[k], hp, n) <= MAX_AMBIGUOUS - spare, (tag, k, refs[k])
    for i in range(K):
        for j in range(i + 1, K):
            (li, bi, loi, hii), (lj, bj, loj, hij) = refs[i], refs[j]
            assert abs(li - lj) > margin * (bi + bj), f"{tag}: candidates {i} and {j} have overlapping loss intervals ({li} +- {bi}, {lj} +- {bj})"
            if hp.loss_mode == 1:
                gap = max(loi, loj) - min(hii, hij)
                assert gap > margin * max(hii - loi, hij - loj), f"{tag}: count windows of candidates {i} and {j}: [{loi}, {hii}], [{loj}, {hij}]"


# ------------------------------------------------------------------------------------------------ GPU plumbing
def make_population(ehp, confs, dev, seeds, env=None, chunk_cols=0, pos_weight=None):
    from mfas_amd import Population
    env = env or {}
    os.environ.update(env)
    try:
        pop = Population(ehp, confs, dev, drop_seeds=seeds, chunk_cols=chunk_cols)
    finally:
        for k in env:
            os.environ.pop(k, None)
    if pos_weight is not None:
        pop.set_pos_weight(pos_weight)
    return pop


def plane_bytes(pop, k, plane=0):
    return pop.get_params(k, plane).cpu().numpy().tobytes()


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


# ------------------------------------------------------------------------------------------------ (c) status at every flagging site
WIDE_CONFS = ([[1, 2, 0], [0, 1, 2]], [[0, 1, 2]], [[1, 0, 0], [2, 2, 1], [0, 1, 0]])
# name: (R, C, B, env, chunk_cols, K, tap_bits, check, widths, confs)
STATUS_SCHEDULES = {name: GT.TRAIN_SCHEDULES[name] + (W_A, GT.SCHED_CONFS) for name in
                    ("persistent", "lean_chain", "general_mb1", "general_mb2", "general_mb4", "same_group", "chain_split")}
STATUS_SCHEDULES["persistent"] = STATUS_SCHEDULES["persistent"][:5] + (3,) + STATUS_SCHEDULES["persistent"][6:]
STATUS_SCHEDULES.update({
    "two_group": (32, 60, 16, {"MFAS_GROUPS": "2"}, 0, 12, 0, lambda s: s["persistent"] == 0 and s["groups"] == 2, W_A, GT.SCHED_CONFS),
    "wide": (80, 60, 33, {}, 0, 3, 0, lambda s: s["wide"] == 1, W_B, WIDE_CONFS),
})
STATUS_LM1 = ("persistent", "general_mb2", "chain_split", "wide")
STATUS_SEGMENTED = "general_mb1"
E_STATUS = 2


def status_inputs(name, lm1):
    from tests.helpers import engine_hyper
    R, C, B, env, cc, K, tap_bits, check, w, pool = STATUS_SCHEDULES[name]
    hp = O.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, loss_mode=1 if lm1 else 0, s_sizes=w["s"], v_sizes=w["v"], epochs=E_STATUS)
    confs = [np.array(pool[k % len(pool)]) for k in range(K)]
    ehp = engine_hyper(hp)
    ehp.tap_bits = tap_bits
    tup = (name, R, C, B, w, None, True, 0.5, "lm1" if lm1 else "")
    ntr = GT.train_rows(B)
    return dict(hp=hp, ehp=ehp, confs=confs, seeds=[5 + 3 * k for k in range(K)], env=env, cc=cc, check=check,
                p0s=[O.init_params(c, hp, 40 + k, perturb_bn=True) for k, c in enumerate(confs)],
                ttr=G.case_table(tup, hp, ntr, 61, "bfloat16"), tdv=G.case_table(tup, hp, G.N_EVAL, 62, "bfloat16"),
                etas=O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / B, E_STATUS * -(-ntr // B)))


def poisoned(p, how):
    q = {k: v.copy() for k, v in p.items()}
    if how == "nan":
        q["fusion_layers.0.0.weight"][3, 7] = np.nan
        assert int(q["fusion_layers.0.0.weight"][3:4, 7].view(np.uint32)[0]) == 0x7FC00000     # (never chain_split's all-ones sentinel)
    elif how is not None:
        q["central_classifier.bias"][5] = F32(how)
    return q


def first_batch_loss32(inp, k, params):
    """Candidate k's first train batch with the reference's formula in float32 (the numpy oracle): loss, largest logit."""
    hp = inp["hp"]
    batch = {key: v[:hp.B] for key, v in inp["ttr"].items()}
    feats = {key: v for key, v in batch.items() if key not in ("label", "multilabel")}
    with np.errstate(all="ignore"):
        logits, _ = O.forward({key: v.copy() for key, v in params.items()}, inp["confs"][k], hp, feats, True, seed=inp["seeds"][k], step=0)
        loss = O.bce_loss(logits, batch["multilabel"], G.pos_weight(hp))[0]
    return float(loss), float(np.max(logits))


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
