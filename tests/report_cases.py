"""Case module: what train() reports: the cases, their inputs, the float32 oracle's epochs and the pure conditions."""
import numpy as np

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import train_cases as GT
from tests.ref64_cases import W_A, W_B


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

# Every k_eval instantiation of the table (builds.hip.h: BUILDS_EVAL_ROWS, which also says why the other argument combinations are not
# built): the split builds, the two bf16 x 3 builds, the plain ones.
ALL_BUILDS = ([(4, 1, s, x, False) for s in (1, 2) for x in (False, True)] + [(m, 2, 0, True, True) for m in (4, 2)] +
              [(4, n, 0, False, False) for n in (1, 2, 4)] + [(2, n, 0, False, False) for n in (1, 2, 4, 8)] + [(1, 8, 0, False, False)])

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
