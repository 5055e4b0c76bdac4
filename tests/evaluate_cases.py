"""Case module: the evaluate cases, their inputs, the float32 / float64 vote and the pure checks."""
import math
import os

import numpy as np

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import ref64_cases as G


F32, F64 = np.float32, np.float64
U = R64.U
TAU_VOTE = G.TAU_RUNSTAT        # 4.0
TINY = 2.0 ** -126
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (id, R, C, table dtype, K, N, extra)      extra: multitask / lm1 (loss_mode 1, positive weights)
EVAL_CASES = [
    ("c2", 16, 2, "float32", 5, 37, ""),                    # fewer classes than a lane holds
    ("c23_lm1", 16, 23, "float32", 6, 37, "lm1"),           # odd; the multi-label head
    ("c60_bf16", 16, 60, "bfloat16", 7, 150, ""),           # not a multiple of the lane group; more than one workgroup and row block
    ("c70_mt", 16, 70, "float32", 5, 37, "multitask"),      # more than 64: the 32-lane rows
    ("c256_bf16", 16, 256, "bfloat16", 5, 37, ""),          # the limit: 64 lanes, four classes each
    ("r128_bf16", 128, 60, "bfloat16", 9, 37, ""),          # a second k_eval build (bf16 x 3) feeds the kernel
    ("n1", 16, 60, "float32", 5, 1, ""),                    # a single row
]
EVAL_IDS = [c[0] for c in EVAL_CASES]
MAX_AMBIGUOUS_FRACTION = 0.25


def member_lists(K):
    """(members, weights) per case: M = 1, M = 3, M = K (None: all), and a list with a repeated member under unequal weights."""
    return [([2], None), ([K - 1, 0, 2], None), (None, None), ([1, 3, 1, 0], [0.5, 2.0, 1.0, 0.25])]


def eval_hyper(case):
    _, R, C, dtype, K, N, extra = case
    return O.Hyper(R=R, C=C, B=16, bn=True, drpt=0.5, multitask="multitask" in extra, loss_mode=1 if "lm1" in extra else 0,
                   s_sizes=G.W_A["s"], v_sizes=G.W_A["v"], epochs=1)


def eval_inputs(case):
    """K candidates of one or two cells, each with its own parameters and head bias, and a table of N rows, as numpy."""
    cid, R, C, dtype, K, N, extra = case
    hp = eval_hyper(case)
    base = 9100 + 100 * EVAL_IDS.index(cid)
    rng = np.random.default_rng(base)
    confs = [np.array([[rng.integers(4), rng.integers(4), rng.integers(3)] for _ in range(1 + k % 2)]) for k in range(K)]
    p0s = [O.init_params(c, hp, base + 1 + k, perturb_bn=True) for k, c in enumerate(confs)]
    for p in p0s:
        p["central_classifier.bias"] = rng.standard_normal(C).astype(F32)
    tup = (cid, R, C, 16, G.W_A, None, True, 0.5, extra)
    return dict(hp=hp, confs=confs, p0s=p0s, seeds=[base + 20 + k for k in range(K)], tab=G.case_table(tup, hp, N, base + 50, dtype),
                dtype=dtype)


def oracle_logits(inp):
    """[K][N][C] float32: the numpy oracle's eval-mode forward of every candidate."""
    t = inp["tab"]
    return np.stack([np.asarray(O.forward(p, c, inp["hp"], G.feats_of(t), False)[0], F32) for p, c in zip(inp["p0s"], inp["confs"])])


# ------------------------------------------------------------------------------------------------ the statement
def normalised(weights, M):
    """The weights as the kernel reads them: divided by their sum in double, rounded to float32."""
    w = np.ones(M, F64) if weights is None else np.asarray(weights, F64)
    return (w / w.sum()).astype(F32)


def member_scores(Z, hp, vlogit=None, slogit=None):
    """The members' score rows in float32: the logits, or (logits + vlogit) + slogit in that order under multitask."""
    Z = np.asarray(Z, F32)
    if hp.multitask and hp.loss_mode == 0:
        return (Z + np.asarray(vlogit, F32)[None]) + np.asarray(slogit, F32)[None]
    return Z


def first_argmax(a):
    return np.argmax(a, -1)         # (numpy returns the first maximum)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def sum_term(n):
    """The rounding of an n-term float32 sum of non-negative terms, in units of 2^-24 of the sum: n - 1 additions, each rounding a
    partial sum no larger than the total by at most 2^-24 of it, independently and to either side.  Their sum has a standard
    deviation below sqrt((n - 1) / 3); three of those, sqrt(3 (n - 1)), are taken (the worst case n - 1 would let 255 units pass
    at C = 256).  Sound for any summation order: no order makes more than n - 1 additions."""
    return math.sqrt(3.0 * max(n - 1, 0))


def vote64(zs, wn, hp, combine, tau, labels=None, z=None, pos_w=None, dz=None):
    """The vote in float64 on the score rows zs [M][n][C] and weights wn [M], taken as exact.  dz [M][n] (optional): a bound on
    every element of a member's row of zs (the end-to-end comparison: the scores themselves carry ref64's logit bound); a softmax
    moves by at most p (exp(2 dz) - 1) then.  Returns p (n, C), bound (absolute, elementwise: tau 2^-24 M_vote + the dz term),
    amb (n), lo / hi (the ensemble's count window: rows, or 32.32 fixed-point F1), loss (sum) and loss_bound."""
    zs = np.asarray(zs, F64)
    Mm, n, C = zs.shape
    w = np.asarray(wn, F64)[:, None, None]
    dz = np.zeros((Mm, n)) if dz is None else np.asarray(dz, F64)
    Dz = (w[:, :, 0] * dz).sum(0)
    Mz = Mm * (w * np.abs(zs)).sum(0)
    if hp.loss_mode == 0:
        if combine == 0:
            d = zs - zs.max(2, keepdims=True)
            e = np.exp(d)
            p = e / e.sum(2, keepdims=True)
            pbar = (w * p).sum(0)
            Mv = (w * p * (4.0 + np.abs(d) + sum_term(C))).sum(0) + (1.0 + sum_term(Mm)) * pbar
            extra = (w * p * np.expm1(2.0 * dz)[:, :, None]).sum(0)
        else:
            zb = (w * zs).sum(0)
            d = zb - zb.max(1, keepdims=True)
            e = np.exp(d)
            pbar = e / e.sum(1, keepdims=True)
            Mv = pbar * (Mz + (pbar * Mz).sum(1, keepdims=True)) + pbar * (4.0 + np.abs(d) + sum_term(C)) + pbar
            extra = pbar * np.expm1(2.0 * Dz)[:, None]
        bound = tau * U * Mv + extra + R64.UNDERFLOW      # (a float32 below 2^-126 is rounded at 2^-149, or flushed to 0)
        order = np.argsort(-pbar, 1, kind="stable")
        rows_i = np.arange(n)
        top = pbar[rows_i, order[:, 0]]
        second = pbar[rows_i, order[:, 1]] if C > 1 else np.full(n, -np.inf)
        amb = (top - second) <= 2.0 * bound.max(1)
        correct = order[:, 0] == labels
        lo = int((correct & ~amb).sum())
        hi = lo + int(amb.sum())
        pl, bl = pbar[rows_i, labels], bound[rows_i, labels]
        rows = -np.log(np.maximum(pl, TINY))
        lossb = bl / np.maximum(pl - bl, 1e-300) + 4 * U * (np.abs(rows) + 1.0)
    else:
        pw = np.ones(C) if pos_w is None else np.asarray(pos_w, F64)
        if combine == 0:
            p = _sig(zs)
            pbar = (w * p).sum(0)
            Mv = 5.0 * (w * p).sum(0) + (1.0 + sum_term(Mm)) * pbar
            extra = (w * p * np.expm1(2.0 * dz)[:, :, None]).sum(0)
            rows, lossb = np.zeros(n), np.zeros(n)          # reported as 0
        else:
            zb = (w * zs).sum(0)
            pbar = _sig(zb)
            Mv = pbar * (1.0 - pbar) * Mz + 5.0 * pbar
            extra = pbar * np.expm1(2.0 * Dz)[:, None]
            rows = R64.bce_rows(zb, z, pw)
            lossb = (np.maximum(pw, 1.0)[None, :] * (tau * U * Mz + Dz[:, None])).mean(1) + 64 * U * (rows + 1.0)
        bound = tau * U * Mv + extra + R64.UNDERFLOW      # (a float32 below 2^-126 is rounded at 2^-149, or flushed to 0)
        th = float(F32(hp.f1_threshold))
        amb = (np.abs(pbar - th) <= bound + U * th).any(1)
        pr, tr = pbar > th, np.asarray(z, F64) > 0.5
        den = pr.sum(1) + tr.sum(1)
        f1 = np.where(den > 0, 2.0 * (pr & tr).sum(1) / np.maximum(den, 1), 0.0)
        one = float(1 << 32)
        base = float(np.floor(f1[~amb] * one).sum())
        lo, hi = base - n, base + one * amb.sum() + n
    return dict(p=pbar, M=Mv, bound=bound, amb=amb, lo=lo, hi=hi, loss=float(rows.sum()), loss_bound=float(lossb.sum()))


def check_vote(ref, scores, corrects, loss_sum, tag, record=None):
    """The checker: the ensemble's probabilities elementwise inside the statement's bound, its count inside the window the ambiguous
    rows leave, its loss sum inside the summed row bound.  Returns the worst ratio of the probabilities (in units of the bound)."""
    got = np.asarray(scores, F64)
    assert got.shape == ref["p"].shape, (tag, got.shape, ref["p"].shape)
    r = R64.assert_close64(got, ref["p"], ref["bound"] / U, 1.0, f"{tag} scores", record=record)
    assert ref["lo"] <= corrects <= ref["hi"], f"{tag} ensemble count: got {corrects}, the statement allows [{ref['lo']}, {ref['hi']}]"
    assert abs(float(loss_sum) - ref["loss"]) <= ref["loss_bound"], \
        f"{tag} ensemble loss sum: got {float(loss_sum)!r}, statement {ref['loss']!r}, bound {ref['loss_bound']:.3g}"
    return r


def check_members(zs32, preds, tag):
    """Every member's decision is the FIRST maximum of its float32 score row, exactly."""
    want = first_argmax(np.asarray(zs32, F32))
    assert np.array_equal(np.asarray(preds), want), f"{tag}: member decisions differ from the first maximum at {np.argwhere(np.asarray(preds) != want)[:4].tolist()}"


def check_conditions(ref, zs32, hp, tag):
    """At most a quarter of the rows ambiguous; no member's top-two scores within 1e-5 relative (loss_mode 0)."""
    n = len(ref["amb"])
    assert ref["amb"].sum() <= MAX_AMBIGUOUS_FRACTION * n, f"{tag}: {int(ref['amb'].sum())} of {n} rows are ambiguous"
    if hp.loss_mode == 0 and zs32.shape[2] > 1:
        s = np.sort(np.asarray(zs32, F64), 2)
        gap = s[:, :, -1] - s[:, :, -2]
        assert (gap > 1e-5 * np.maximum(np.abs(s[:, :, -1]), np.abs(s[:, :, -2]))).all(), f"{tag}: a member's top-two scores nearly tie"


# ------------------------------------------------------------------------------------------------ the float32 restatement
def _serial_sum(a):
    """Row sums of a float32 (n, C) array, class after class in float32."""
    s = np.zeros(a.shape[0], F32)
    for c in range(a.shape[1]):
        s = (s + a[:, c]).astype(F32)
    return s


def vote32(Z, weights, hp, combine, labels=None, vlogit=None, slogit=None, z=None, pos_w=None, mut=""):
    """The vote in float32 with serial sums, members in list order.  mut: one of the mutations the checker must catch."""
    Z = np.asarray(Z, F32)
    Mm, n, C = Z.shape
    wn = normalised(weights, Mm)
    if mut == "no_norm":
        wn = np.asarray(weights, F32)
    zs = Z if mut == "no_multitask" else member_scores(Z, hp, vlogit, slogit)
    amax = (lambda a: C - 1 - np.argmax(a[:, ::-1], 1)) if mut == "last_max" else first_argmax
    one = F32(1.0)
    acc = np.zeros((n, C), F32)
    preds = np.zeros((Mm, n), np.int64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for m in range(Mm):
            s = zs[m]
            if hp.loss_mode == 0:
                preds[m] = amax(s)
            if mut == "drop_weight" and m == 1:
                continue
            if combine == 1:
                term = wn[m] * s
            elif hp.loss_mode == 0:
                mx = np.zeros(n, F32) if mut == "no_max" else s.max(1)
                e = np.exp((s - mx[:, None]).astype(F32)).astype(F32)
                term = wn[m] * (e / _serial_sum(e)[:, None]).astype(F32)
            else:
                term = wn[m] * (one / (one + np.exp(-s).astype(F32))).astype(F32)
            acc = (acc + term.astype(F32)).astype(F32)
        if hp.loss_mode == 0:
            if combine == 1:
                e = np.exp((acc - acc.max(1)[:, None]).astype(F32)).astype(F32)
                acc = (e / _serial_sum(e)[:, None]).astype(F32)
            pred = amax(acc)
            pl = acc[np.arange(n), labels]
            rows = -np.log(np.where(pl < F32(TINY), F32(TINY), pl).astype(F32)).astype(F32)
            corr = int((pred == labels).sum())
        else:
            rows = np.zeros(n, F32)
            if combine == 1:
                acc = (one / (one + np.exp(-acc).astype(F32))).astype(F32)
                pw, t = np.asarray(pos_w, F32), np.asarray(z, F32)
                rows = (_serial_sum((pw[None] * t * -np.log(acc) + (one - t) * -np.log(one - acc)).astype(F32)) / F32(C)).astype(F32)
            pr, tr = acc > F32(hp.f1_threshold), np.asarray(z, F32) > 0.5
            tp, den = (pr & tr).sum(1), pr.sum(1) + tr.sum(1)
            corr = int(sum(((2 * int(a)) << 32) // int(b) if b > 0 else 0 for a, b in zip(tp, den)))
    return dict(scores=acc, preds=preds, corrects=corr, loss=float(rows.astype(F64).sum()))


def table_columns(t, hp):
    return dict(labels=t["label"], z=t.get("multilabel"), pos_w=G.pos_weight(hp) if hp.loss_mode == 1 else None)
