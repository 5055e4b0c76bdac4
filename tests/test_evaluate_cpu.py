"""Population.evaluate (mfas_population_evaluate, k_vote) without a device: the float64 statement of the vote with its elementwise
error scale, a float32 restatement calibrated against it on every input the GPU file uses, the conditions that keep the comparison
from hiding a failure, five mutations the checker must catch, and the argument checks that need no GPU.

The statement (vote64).  A member's score row z_m is its logits (multitask: (logits + vlogit) + slogit, formed in float32 in that
order: an exact input of the vote); its probability row p_m is softmax(z_m - max z_m) (loss_mode 1: sigmoid(z_m)).  The weights are
normalised in double and rounded to float32 (normalised(): exact inputs as well).
  combine 0:  pbar = sum_m w_m p_m.
              The issue's scale, sum_m w_m p_mc (2 + |z_mc - max z_m|) + pbar_c (the argument of exp rounded at 2^-24 |z - max|, exp
              itself within one ulp, one unit for pbar), does NOT calibrate: the serial restatement reaches 1.84 on c60_bf16,
              element (51, 1) of the one-member list, because nothing in it pays for the row sum of C exponentials, the division or
              the product w p.  It is widened by derived terms, not the tau:
              M_vote = sum_m w_m p_mc (4 + |z_mc - max z_m| + S(C)) + (1 + S(M)) pbar_c,   S(n) = sqrt(3 (n - 1)) (sum_term: the
              rounding of an n-term sum), +2 for the division and the product.
              loss_mode 1: M_vote = 5 sum_m w_m p_mc + (1 + S(M)) pbar_c (exp, 1 + e, the division, the product; the sigmoid has no
              maximum to subtract and no row sum).
  combine 1:  zbar = sum_m w_m z_m with M_z = M sum_m w_m |z_mc| (a product and at most M - 1 additions of partial sums below
              sum_m w_m |z_mc|, whatever the order); pbar = softmax(zbar), and a score error delta moves p_c by at most
              p_c (delta_c + sum_j p_j delta_j):
              M_vote = pbar_c (M_z,c + sum_j pbar_j M_z,j) + pbar_c (4 + |zbar_c - max| + S(C)) + pbar_c;
              loss_mode 1: M_vote = pbar (1 - pbar) M_z + 5 pbar.
The GPU allowance is TAU_VOTE = 4 (the project's smallest tau, TAU_RUNSTAT): the kernel may order the class sum and the member
sum differently from the serial float32 restatement, which itself stays at or below 1 on every input (the calibration limit of
tests/test_ref64_cpu.py).  Worst ratios of the restatement per case (printed with -s): c2 0.250, c23_lm1 0.501, c60_bf16 0.412,
c70_mt 0.406, c256_bf16 0.426, r128_bf16 0.431, n1 0.237.
A row is AMBIGUOUS when the statement's top-two gap of pbar is within twice the row's largest bound (loss_mode 1: when a class
lies within its bound of the threshold); it may go either way, as in ref64.dev_stats.
"""
import math
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import test_gpu_ref64 as G

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


def run_checker(Z, weights, hp, combine, t, tag, mut="", tau=TAU_VOTE, record=None):
    """vote32 (possibly mutated) through the whole checker against vote64 on the same float32 scores."""
    cols = table_columns(t, hp)
    zs = member_scores(Z, hp, t.get("vlogit"), t.get("slogit"))
    ref = vote64(zs, normalised(weights, len(Z)), hp, combine, tau, **cols)
    got = vote32(Z, weights, hp, combine, vlogit=t.get("vlogit"), slogit=t.get("slogit"), mut=mut, **cols)
    if hp.loss_mode == 0:
        check_members(zs, got["preds"], tag)
    return check_vote(ref, got["scores"], got["corrects"], got["loss"], tag, record=record), ref, zs


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("case", EVAL_CASES, ids=EVAL_IDS)
def test_float32_restatement_calibration_and_conditions(case):
    """On every input the GPU file uses (the oracle's logits on the same seeds, every member list, both combines): the serial
    float32 restatement stays at or below 1 x 2^-24 M_vote, at most a quarter of the rows are ambiguous at the GPU's tau, and no
    member's top-two scores nearly tie."""
    inp = eval_inputs(case)
    hp, Zall = inp["hp"], oracle_logits(inp)
    worst = 0.0
    for members, weights in member_lists(case[4]):
        Z = Zall if members is None else Zall[members]
        for combine in (0, 1):
            tag = f"{case[0]} members {members} combine {combine}"
            r, _, zs = run_checker(Z, weights, hp, combine, inp["tab"], tag, tau=1.0)
            worst = max(worst, r)
            ref = vote64(zs, normalised(weights, len(Z)), hp, combine, TAU_VOTE, **table_columns(inp["tab"], hp))
            check_conditions(ref, zs, hp, tag)
    print(f"\n  vote32 / vote64 worst ratio, {case[0]:12s} {worst:.3f}")
    assert worst <= 1.0


def _mutation_case(cid):
    case = EVAL_CASES[EVAL_IDS.index(cid)]
    inp = eval_inputs(case)
    return inp, oracle_logits(inp)


def test_mutation_dropped_weight_fails():
    inp, Z = _mutation_case("c60_bf16")
    run_checker(Z[[6, 0, 2]], None, inp["hp"], 0, inp["tab"], "control")
    for combine in (0, 1):
        with pytest.raises(AssertionError):
            run_checker(Z[[6, 0, 2]], None, inp["hp"], combine, inp["tab"], "drop_weight", mut="drop_weight")


def test_mutation_softmax_without_the_maximum_fails_on_large_logits():
    inp, Z = _mutation_case("c60_bf16")
    big = (Z[[6, 0, 2]] * F32(400.0)).astype(F32)            # exp overflows float32 without the subtraction
    assert np.abs(big).max() > 100.0
    run_checker(big, None, inp["hp"], 0, inp["tab"], "control")
    with pytest.raises(AssertionError):
        run_checker(big, None, inp["hp"], 0, inp["tab"], "no_max", mut="no_max")


def test_mutation_last_maximum_fails_on_a_constructed_tie():
    inp, Z = _mutation_case("c60_bf16")
    tie = Z[[6, 0, 2]].copy()
    tie[1, 5, 40] = tie[1, 5, 3] = tie[1, 5].max() + F32(1.0)      # two equal maxima in one member's row: the first one counts
    run_checker(tie, None, inp["hp"], 0, inp["tab"], "control")
    with pytest.raises(AssertionError, match="first maximum"):
        run_checker(tie, None, inp["hp"], 0, inp["tab"], "last_max", mut="last_max")


def test_mutation_unnormalised_weights_fail():
    inp, Z = _mutation_case("c60_bf16")
    run_checker(Z[[6, 0, 2]], [2.0, 1.0, 1.0], inp["hp"], 0, inp["tab"], "control")
    with pytest.raises(AssertionError):
        run_checker(Z[[6, 0, 2]], [2.0, 1.0, 1.0], inp["hp"], 0, inp["tab"], "no_norm", mut="no_norm")
    with pytest.raises(AssertionError):      # (a softmax hides a common factor of the scores only when it is 1)
        run_checker(Z[[6, 0, 2]], [2.0, 1.0, 1.0], inp["hp"], 1, inp["tab"], "no_norm", mut="no_norm")


def test_mutation_multitask_sum_left_out_fails():
    inp, Z = _mutation_case("c70_mt")
    for combine in (0, 1):
        run_checker(Z, None, inp["hp"], combine, inp["tab"], "control")
        with pytest.raises(AssertionError):
            run_checker(Z, None, inp["hp"], combine, inp["tab"], "no_multitask", mut="no_multitask")


def test_weights_two_one_one_equal_a_repeated_member():
    """(2, 1, 1) on (a, b, c) is uniform on (a, a, b, c): the same statement, so the GPU file may hold one to the other's bound."""
    inp, Z = _mutation_case("c60_bf16")
    hp, cols = inp["hp"], table_columns(inp["tab"], inp["hp"])
    for combine in (0, 1):
        a = vote64(Z[[4, 1, 5]], normalised([2, 1, 1], 3), hp, combine, TAU_VOTE, **cols)
        b = vote64(Z[[4, 4, 1, 5]], normalised(None, 4), hp, combine, TAU_VOTE, **cols)
        assert np.abs(a["p"] - b["p"]).max() <= 1e-15


def test_python_argument_checks():
    from mfas_amd.engine import evaluate_arguments as ea
    mem, w, comb = ea(5, None, None, 0, "prob", 0, 0, False)
    assert mem.dtype == np.int32 and mem.tolist() == [0, 1, 2, 3, 4] and w is None and comb == 0
    mem, w, comb = ea(5, [1, 3, 1], [0.5, 2, 1], 3, "score", 1 << 20, 0, True)
    assert mem.tolist() == [1, 3, 1] and w.dtype == np.float32 and w.tolist() == [0.5, 2.0, 1.0] and comb == 1
    for kw, msg in ((dict(members=[0, 5]), r"member 5 is outside \[0, 5\)"), (dict(members=[-1]), r"member -1 is outside"),
                    (dict(members=[]), "no members"), (dict(weights=[1.0]), "1 weights for 2 members"),
                    (dict(weights=[1.0, -0.5]), "finite and >= 0"), (dict(weights=[1.0, float("nan")]), "finite and >= 0"),
                    (dict(weights=[1.0, float("inf")]), "finite and >= 0"), (dict(weights=[0.0, 0.0]), "sum to 0"),
                    (dict(plane=1), "plane 1"), (dict(combine="mean"), "combine 'mean'"), (dict(scratch_bytes=-1), "scratch_bytes -1"),
                    (dict(loss_mode=1, return_preds=True), "return_preds with loss_mode 1")):
        args = dict(members=[0, 1], weights=None, plane=0, combine="prob", scratch_bytes=0, loss_mode=0, return_preds=False)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            ea(5, **args)


def test_header_exports_and_ctypes_agree_on_evaluate():
    import __graft_entry__ as ge
    ge.build()
    from mfas_amd import _lib
    name = "mfas_population_evaluate"
    hdr = open(os.path.join(ROOT, "include", "mfas_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "the header does not declare " + name
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert name in _lib.EXPORTS
    fn = getattr(_lib.lib(), name)
    assert len(fn.argtypes) == len(params) == 12, (len(fn.argtypes), params)
    import ctypes
    for p, a in zip(params, fn.argtypes):       # by-value integers as the header sizes them; everything else a pointer
        want = ctypes.c_int64 if p.startswith("int64_t ") else (ctypes.c_int32 if p.startswith("int32_t ") and "*" not in p else None)
        assert (a is want) if want else (a in (ctypes.c_void_p, ctypes.POINTER(_lib.mfas_table))), (p, a)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert name in doc
    import mfas_amd
    assert callable(mfas_amd.test_population_track_acc) and hasattr(mfas_amd.Population, "evaluate")
    assert math.isclose(TAU_VOTE, 4.0)
