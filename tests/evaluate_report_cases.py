"""Case module: the evaluate-report cases, their inputs and the pure report checks."""
import numpy as np

from oracle import np_oracle as O
from tests import evaluate_cases as EC
from tests import ref64 as R64
from tests import ref64_cases as G


F32, F64 = np.float32, np.float64
U = R64.U


# EVAL_CASES' "c2" fails the conditions below (one of its members decides class 0 on every row: a single non-zero off-diagonal cell),
# so a case of the same size stands in for it there: the head biases are zero, which leaves both classes decided by every member.
# c2 itself stays in every comparison.
EXTRA_CASES = {"c2_spread": (("c2_spread", 16, 2, "float32", 5, 37, ""), 12196)}       # id -> (case, seed base)
REPORT_CASES = EC.EVAL_CASES + [c for c, _ in EXTRA_CASES.values()]


def report_inputs(case):
    """eval_inputs for EVAL_CASES; the same construction on a seed base of its own for EXTRA_CASES."""
    cid, R, C, dtype, K, N, extra = case
    if cid not in EXTRA_CASES:
        return EC.eval_inputs(case)
    base = EXTRA_CASES[cid][1]
    hp = EC.eval_hyper(case)
    rng = np.random.default_rng(base)
    confs = [np.array([[rng.integers(4), rng.integers(4), rng.integers(3)] for _ in range(1 + k % 2)]) for k in range(K)]
    p0s = [O.init_params(c, hp, base + 1 + k, perturb_bn=True) for k, c in enumerate(confs)]
    for p in p0s:
        p["central_classifier.bias"] = np.zeros(C, F32)
    tup = (cid, R, C, 16, G.W_A, None, True, 0.5, extra)
    return dict(hp=hp, confs=confs, p0s=p0s, seeds=[base + 20 + k for k in range(K)], tab=G.case_table(tup, hp, N, base + 50, dtype),
                dtype=dtype)


# ------------------------------------------------------------------------------------------------ the restatement
def decide32(x, mut=""):
    """The first maximum of every row of x (.., C); a NaN never wins, a NaN in class 0 decides class 0."""
    x = np.asarray(x, F32)
    a = np.where(np.isnan(x), F32(-np.inf), x)
    C = x.shape[-1]
    pred = C - 1 - np.argmax(a[..., ::-1], -1) if mut == "last_max" else np.argmax(a, -1)
    return np.where(np.isnan(x[..., 0]), 0, pred)


def rank32(x, labels, mut=""):
    """The number of classes that precede the label: score descending, NaN last, equal scores by lower class first."""
    x = np.asarray(x, F32)
    C = x.shape[-1]
    lab = np.broadcast_to(np.asarray(labels, np.int64), x.shape[:-1])[..., None]
    xl = np.take_along_axis(x, lab, -1)
    cls = np.arange(C)
    tie = (cls > lab) if mut == "rank_tie_high" else (cls < lab)
    with np.errstate(invalid="ignore"):
        before = np.where(np.isnan(xl), ~np.isnan(x) | tie, (x > xl) | ((x == xl) & tie))
        if mut == "nan_first":
            before = np.where(np.isnan(xl), (cls < lab) & np.isnan(x), before | np.isnan(x))
    return before.sum(-1)


def tally32(zs32, scores32, truth, hp, mut=""):
    """The report of slots (members zs32 [M][n][C], then the ensemble scores32 (n, C)) against `truth` (labels [n], or multilabel
    (n, C) under loss_mode 1), by comparisons only.  Returns {"confusion", "rank_hist"} or {"label_counts"}, int64, slot first."""
    rows = np.concatenate([np.asarray(zs32, F32), np.asarray(scores32, F32)[None]], 0)
    S, n, C = rows.shape
    if hp.loss_mode == 0:
        lab = np.asarray(truth, np.int64)
        pred, rank = decide32(rows, mut), rank32(rows, lab[None], mut)
        conf, hist = np.zeros((S, C, C), np.int64), np.zeros((S, C), np.int64)
        for s in range(S):
            np.add.at(conf[s], (pred[s], lab) if mut == "swap" else (lab, pred[s]), 1)
            np.add.at(hist[s], rank[s], 1)
        return dict(confusion=conf, rank_hist=hist)
    th = F32(hp.f1_threshold)
    pr = (rows >= th) if mut == "ge" else (rows > th)
    tr = np.broadcast_to(np.asarray(truth, F32) > 0.5, rows.shape)
    if mut == "swap_pos":
        pr, tr = tr, pr
    return dict(label_counts=np.stack([(pr & tr).sum(1), pr.sum(1), tr.sum(1)], -1).astype(np.int64))


def check_identities(rep, truth, hp, tag, nan_free=True):
    """What the arrays keep among themselves whatever the scores are."""
    n = len(truth)
    if hp.loss_mode == 0:
        conf, hist = rep["confusion"], rep["rank_hist"]
        C = hist.shape[1]
        assert (conf >= 0).all() and (hist >= 0).all(), tag
        assert (conf.sum((1, 2)) == n).all(), f"{tag}: a confusion slice does not sum to N"
        assert (conf.sum(2) == np.bincount(np.asarray(truth), minlength=C)[None]).all(), f"{tag}: row sums are not the label histogram"
        assert (hist.sum(1) == n).all(), f"{tag}: a rank histogram does not sum to N"
        cum = np.cumsum(hist, 1)
        assert (np.diff(cum, axis=1) >= 0).all() and (cum[:, -1] == n).all(), tag
        if nan_free:        # rank 0 is "decided correctly" on every row whose class-0 score is not NaN
            assert (np.trace(conf, axis1=1, axis2=2) == hist[:, 0]).all(), f"{tag}: trace differs from rank_hist[:, 0]"
    else:
        lc = rep["label_counts"]
        assert (lc >= 0).all() and (lc[..., 0] <= lc[..., 1]).all() and (lc[..., 0] <= lc[..., 2]).all(), tag
        assert (lc[..., 2] == (np.asarray(truth) > 0.5).sum(0)[None]).all(), f"{tag}: actual positives are not the table's"


def check_report(rep, zs32, scores32, truth, hp, tag, nan_free=True):
    """The checker: the arrays equal the restatement on the same float32 rows, exactly, and keep the identities."""
    want = tally32(zs32, scores32, truth, hp)
    assert set(want) <= set(rep), (tag, sorted(rep))
    for k, w in want.items():
        got = np.asarray(rep[k])
        assert got.shape == w.shape and got.dtype == np.int64, (tag, k, got.shape, got.dtype, w.shape)
        assert np.array_equal(got, w), f"{tag}: {k} differs from the restatement at {np.argwhere(got != w)[:4].tolist()}"
    check_identities(rep, truth, hp, tag, nan_free)


def open_elements(zs, hp, t):
    """loss_mode 1, per member: the elements whose decision the float64 statement leaves open (vote64 with M = 1, combine 0:
    |sigmoid64(z) - th| inside the element's bound), and the statement's decisions elsewhere.  Returns (open, predicted) [M][n][C]."""
    th = float(F32(hp.f1_threshold))
    opened, pred = [], []
    for m in range(len(zs)):
        ref = EC.vote64(zs[m:m + 1], EC.normalised(None, 1), hp, 0, EC.TAU_VOTE, **EC.table_columns(t, hp))
        opened.append(np.abs(ref["p"] - th) <= ref["bound"] + U * th)
        pred.append(ref["p"] > th)
    return np.stack(opened), np.stack(pred)


def count_window(opened, pred, multilabel):
    """(lo, hi) int64 [M][C][3]: the label counts the open elements leave, cell by cell."""
    tr = np.broadcast_to(np.asarray(multilabel, F32) > 0.5, pred.shape)
    lo_p, hi_p = pred & ~opened, pred | opened
    lo = np.stack([(lo_p & tr).sum(1), lo_p.sum(1), tr.sum(1)], -1)
    hi = np.stack([(hi_p & tr).sum(1), hi_p.sum(1), tr.sum(1)], -1)
    return lo.astype(np.int64), hi.astype(np.int64)
