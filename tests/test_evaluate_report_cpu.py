"""Population.evaluate(report=True) (mfas_population_evaluate_report, k_tally) without a device: a numpy restatement of the tallies
that only compares, the identities the arrays keep among themselves, the conditions on the inputs that keep the GPU comparison from
hiding a failure, six mutations the checker must catch, report_metrics against its definitions (and sklearn where it imports), and
the agreement of header, exports, ctypes and INTEGRATION.md on the new entry.

The statement (tally32).  A SLOT is a member of the list (in list order) or, last, the ensemble.  Its score row is float32: a
member's score row as the vote reads it (test_evaluate_cpu.member_scores), the ensemble's probabilities as k_vote wrote them.
  loss_mode 0   decision: the first maximum, a NaN never winning a comparison, a NaN in class 0 deciding class 0;
                confusion[s][label][decision] += 1;
                rank of the label: the number of classes before it in the order "score descending, NaN last, equal scores by lower
                class first"; rank_hist[s][rank] += 1.
  loss_mode 1   the slot's row holds PROBABILITIES (a member's float32 sigmoid — what a one-member "prob" vote returns as scores);
                per class predicted = p > float32(f1_threshold), actual = multilabel > 0.5;
                label_counts[s][c] += (predicted and actual, predicted, actual).
Everything is an integer count of comparisons of float32 numbers: the GPU file holds the engine to it exactly, with no tolerance.
"""
import inspect
import os
import re

import numpy as np
import pytest

from tests import evaluate_cases as EC
from tests.evaluate_report_cases import F32, F64, REPORT_CASES, check_report, count_window, decide32, open_elements, report_inputs, tally32

ROOT = EC.ROOT
REPORT_IDS = [c[0] for c in REPORT_CASES]
CONDITIONS_WAIVED = ("c2",)


def truth_of(t, hp):
    return t["multilabel"] if hp.loss_mode == 1 else t["label"]


def member_probabilities(Z, hp):
    """loss_mode 1: every member's float32 sigmoid, as a one-member "prob" vote returns it (weight 1: 0 + 1 * p is exact)."""
    return np.stack([EC.vote32(Z[m:m + 1], None, hp, 0, z=np.zeros(Z.shape[1:], F32))["scores"] for m in range(len(Z))])


def oracle_slots(inp, Zall, members, weights, combine):
    """The slots of one evaluate call on the oracle's logits: (member rows, ensemble rows) as tally32 takes them."""
    hp, t = inp["hp"], inp["tab"]
    Z = Zall if members is None else Zall[members]
    v = EC.vote32(Z, weights, hp, combine, vlogit=t.get("vlogit"), slogit=t.get("slogit"), **EC.table_columns(t, hp))
    zs = member_probabilities(Z, hp) if hp.loss_mode == 1 else EC.member_scores(Z, hp, t.get("vlogit"), t.get("slogit"))
    return zs, v["scores"]


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def check_input_conditions(rep, case, tag):
    """On the restatement's output for the oracle's logits: what keeps a wrong report from passing unnoticed."""
    cid, C, N, extra = case[0], case[2], case[5], case[6]
    if "lm1" in extra:
        lc = rep["label_counts"]
        assert ((lc[..., 0] < lc[..., 1]).any(1)).all(), f"{tag}: a slot has no class with tp < predicted"
        assert ((lc[..., 0] < lc[..., 2]).any(1)).all(), f"{tag}: a slot has no class with tp < actual"
        return
    conf, hist = rep["confusion"], rep["rank_hist"]
    if N >= 37 and cid not in CONDITIONS_WAIVED:
        for s in range(len(conf)):
            off = conf[s] * (1 - np.eye(C, dtype=np.int64))
            assert (off > 0).sum() >= 2, f"{tag}: slot {s} has fewer than two non-zero off-diagonal cells"
            assert not np.array_equal(conf[s], conf[s].T), f"{tag}: slot {s}'s confusion is symmetric"
        if C > 5:
            assert (hist[:, 5:].sum(1) > 0).all(), f"{tag}: a slot has no row of rank >= 5 (top-5 would be trivial)"


@pytest.mark.parametrize("case", REPORT_CASES, ids=REPORT_IDS)
def test_restatement_identities_and_input_conditions(case):
    inp = report_inputs(case)
    hp, Zall = inp["hp"], EC.oracle_logits(inp)
    truth = truth_of(inp["tab"], hp)
    for members, weights in EC.member_lists(case[4]):
        for combine in (0, 1):
            tag = f"{case[0]} members {members} combine {combine}"
            zs, sc = oracle_slots(inp, Zall, members, weights, combine)
            rep = tally32(zs, sc, truth, hp)
            check_report(rep, zs, sc, truth, hp, tag)
            check_input_conditions(rep, case, tag)
            if members is not None and len(members) == 4:       # the repeated member: identical slices
                for k, v in rep.items():
                    assert np.array_equal(v[0], v[2]), (tag, k)
    if hp.loss_mode == 1:       # the share of elements the float64 statement leaves open: a condition on the input
        opened, pred = open_elements(np.asarray(Zall, F64), hp, inp["tab"])
        assert opened.mean() <= EC.MAX_AMBIGUOUS_FRACTION, opened.mean()
        lo, hi = count_window(opened, pred, truth)
        got = tally32(member_probabilities(Zall, hp), np.zeros(Zall.shape[1:], F32), truth, hp)["label_counts"][:-1]
        assert ((lo <= got) & (got <= hi)).all()


# ------------------------------------------------------------------------------------------------ mutations
def _slots(cid, members=(6, 0, 2), combine=0):
    case = EC.EVAL_CASES[EC.EVAL_IDS.index(cid)]
    inp = EC.eval_inputs(case)
    zs, sc = oracle_slots(inp, EC.oracle_logits(inp), list(members), None, combine)
    return inp["hp"], np.array(zs), np.array(sc), truth_of(inp["tab"], inp["hp"])


def _mutant_fails(hp, zs, sc, truth, mut, match=None):
    check_report(tally32(zs, sc, truth, hp), zs, sc, truth, hp, "control", nan_free=not np.isnan(zs[..., 0]).any())
    with pytest.raises(AssertionError, match=match):
        check_report(tally32(zs, sc, truth, hp, mut=mut), zs, sc, truth, hp, mut, nan_free=not np.isnan(zs[..., 0]).any())


def test_mutation_label_and_decision_swapped_fails():
    _mutant_fails(*_slots("c60_bf16"), "swap", match="confusion differs")


def test_mutation_last_maximum_fails_on_a_constructed_tie():
    hp, zs, sc, truth = _slots("c60_bf16")
    zs[1, 5, 40] = zs[1, 5, 3] = zs[1, 5].max() + F32(1.0)
    _mutant_fails(hp, zs, sc, truth, "last_max", match="confusion differs")


def test_mutation_rank_tie_towards_the_higher_class_fails():
    hp, zs, sc, truth = _slots("c60_bf16")
    lab = int(truth[7])
    other = lab + 1 if lab + 1 < hp.C else lab - 1
    zs[0, 7, other] = zs[0, 7, lab]         # one class ties with the label: it precedes the label only if it is the lower one
    _mutant_fails(hp, zs, sc, truth, "rank_tie_high", match="rank_hist differs")


def test_mutation_nan_ranked_first_fails():
    hp, zs, sc, truth = _slots("c60_bf16")
    zs[2, :, 3] = F32(np.nan)               # a NaN in class 3 of every row of one member: never before a label that has a score
    assert (truth != 3).any()
    _mutant_fails(hp, zs, sc, truth, "nan_first", match="rank_hist differs")
    zs[1, :, 0] = F32(np.nan)               # and a NaN in class 0: decides class 0, ranks last
    rep = tally32(zs, sc, truth, hp)
    assert rep["confusion"][1, :, 1:].sum() == 0 and rep["rank_hist"][1, hp.C - 1] == (truth == 0).sum()


def test_mutation_predicted_and_actual_swapped_fails():
    _mutant_fails(*_slots("c23_lm1", (5, 0, 2)), "swap_pos", match="label_counts differs")


def test_mutation_threshold_with_greater_or_equal_fails_on_a_score_equal_to_it():
    hp, zs, sc, truth = _slots("c23_lm1", (5, 0, 2))
    sc[4, 9] = F32(hp.f1_threshold)         # exactly the threshold: not predicted
    _mutant_fails(hp, zs, sc, truth, "ge", match="label_counts differs")


# ------------------------------------------------------------------------------------------------ report_metrics
def test_report_metrics_against_the_definitions():
    from mfas_amd.engine import report_metrics
    conf = np.zeros((2, 4, 4), np.int64)
    conf[0] = [[3, 1, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0], [1, 0, 0, 5]]         # class 2 has no rows; slot 1 is all zero
    hist = np.array([[8, 2, 1, 1], [0, 0, 0, 0]], np.int64)
    m = report_metrics(confusion=conf, rank_hist=hist, topk=(1, 2, 5))
    acc = m["per_class_accuracy"]
    assert acc.dtype == F64 and acc.shape == (2, 4)
    assert acc[0, 0] == 0.75 and acc[0, 1] == 0.0 and np.isnan(acc[0, 2]) and acc[0, 3] == 5.0 / 6.0 and np.isnan(acc[1]).all()
    assert m["topk"][1].tolist() == [8, 0] and m["topk"][2].tolist() == [10, 0] and m["topk"][5].tolist() == [12, 0]      # k > C: every row
    assert set(m) == {"per_class_accuracy", "topk"}
    with pytest.raises(ValueError, match="top-0"):
        report_metrics(rank_hist=hist, topk=(0,))
    #            tp pred act
    lc = np.array([[[2, 4, 3], [0, 0, 0], [0, 2, 0], [0, 0, 5], [6, 6, 6]], np.zeros((5, 3))], np.int64)     # an empty class; an all-zero slot
    m = report_metrics(label_counts=lc)
    assert m["precision"][0].tolist() == [0.5, 0.0, 0.0, 0.0, 1.0] and m["recall"][0].tolist() == [2.0 / 3.0, 0.0, 0.0, 0.0, 1.0]
    f1 = [4.0 / 7.0, 0.0, 0.0, 0.0, 1.0]
    assert m["f1"][0].tolist() == f1
    assert m["f1_micro"][0] == 16.0 / 26.0 and m["f1_macro"][0] == sum(f1) / 5.0
    assert m["f1_weighted"][0] == (f1[0] * 3.0 + 1.0 * 6.0) / 14.0
    for k in ("precision", "recall", "f1", "f1_micro", "f1_macro", "f1_weighted"):
        assert m[k].dtype == F64 and not m[k][1].any(), k         # 0 / 0 is 0
    one = report_metrics(label_counts=lc[0])                        # a single slot without the leading axis
    assert one["f1_micro"] == m["f1_micro"][0] and one["f1"].tolist() == f1


def test_report_metrics_against_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    from mfas_amd.engine import report_metrics
    rng = np.random.default_rng(5)
    n, C = 200, 7
    y = rng.integers(0, C - 1, n)                   # class C-1 has no rows
    x = rng.standard_normal((1, n, C)).astype(F32)
    hp0 = EC.eval_hyper(("x", 16, C, "float32", 1, n, ""))
    rep = tally32(x, x[0], y, hp0)
    want = skm.confusion_matrix(y, decide32(x[0]), labels=list(range(C)))
    assert np.array_equal(rep["confusion"][0], want) and np.array_equal(rep["confusion"][1], want)
    m = report_metrics(**rep)
    assert m["topk"][1][0] == skm.accuracy_score(y, decide32(x[0]), normalize=False)
    assert m["topk"][5][0] == round(skm.top_k_accuracy_score(y, x[0], k=5, labels=list(range(C)), normalize=False))
    hp1 = EC.eval_hyper(("x", 16, C, "float32", 1, n, "lm1"))
    p = rng.random((1, n, C)).astype(F32)
    t = (rng.random((n, C)) < 0.3).astype(F32)
    t[:, 2] = 0.0                                   # a class that is never actual
    p[0, :, 4] = 0.0                                # a class that is never predicted
    lc = tally32(p, p[0], t, hp1)["label_counts"]
    m = report_metrics(label_counts=lc)
    yp, yt = (p[0] > F32(hp1.f1_threshold)).astype(int), t.astype(int)
    for avg in ("micro", "macro", "weighted"):
        assert abs(m["f1_" + avg][0] - skm.f1_score(yt, yp, average=avg, zero_division=0)) <= 1e-12, avg
    assert np.abs(m["f1"][0] - skm.f1_score(yt, yp, average=None, zero_division=0)).max() <= 1e-12
    assert np.abs(m["precision"][0] - skm.precision_score(yt, yp, average=None, zero_division=0)).max() <= 1e-12
    assert np.abs(m["recall"][0] - skm.recall_score(yt, yp, average=None, zero_division=0)).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ the ABI and the entry points
def _declared_parameters(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "the header does not declare " + name
    return [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_header_exports_ctypes_and_integration_agree_on_the_report_entry():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from mfas_amd import _lib
    name, old = "mfas_population_evaluate_report", "mfas_population_evaluate"
    hdr = open(os.path.join(ROOT, "include", "mfas_hip.h")).read()
    params, params_old = _declared_parameters(hdr, name), _declared_parameters(hdr, old)
    assert len(params) == 15 and len(params_old) == 12
    assert params[:12] == params_old, "the first twelve parameters are mfas_population_evaluate's"
    assert [p.split()[0] + p.split()[-1] for p in params[12:]] == ["int64_t*confusion", "int64_t*rank_hist", "int64_t*label_counts"], params[12:]
    assert name in _lib.EXPORTS and old in _lib.EXPORTS
    fn, fo = getattr(_lib.lib(), name), getattr(_lib.lib(), old)
    assert len(fn.argtypes) == 15 and len(fo.argtypes) == 12 and list(fn.argtypes[:12]) == list(fo.argtypes)
    assert all(a is ctypes.c_void_p for a in fn.argtypes[12:])
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`" + name + "(" in doc and "confusion, rank_hist, label_counts)" in doc
    assert "Rank 0 coincides with" in doc and "Rank 0 coincides with" in open(os.path.join(ROOT, "mfas_amd", "csrc", "tally.hip.h")).read()


def test_report_keyword_and_flag():
    import main_found_ntu
    import mfas_amd
    from mfas_amd.engine import evaluate_arguments
    sig = inspect.signature(mfas_amd.Population.evaluate)
    assert list(sig.parameters)[-1] == "report" and sig.parameters["report"].default is False
    assert "report" not in inspect.signature(evaluate_arguments).parameters
    assert inspect.signature(mfas_amd.test_population_track_acc).parameters["report"].default is False
    assert mfas_amd.report_metrics is mfas_amd.engine.report_metrics
    base = ["--synthetic", "64", "32", "48", "--ensemble", "0", "1", "--no-multitask"]
    assert main_found_ntu.parse_args(base).report is False
    assert main_found_ntu.parse_args(base + ["--report"]).report is True


def test_report_lines():
    from mfas_amd.engine import report_metrics
    from mfas_amd.train_ntu import format_report
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 50, 8)).astype(F32)
    y = rng.integers(0, 8, 50)
    rep = tally32(x, x[0], y, EC.eval_hyper(("x", 16, 8, "float32", 2, 50, "")))
    rep.update(report_metrics(**rep))
    lines = format_report(rep, ["Member 0", "Member 1", "Ensemble"], 50.0)
    assert len(lines) == 3 and lines[0].split(" top-1")[1] == lines[2].split(" top-1")[1]
    assert re.fullmatch(r"Ensemble top-1: 0\.\d{4} top-5: 0\.\d{4} worst classes: (\d \(\d\.\d{3}\)(, )?){5}", lines[2]), lines[2]
    acc = rep["per_class_accuracy"][2]
    assert int(lines[2].split("worst classes: ")[1].split(" ")[0]) == int(np.argmin(acc))
    lc = np.array([[[2, 4, 3], [6, 6, 6]]] * 2, np.int64)
    m = dict(label_counts=lc, **report_metrics(label_counts=lc))
    assert format_report(m, ["Member 0", "Ensemble"], 9.0)[1] == "Ensemble F1 micro: {:.4f} macro: {:.4f} weighted: {:.4f}".format(
        16.0 / 19.0, (4.0 / 7.0 + 1.0) / 2.0, (4.0 / 7.0 * 3.0 + 6.0) / 9.0)
