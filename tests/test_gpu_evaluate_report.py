"""Population.evaluate(report=True) (mfas_population_evaluate_report: k_tally after every row block's k_vote) on the GPU, against the
comparison-only restatement of tests/test_evaluate_report_cpu.py (tally32) on the engine's OWN float32 rows.  Every comparison is
an exact integer equality; the only window is the one the float64 statement of a sigmoid leaves around the threshold (2, last part).

  1. single-label: member slots are the 2-D histogram of (label, member_preds) and tally32 of forward()'s score rows, the ensemble
     slot is tally32 of the returned scores, the traces are the counts the call reports, a repeated member repeats its slices;
  2. multi-label: a member's slot is the ensemble slot of its own one-member call (whose scores ARE its float32 sigmoid), the
     ensemble slot is the counts of the returned scores, and every member slot lies in the window vote64 leaves;
  3. invariances: run to run, scratch_bytes (64-row blocks of N = 150 among them), each array alone, with and without the
     caller's scores, and every other output byte-identical to the call without a report;
  4. NaN rows: a NaN in class 0 of one member, in class 3 of another;
  5. the new refusals, which change nothing;  6. main_found_ntu --ensemble ... --report.
Cases: REPORT_CASES = EVAL_CASES (C in {2, 23, 60, 70, 256}, N in {1, 37, 150}, K <= 9) and the two-class stand-in c2_spread.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_evaluate_report.py -m gpu -x -q
"""
import ctypes

import numpy as np
import pytest

from tests import evaluate_cases as EC
from tests import evaluate_report_cases as RC
from tests import evaluate_gpu as EV
from tests import gpu_support as G
from tests.gpu_support import dev  # noqa: F401
from tests.report_gpu import make_population

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SINGLE = [c[0] for c in RC.REPORT_CASES if "lm1" not in c[6]]
KEYS = ("confusion", "rank_hist", "label_counts")


# ------------------------------------------------------------------------------------------------ plumbing
def _build(inp, case, dev):
    """What evaluate_gpu.world builds, for inputs of this file's own."""
    from tests.helpers import engine_hyper
    hp = inp["hp"]
    pop = make_population(engine_hyper(hp), inp["confs"], dev, inp["seeds"], pos_weight=G.pos_weight(hp) if hp.loss_mode else None)
    for k, p in enumerate(inp["p0s"]):
        pop.set_state_dict(k, p)
    tab = G.gpu_table(inp["tab"], inp["dtype"], dev)
    fwd = [pop.forward(k, tab, count=True) for k in range(pop.K)]
    inp.update(pop=pop, gtab=tab, Z=np.stack([f[0].cpu().numpy() for f in fwd]), counts=[f[1] for f in fwd], case=case)
    return inp


def world(cid, dev):
    """evaluate_gpu.world; a case of EXTRA_CASES enters its cache built the same way."""
    if cid in RC.EXTRA_CASES:
        case = RC.EXTRA_CASES[cid][0]
        EV.add_world(cid, lambda: _build(RC.report_inputs(case), case, dev))
    return EV.world(cid, dev)


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    EV.close_worlds()


def arrays(res):
    return {k: res["report"][k] for k in KEYS if k in res["report"]}


def same(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == np.int64 and np.array_equal(a[k], b[k]) for k in a)


def hist2d(lab, pred, C):
    return np.bincount(np.asarray(lab, np.int64) * C + np.asarray(pred, np.int64), minlength=C * C).reshape(C, C)


def counts_of(p, multilabel, hp):
    pr, tr = np.asarray(p, F32) > F32(hp.f1_threshold), np.asarray(multilabel, F32) > 0.5
    return np.stack([(pr & tr).sum(0), pr.sum(0), tr.sum(0)], -1).astype(np.int64)


def raw_report(pop, tab, members=None, weights=None, combine=0, scratch=0, scores=None, confusion=None, rank_hist=None, label_counts=None):
    """mfas_population_evaluate_report as the C ABI takes it; returns (rc, message)."""
    mem = None if members is None else np.asarray(members, np.int32)
    wts = None if weights is None else np.asarray(weights, np.float32)
    tc = tab.to_c()
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731
    rc = pop.lib.mfas_population_evaluate_report(pop._h, ctypes.byref(tc), 0, None if mem is None else mem.ctypes.data,
                                                 None if wts is None else wts.ctypes.data, pop.K if mem is None else len(mem), combine,
                                                 scratch, None, None, ptr(scores), None, ptr(confusion), ptr(rank_hist), ptr(label_counts))
    return rc, pop.lib.mfas_last_error().decode()


# ------------------------------------------------------------------------------------------------ 1: single-label
@pytest.mark.parametrize("cid", SINGLE)
def test_single_label_report_is_the_tally_of_the_engines_own_rows(dev, cid):
    w = world(cid, dev)
    hp, t, K = w["hp"], w["tab"], w["case"][4]
    lab, C = t["label"], hp.C
    for members, weights in EC.member_lists(K):
        idx = list(range(K)) if members is None else members
        for combine in (0, 1):
            tag = f"{cid} members {members} combine {combine}"
            res = EV.evaluate(w, members, weights, combine, report=True)
            rep, preds = arrays(res), res["preds"].cpu().numpy()
            assert sorted(rep) == ["confusion", "rank_hist"] and rep["confusion"].shape == (len(idx) + 1, C, C), tag
            for s in range(len(idx)):       # the decisions the same call returned
                assert np.array_equal(rep["confusion"][s], hist2d(lab, preds[s], C)), f"{tag}: slot {s} against member_preds"
            zs = EC.member_scores(w["Z"][idx], hp, t.get("vlogit"), t.get("slogit"))
            RC.check_report(rep, zs, res["scores"].cpu().numpy(), lab, hp, tag)
            tr = np.trace(rep["confusion"], axis1=1, axis2=2)
            assert tr[:-1].tolist() == res["member_stats"]["dev_corrects"].tolist() and int(tr[-1]) == res["ensemble"]["corrects"], tag
            if len(idx) == 4:               # [1, 3, 1, 0]
                assert np.array_equal(rep["confusion"][0], rep["confusion"][2]) and np.array_equal(rep["rank_hist"][0], rep["rank_hist"][2])
            m = res["report"]
            assert m["topk"][1].tolist() == tr.tolist() and (m["topk"][5] >= m["topk"][1]).all() and m["per_class_accuracy"].shape == (len(idx) + 1, C)


# ------------------------------------------------------------------------------------------------ 2: multi-label
def test_multi_label_report(dev):
    w = world("c23_lm1", dev)
    hp, t, K = w["hp"], w["tab"], w["case"][4]
    z = t["multilabel"]
    single, P = [], []
    for k in range(K):      # one member of weight 1: k_vote's scores are that member's float32 sigmoid exactly
        res = EV.evaluate(w, [k], None, 0, report=True)
        lc, sc = arrays(res)["label_counts"], res["scores"].cpu().numpy()
        assert lc.shape == (2, hp.C, 3) and np.array_equal(lc[0], lc[1]) and np.array_equal(lc[0], counts_of(sc, z, hp)), k
        single.append(lc[0])
        P.append(sc)
    single, P = np.stack(single), np.stack(P)
    for members, weights in EC.member_lists(K):
        idx = list(range(K)) if members is None else members
        for combine in (0, 1):
            tag = f"c23_lm1 members {members} combine {combine}"
            res = EV.evaluate(w, members, weights, combine, report=True)
            rep = arrays(res)
            assert sorted(rep) == ["label_counts"] and np.array_equal(rep["label_counts"][:-1], single[idx]), tag
            RC.check_report(rep, P[idx], res["scores"].cpu().numpy(), z, hp, tag)
            m = res["report"]
            assert all(m[k].shape == (len(idx) + 1,) for k in ("f1_micro", "f1_macro", "f1_weighted")) and m["f1"].shape == (len(idx) + 1, hp.C)
    # independent of the engine's scores: the float64 sigmoid of the engine's logits decides every element outside its bound
    opened, pred = RC.open_elements(np.asarray(w["Z"], F64), hp, t)
    assert opened.mean() <= EC.MAX_AMBIGUOUS_FRACTION, opened.mean()
    lo, hi = RC.count_window(opened, pred, z)
    assert ((lo <= single) & (single <= hi)).all(), np.argwhere((lo > single) | (single > hi))[:4].tolist()


# ------------------------------------------------------------------------------------------------ 3: invariances
@pytest.mark.parametrize("cid", ["c60_bf16", "c23_lm1"])
def test_report_is_invariant_and_leaves_every_other_output_alone(dev, cid):
    torch = G._torch()
    w = world(cid, dev)
    hp, K, C, n = w["hp"], w["case"][4], w["hp"].C, w["case"][5]
    for members, weights in EC.member_lists(K)[2:]:
        M = K if members is None else len(members)
        for combine in (0, 1):
            tag = f"{cid} members {members} combine {combine}"
            plain = EV.evaluate(w, members, weights, combine)
            res = EV.evaluate(w, members, weights, combine, report=True)
            base = arrays(res)
            assert "report" not in plain and EV.outputs(res) == EV.outputs(plain), tag
            assert same(arrays(EV.evaluate(w, members, weights, combine, report=True)), base), tag
            for rows in (1, 40, 64):        # 64: N = 150 walks as 64 + 64 + 22 rows
                r2 = EV.evaluate(w, members, weights, combine, report=True, scratch_bytes=rows * M * C * 4)
                assert same(arrays(r2), base) and EV.outputs(r2) == EV.outputs(plain), (tag, rows)
            # without the caller's scores the ensemble's rows live in the arena
            r3 = w["pop"].evaluate(w["gtab"], members=members, weights=weights, combine=EV.COMBINE[combine], report=True)
            assert same(arrays(r3), base) and "scores" not in r3, tag
            assert r3["ensemble"] == plain["ensemble"] and r3["member_stats"].tobytes() == plain["member_stats"].tobytes(), tag
            # each array alone, through the C ABI
            for k in base:
                buf = torch.full(base[k].shape, -7, dtype=torch.int64, device=dev)
                rc, err = raw_report(w["pop"], w["gtab"], members, weights, combine, **{k: buf})
                assert rc == 0, err
                assert np.array_equal(buf.cpu().numpy(), base[k]), (tag, k)
            assert EV.outputs(EV.evaluate(w, members, weights, combine)) == EV.outputs(plain), tag
    assert n == 150 or cid != "c60_bf16"


# ------------------------------------------------------------------------------------------------ 4: NaN rows
def test_nan_rows(dev):
    case = EC.EVAL_CASES[EC.EVAL_IDS.index("c60_bf16")]
    inp = EC.eval_inputs(case)
    inp["p0s"][1]["central_classifier.bias"][0] = F32(np.nan)
    inp["p0s"][3]["central_classifier.bias"][3] = F32(np.nan)
    w = _build(inp, case, dev)
    try:
        hp, t, C = w["hp"], w["tab"], w["hp"].C
        lab = t["label"]
        assert np.isnan(w["Z"][1][:, 0]).all() and np.isnan(w["Z"][3][:, 3]).all() and not np.isnan(w["Z"][[0, 2, 4, 5, 6]]).any()
        for members in ([1, 3, 0], [0, 2, 3], None):
            idx = list(range(w["pop"].K)) if members is None else members
            for combine in (0, 1):
                tag = f"nan members {members} combine {combine}"
                res = EV.evaluate(w, members, None, combine, report=True)
                rep, preds = arrays(res), res["preds"].cpu().numpy()
                for s in range(len(idx)):
                    assert np.array_equal(rep["confusion"][s], hist2d(lab, preds[s], C)), f"{tag}: slot {s} against member_preds"
                RC.check_report(rep, w["Z"][idx], res["scores"].cpu().numpy(), lab, hp, tag, nan_free=False)
                if 1 in idx:            # a NaN in class 0 decides class 0 on every row and ranks last
                    s = idx.index(1)
                    assert rep["confusion"][s][:, 1:].sum() == 0 and rep["rank_hist"][s][C - 1] == (lab == 0).sum(), tag
                s = idx.index(3)        # a NaN in class 3 is never decided, and ranks last where it is the label
                assert rep["confusion"][s][:, 3].sum() == 0 and rep["rank_hist"][s][C - 1] == (lab == 3).sum(), tag
    finally:
        w["pop"].close()


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_new_refusals_name_the_argument_and_change_nothing(dev):
    torch = G._torch()
    for cid, key, msg in (("c60_bf16", "label_counts", "label_counts with loss_mode 0"), ("c23_lm1", "confusion", "confusion with loss_mode 1"),
                          ("c23_lm1", "rank_hist", "rank_hist with loss_mode 1")):
        w = world(cid, dev)
        C, K = w["hp"].C, w["case"][4]
        before = EV.outputs(EV.evaluate(w, None, None, 0))
        rep_before = arrays(EV.evaluate(w, None, None, 0, report=True))
        good = {"c60_bf16": "confusion", "c23_lm1": "label_counts"}[cid]        # an array the call would accept, given as well
        bufs = {k: torch.full((K + 1, C, {"confusion": C, "rank_hist": 1, "label_counts": 3}[k]), -7, dtype=torch.int64, device=dev)
                for k in (key, good)}
        rc, err = raw_report(w["pop"], w["gtab"], **bufs)
        assert rc == -1 and msg in err, (rc, err)
        assert all((b == -7).all().item() for b in bufs.values()), "a refused call wrote to an array"
        assert EV.outputs(EV.evaluate(w, None, None, 0)) == before
        assert same(arrays(EV.evaluate(w, None, None, 0, report=True)), rep_before)
    w = world("c60_bf16", dev)      # an existing refusal through the new entry: nothing is cleared either
    buf = torch.full((3, 60, 60), -7, dtype=torch.int64, device=dev)
    rc, err = raw_report(w["pop"], w["gtab"], members=[0, 99], confusion=buf)
    assert rc == -1 and "member 1 is candidate 99" in err and (buf == -7).all().item()


# ------------------------------------------------------------------------------------------------ the command line
def test_main_found_ntu_ensemble_report(dev, capsys):
    import re
    import main_found_ntu
    member, ens = main_found_ntu.main(["--synthetic", "64", "32", "48", "--ensemble", "0", "1", "--no-multitask", "--no-verbose", "--report",
                                       "--inner_representation_size", "16", "--epochs", "1", "--batchsize", "16"])
    out = capsys.readouterr().out
    got = {m.group(1): (float(m.group(2)), float(m.group(3)))
           for m in re.finditer(r"^(Member \d \(candidate \d\)|Ensemble) top-1: (\d\.\d{4}) top-5: (\d\.\d{4}) worst classes: \d+ \(", out, re.M)}
    assert sorted(got) == ["Ensemble", "Member 0 (candidate 0)", "Member 1 (candidate 1)"], out
    for name, acc in (("Member 0 (candidate 0)", member[0]), ("Member 1 (candidate 1)", member[1]), ("Ensemble", ens)):
        assert abs(got[name][0] - float(acc)) <= 0.50001e-4 and got[name][0] <= got[name][1] <= 1.0, (name, got[name], float(acc))
    assert "Conf 0 test accuracy" in out and "Ensemble test accuracy" in out        # what the run prints without the flag is still there
