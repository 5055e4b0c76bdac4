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

from tests.evaluate_cases import (EVAL_CASES, EVAL_IDS, F32, ROOT, TAU_VOTE, check_conditions, check_members, check_vote, eval_inputs,
                                  member_lists, member_scores, normalised, oracle_logits, table_columns, vote32, vote64)


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
