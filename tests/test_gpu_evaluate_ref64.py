"""Population.evaluate (mfas_population_evaluate: k_eval per member, then k_vote) on the GPU, against the float64 statement of the
vote in tests/test_evaluate_cpu.py (vote64, its error scale M_vote, TAU_VOTE = 4, the ambiguity rule) and against tests/ref64.py.

  1. members are the existing entry points, exactly (forward's count, the first maximum of forward's scores, the dev pass of train);
  2. the vote on exact inputs: the engine's own float32 logits through vote64;
  3. end to end against ref64 (two cases): ref64's logits with their bound TAU_LOGITS 2^-24 max_c Ml per row;
  4. invariances: run to run, scratch_bytes, M = 1, members=None, weights against a repeated member;
  5. plane 3 of an unfinished snapshot_best schedule;  6. no side effects on a schedule run in segments;  7. every refusal;
  8. main_found_ntu --ensemble.
EVAL_CASES (tests/test_evaluate_cpu.py) covers C in {2, 23, 60, 70, 256}, f32 / bf16 tables, R = 16 and one R = 128 bf16 case,
loss_mode 0 / multitask / loss_mode 1 with positive weights, N in {1, 37, 150}; every case runs M in {1, 3, K} and a list with a
repeated member, with both combines.

Observed on the MI355X (18 tests, 3 s; the table is printed with -s): the ensemble's probabilities use at most 0.092 of their bound
on the engine's own logits (c70_mt, mean of probabilities; 0.041 .. 0.092 over the cases, i.e. under 0.4 x 2^-24 M_vote), and 0.019 /
0.008 of the end-to-end bound (c60_bf16 / c23_lm1).

Run on its own, with a time limit:  python -m pytest tests/test_gpu_evaluate_ref64.py -m gpu -x -q -s
"""
import ctypes

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import evaluate_cases as EC
from tests import gpu_support as G
from tests.gpu_support import dev  # noqa: F401
from tests.report_gpu import make_population, plane_bytes
from tests.evaluate_gpu import COMBINE, close_worlds, evaluate, outputs, world

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
U = R64.U


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    close_worlds()


def statement(w, members, weights, combine, Z=None, dz=None):
    hp, t = w["hp"], w["tab"]
    Z = w["Z"] if Z is None else Z
    Z = Z if members is None else Z[members]
    zs = EC.member_scores(Z, hp, t.get("vlogit"), t.get("slogit")) if dz is None else Z
    return EC.vote64(zs, EC.normalised(weights, len(Z)), hp, combine, EC.TAU_VOTE, dz=dz, **EC.table_columns(t, hp)), zs


# ------------------------------------------------------------------------------------------------ 1, 2 and part of 4
@pytest.mark.parametrize("cid", EC.EVAL_IDS)
def test_members_are_forward_and_the_vote_meets_its_statement(dev, cid):
    w = world(cid, dev)
    hp, K, n = w["hp"], w["case"][4], w["case"][5]
    for members, weights in EC.member_lists(K):
        idx = list(range(K)) if members is None else members
        for combine in (0, 1):
            tag = f"{cid} members {members} combine {combine}"
            res = evaluate(w, members, weights, combine)
            # 1. members: the count forward() reports, the first maximum of forward()'s float32 scores
            assert res["member_stats"]["dev_corrects"].tolist() == [w["counts"][k] for k in idx], tag
            assert not res["member_stats"]["train_loss_sum"].any() and not res["member_stats"]["train_corrects"].any()
            ref, zs = statement(w, members, weights, combine)
            if hp.loss_mode == 0:
                EC.check_members(zs, res["preds"].cpu().numpy(), tag)
            # 2. the vote on the engine's own logits
            EC.check_conditions(ref, zs, hp, tag)
            EC.check_vote(ref, res["scores"].cpu().numpy(), res["ensemble"]["corrects"], res["ensemble"]["loss_sum"], tag,
                          record=f"vote (fraction of tau)/{cid}/{COMBINE[combine]}")
            if len(idx) == 1:       # 4. one member: the ensemble decides what the member decides
                assert res["ensemble"]["corrects"] == int(res["member_stats"]["dev_corrects"][0]), tag
            if members is None:     # 4. None is 0 .. K-1
                assert outputs(res) == outputs(evaluate(w, list(range(K)), None, combine)), tag
            if hp.loss_mode == 1 and combine == 0:
                assert res["ensemble"]["loss_sum"] == 0.0
    assert n == len(w["tab"]["label"])


# ------------------------------------------------------------------------------------------------ 1: the dev pass of train()
@pytest.mark.parametrize("cid", ["c60_bf16", "c23_lm1", "r128_bf16"])
def test_member_stats_are_the_dev_pass_numbers(dev, cid):
    """After train(epochs=1) with the same table as dev, every member's statistics are that epoch's: the count exactly, the loss
    within N 2^-53 relative (a double atomic sum of the same float tile sums, in another order)."""
    from tests.helpers import engine_hyper
    case = EC.EVAL_CASES[EC.EVAL_IDS.index(cid)]
    inp = EC.eval_inputs(case)
    hp, K, n = inp["hp"], case[4], case[5]
    ntr = 2 * hp.B + 3
    ttr = G.case_table((cid, case[1], case[2], hp.B, G.W_A, None, True, 0.5, case[6]), hp, ntr, 9090, inp["dtype"])
    pop = make_population(engine_hyper(hp), inp["confs"], dev, inp["seeds"], pos_weight=G.pos_weight(hp) if hp.loss_mode else None)
    try:
        for k, p in enumerate(inp["p0s"]):
            pop.set_state_dict(k, p)
        tdv = G.gpu_table(inp["tab"], inp["dtype"], dev)
        stats, status = pop.train(G.gpu_table(ttr, inp["dtype"], dev), tdv, 1, O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, -(-ntr // hp.B)))
        assert not status.any()
        res = pop.evaluate(tdv)
    finally:
        pop.close()
    assert res["member_stats"]["dev_corrects"].tolist() == stats["dev_corrects"][:, 0].tolist()
    want, got = stats["dev_loss_sum"][:, 0], res["member_stats"]["dev_loss_sum"]
    assert (np.abs(got - want) <= n * 2.0 ** -53 * np.abs(want)).all(), (got, want)
    assert (want != 0).all()


# ------------------------------------------------------------------------------------------------ 3: end to end
@pytest.mark.parametrize("cid,members,combine", [("c60_bf16", None, 0), ("c23_lm1", [5, 0, 2], 1)])
def test_end_to_end_against_ref64(dev, cid, members, combine):
    """ref64's eval-mode logits and Ml: a member's row is known to delta_m = TAU_LOGITS 2^-24 max_c Ml, which moves its softmax (or
    sigmoid) by at most p (exp(2 delta_m) - 1); that joins the allowance of statement 2.  Decisions through the ambiguity rule."""
    w = world(cid, dev)
    hp, f = w["hp"], G.feats_of(w["tab"])
    lg, dz = [], []
    for p, c in zip(w["p0s"], w["confs"]):
        l, Ml, _ = R64.forward(p, c, hp, f, False)
        lg.append(l)
        dz.append(G.TAU_LOGITS * U * Ml.max(1))
    ref, zs = statement(w, members, None, combine, Z=np.stack(lg), dz=np.stack(dz) if members is None else np.stack(dz)[members])
    EC.check_conditions(ref, zs, hp, f"{cid} end to end")
    res = evaluate(w, members, None, combine)
    EC.check_vote(ref, res["scores"].cpu().numpy(), res["ensemble"]["corrects"], res["ensemble"]["loss_sum"], f"{cid} end to end",
                  record=f"vote end to end (fraction of the bound)/{cid}")


# ------------------------------------------------------------------------------------------------ 4: invariances
def test_bit_identical_across_runs_and_scratch_sizes(dev):
    w = world("c60_bf16", dev)
    K, C = w["case"][4], w["hp"].C
    for members, weights in EC.member_lists(K)[2:]:
        M = K if members is None else len(members)
        for combine in (0, 1):
            base = outputs(evaluate(w, members, weights, combine))
            assert outputs(evaluate(w, members, weights, combine)) == base
            for rows in (1, 40):        # one row per block; 40 rows: four blocks of 150, the last ragged
                assert outputs(evaluate(w, members, weights, combine, scratch_bytes=rows * M * C * 4)) == base, (members, combine, rows)


def test_weights_equal_a_repeated_member_within_the_allowance(dev):
    w = world("c60_bf16", dev)
    for combine in (0, 1):
        a = evaluate(w, [4, 1, 5], [2.0, 1.0, 1.0], combine)["scores"].cpu().numpy().astype(F64)
        b = evaluate(w, [4, 4, 1, 5], None, combine)["scores"].cpu().numpy().astype(F64)
        ra, _ = statement(w, [4, 1, 5], [2.0, 1.0, 1.0], combine)
        rb, _ = statement(w, [4, 4, 1, 5], None, combine)
        assert (np.abs(a - b) <= ra["bound"] + rb["bound"]).all()


# ------------------------------------------------------------------------------------------------ 5, 6: plane 3, no side effects
def _segment_inputs(dev, K=5):
    from tests.helpers import engine_hyper
    hp = O.Hyper(R=16, C=60, B=16, bn=True, drpt=0.5, s_sizes=G.W_A["s"], v_sizes=G.W_A["v"], epochs=3)
    rng = np.random.default_rng(77)
    confs = [np.array([[rng.integers(4), rng.integers(4), rng.integers(3)] for _ in range(1 + k % 2)]) for k in range(K)]
    tup = ("seg", 16, 60, 16, G.W_A, None, True, 0.5, "")
    ntr = 2 * hp.B + 3
    return dict(hp=hp, ehp=engine_hyper(hp), confs=confs, seeds=[31 + k for k in range(K)],
                p0s=[O.init_params(c, hp, 500 + k, perturb_bn=True) for k, c in enumerate(confs)],
                ttr=G.gpu_table(G.case_table(tup, hp, ntr, 601, "bfloat16"), "bfloat16", dev),
                tdv=G.gpu_table(G.case_table(tup, hp, 37, 602, "bfloat16"), "bfloat16", dev),
                etas=O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, 3 * -(-ntr // hp.B)))


def _fresh(inp, dev):
    pop = make_population(inp["ehp"], inp["confs"], dev, inp["seeds"])
    for k, p in enumerate(inp["p0s"]):
        pop.set_state_dict(k, p)
    return pop


def test_plane_3_is_the_kept_best_of_an_unfinished_schedule(dev):
    inp = _segment_inputs(dev)
    K = len(inp["confs"])
    pop, other = _fresh(inp, dev), _fresh(inp, dev)
    try:
        with pytest.raises(RuntimeError, match=r"plane 3: candidate 0 keeps no best-epoch parameters"):
            pop.evaluate(inp["tdv"], plane=3)
        pop.train(inp["ttr"], inp["tdv"], 3, inp["etas"], snapshot_best=True, first_epoch=0, last_epoch=2)
        for k in range(K):
            other.set_params(k, pop.get_params(k, 3))
        for combine in COMBINE:
            a = pop.evaluate(inp["tdv"], plane=3, combine=combine, return_scores=True, return_preds=True)
            b = other.evaluate(inp["tdv"], plane=0, combine=combine, return_scores=True, return_preds=True)
            assert outputs(a) == outputs(b)
            assert np.allclose(a["member_stats"]["dev_loss_sum"], b["member_stats"]["dev_loss_sum"], rtol=37 * 2.0 ** -53, atol=0)
    finally:
        pop.close()
        other.close()


def test_no_side_effects_between_two_segments(dev):
    inp = _segment_inputs(dev)
    K = len(inp["confs"])
    runs = []
    for with_eval in (True, False):
        pop = _fresh(inp, dev)
        try:
            s1, _ = pop.train(inp["ttr"], inp["tdv"], 3, inp["etas"], snapshot_best=True, first_epoch=0, last_epoch=2)
            if with_eval:
                rec = pop.launch_record()
                prog = [pop.get_progress(k) for k in range(K)]
                for plane in (0, 3):
                    pop.evaluate(inp["tdv"], members=[1, 0, 1], weights=[1, 2, 3], plane=plane, combine="score", scratch_bytes=3 * 60 * 4 * 5,
                                 return_scores=True, return_preds=True)
                assert pop.launch_record() == rec and rec
                assert [pop.get_progress(k) for k in range(K)] == prog
            s2, st2 = pop.train(inp["ttr"], inp["tdv"], 3, inp["etas"], snapshot_best=True, first_epoch=2, last_epoch=3)
            runs.append(dict(planes=[[plane_bytes(pop, k, pl) for pl in (0, 1, 2)] for k in range(K)], s1=s1.tobytes(), s2=s2.tobytes(),
                             status=st2.tolist(), prog=[pop.get_progress(k) for k in range(K)], rec=pop.launch_record()))
        finally:
            pop.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------ 7: refusals
def _raw_evaluate(pop, tab, plane=0, members=None, weights=None, M=None, combine=0, scratch=0, preds=None):
    """mfas_population_evaluate as the C ABI takes it (the Python face checks most arguments itself); returns (rc, message)."""
    from mfas_amd import _lib
    mem = None if members is None else np.asarray(members, np.int32)
    wts = None if weights is None else np.asarray(weights, np.float32)
    tc = tab if isinstance(tab, _lib.mfas_table) else tab.to_c()
    M = (pop.K if mem is None else len(mem)) if M is None else M
    rc = pop.lib.mfas_population_evaluate(pop._h, ctypes.byref(tc), plane, None if mem is None else mem.ctypes.data,
                                          None if wts is None else wts.ctypes.data, M, combine, scratch, None,
                                          None if preds is None else ctypes.c_void_p(preds.data_ptr()), None, None)
    return rc, pop.lib.mfas_last_error().decode()


def test_every_refusal_names_the_value_and_changes_nothing(dev):
    import re
    torch = G._torch()
    w = world("c60_bf16", dev)
    pop, tab, K = w["pop"], w["gtab"], w["case"][4]
    before = outputs(evaluate(w, None, None, 0))
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(members=[0, K]), rf"member 1 is candidate {K}, outside \[0, {K}\)"),
        (dict(members=[-1]), r"member 0 is candidate -1, outside"),
        (dict(members=[0], M=0), r"M = 0 members"),
        (dict(members=[0], M=-3), r"M = -3 members"),
        (dict(members=None, M=K - 1), rf"members == NULL means all {K} candidates, but M = {K - 1}"),
        (dict(members=[0, 1], weights=[1.0, -0.5]), r"weight 1 is -0.5"),
        (dict(members=[0, 1], weights=[nan, 1.0]), r"weight 0 is -?nan"),
        (dict(members=[0, 1], weights=[1.0, inf]), r"weight 1 is inf"),
        (dict(members=[0, 1], weights=[0.0, 0.0]), r"weights sum to 0"),
        (dict(plane=1), r"plane 1 \(0 = live parameters, 3 = kept best\)"),
        (dict(plane=3, members=[2]), r"plane 3: candidate 2 keeps no best-epoch parameters \(no snapshot_best schedule in progress\)"),
        (dict(combine=2), r"combine 2 \(0 = mean of probabilities, 1 = mean of scores\)"),
        (dict(members=[0, 1, 2], scratch=3 * 60 * 4 - 1), r"scratch_bytes 719 holds no row of 3 members' logits \(720 bytes\)"),
        (dict(scratch=-8), r"scratch_bytes -8 is negative"),
    ]
    for kw, msg in cases:
        rc, err = _raw_evaluate(pop, tab, **kw)
        assert rc == -1 and re.search(msg, err), (kw, rc, err)
    # table faults, as mfas_population_forward refuses them
    tc = tab.to_c()
    tc.label = None
    assert _raw_evaluate(pop, tc)[0] == -1 and "labels missing" in _raw_evaluate(pop, tc)[1]
    tc = tab.to_c()
    tc.N = 0
    assert _raw_evaluate(pop, tc)[0] == -1 and "null or empty" in _raw_evaluate(pop, tc)[1]
    tc = tab.to_c()
    tc.dtype = 7
    assert _raw_evaluate(pop, tc)[0] == -1 and "bad dtype" in _raw_evaluate(pop, tc)[1]
    mt = world("c70_mt", dev)
    tc = mt["gtab"].to_c()
    tc.vlogit = None
    assert _raw_evaluate(mt["pop"], tc)[0] == -1 and "multitask needs vlogit/slogit" in _raw_evaluate(mt["pop"], tc)[1]
    # member_preds with the multi-label head
    lm = world("c23_lm1", dev)
    preds = torch.empty((lm["pop"].K, len(lm["gtab"])), dtype=torch.int32, device=dev)
    rc, err = _raw_evaluate(lm["pop"], lm["gtab"], preds=preds)
    assert rc == -1 and "member_preds with loss_mode 1" in err, err
    # the Python face: its own checks, a table without a selected tap, a label outside [0, C)
    with pytest.raises(ValueError, match=r"member 9 is outside"):
        pop.evaluate(tab, members=[9])
    with pytest.raises(ValueError, match="return_preds with loss_mode 1"):
        lm["pop"].evaluate(lm["gtab"], return_preds=True)
    from mfas_amd.engine import FeatureTable
    true_taps = {k: v[:, :tab.widths[k]] for k, v in tab.taps.items()}
    short = FeatureTable({k: v for k, v in true_taps.items() if k != "s0"}, tab.label)
    if "s0" in pop._used_taps:
        with pytest.raises(ValueError, match="selects tap s0"):
            pop.evaluate(short)
    bad = FeatureTable(true_taps, torch.full_like(tab.label, 60))
    with pytest.raises(IndexError, match="Target 60 is out of bounds"):
        pop.evaluate(bad)
    assert outputs(evaluate(w, None, None, 0)) == before


# ------------------------------------------------------------------------------------------------ 8: the command line
def test_main_found_ntu_ensemble(dev, capsys):
    import main_found_ntu
    member, ens = main_found_ntu.main(["--synthetic", "64", "32", "48", "--ensemble", "0", "1", "--no-multitask", "--no-verbose",
                                       "--inner_representation_size", "16", "--epochs", "1", "--batchsize", "16"])
    assert member.shape == (2,) and all(0.0 <= float(a) <= 1.0 for a in member) and 0.0 <= float(ens) <= 1.0
    assert all(abs(float(a) * 48 - round(float(a) * 48)) < 1e-9 for a in list(member) + [ens])      # counts over the 48 test rows
    out = capsys.readouterr().out
    assert "Conf 0 test accuracy" in out and "Conf 1 test accuracy" in out and "Ensemble test accuracy" in out
    with pytest.raises(SystemExit):         # the search-mode train loop refuses multitask: argparse says so
        main_found_ntu.parse_args(["--ensemble", "0", "1"])
