"""CPU checks behind tests/test_gpu_report_ref64.py, before any GPU result is judged by it:

* calibration: with oracle-trained parameters the float32 oracle's dev logits stay under a quarter of TAU_LOGITS against ref64 on
  every REPORT_CASES shape;
* the conditions that keep the comparison from hiding a failure (pairwise disjoint loss intervals, the ambiguity cap, the
  multi-label count windows) hold for the reference alone;
* five mutations of the per-candidate report (a restatement of k_eval's 1-D grid map) fail check_dev on some candidate;
* every dev-pass build the library's choice (builds.hip.h: eval_key, compiled by tests/builds_header.py) can reach is named by a
  case, the others are listed with the reason;
* the host bookkeeping (best_dev_accuracy, best_dev_f1) against a restatement of the reference's loops, and the best-epoch rule.
"""
import functools

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import builds_header as BH
from tests import ref64 as R64
from tests import gpu_support as G
from tests import report_cases as RP

F32 = np.float32


@functools.lru_cache(maxsize=None)
def trained(cid):
    """A case's inputs and the float32 oracle's parameters of every candidate after each epoch (computed once per case)."""
    case = RP.REPORT_CASES[RP.REPORT_IDS.index(cid)]
    inp = RP.report_inputs(case)
    states = [RP.oracle_epochs(c, inp["hp"], inp["p0s"][k], inp["ttr"], inp["seeds"][k], inp["etas"], RP.E_REPORT)[0]
              for k, c in enumerate(inp["confs"])]
    return inp, states


# ------------------------------------------------------------------------------------------------ calibration and conditions
@pytest.mark.parametrize("cid", RP.REPORT_IDS)
def test_report_cases_calibration_and_conditions(cid):
    inp, states = trained(cid)
    hp, f = inp["hp"], G.feats_of(inp["tdv"])
    for e in range(RP.E_REPORT):
        refs = []
        for k, conf in enumerate(inp["confs"]):
            P = states[k][e]
            lg, Ml, _ = R64.forward(P, conf, hp, f, False)
            lg32, _ = O.forward({key: v.copy() for key, v in P.items()}, conf, hp, f, False)
            r = R64.worst_ratio(lg32, lg, Ml)[0]
            assert r * 4.0 <= G.TAU_LOGITS, (cid, e, k, r)
            refs.append(RP.dev_ref(P, conf, hp, inp["tdv"]))
        RP.check_conditions(refs, hp, RP.N_DEV, f"{cid} epoch {e}", margin=2.0, spare=1)


# ------------------------------------------------------------------------------------------------ mutations of the report
def grid_map(wg, nblk, ncand, groups_of=8):
    """k_eval's B3 grid map (eval.hip.h): workgroup -> (candidate, tile).  Full groups of eight candidates are interleaved tile by
    tile, the candidates behind the last full group keep the plain order.  groups_of: the mutation that computes the candidate of
    an interleaved workgroup with another modulus."""
    per8 = 8 * nblk
    grp, r = divmod(wg, per8)
    if grp < ncand // 8:
        if groups_of == 8:
            return grp * 8 + (r & 7), r >> 3
        return grp * 8 + r % groups_of, r // groups_of
    rem = wg - (ncand // 8) * per8
    return (ncand // 8) * 8 + rem // nblk, rem % nblk


def simulated_report(tiles, K, nblk, mutation=None):
    """The statistics [K][E] a dev pass writes, from the float32 oracle's per-tile sums tiles[e][k][tile] = (loss, count), through
    the grid map; mutation: None or one of MUTATIONS."""
    E = len(tiles)
    out = np.zeros((K, E), dtype=[("train_loss_sum", "f8"), ("dev_loss_sum", "f8"), ("train_corrects", "i8"), ("dev_corrects", "i8")])
    for e in range(E):
        for wg in range(nblk * K):
            k, tile = grid_map(wg, nblk, K, groups_of=nblk if mutation == "nblk_for_8" else 8)
            if tile >= nblk or k >= K:
                continue                                  # (a tile past the table has no valid row)
            if mutation == "ragged_tile_dropped" and tile == nblk - 1:
                continue
            if mutation == "tile1_twice" and tile == 2:
                tile = 1
            slot = e ^ 1 if mutation == "epoch_slot" else e
            loss, count = tiles[e][k][tile]
            out["dev_loss_sum"][k, slot] += loss
            out["dev_corrects"][k, slot] += count
    if mutation == "swap_8_9":
        out[[8, 9]] = out[[9, 8]]
    return out


MUTATIONS = ("swap_8_9", "nblk_for_8", "ragged_tile_dropped", "tile1_twice", "epoch_slot")
MUTATION_CASE = "b3_k11"       # one interleaved group of eight and a remainder of three; three 64-row tiles


@functools.lru_cache(maxsize=None)
def oracle_tiles():
    inp, states = trained(MUTATION_CASE)
    hp = inp["hp"]
    me = G.eval_me(hp)
    nblk = -(-RP.N_DEV // me)
    tiles = []
    for e in range(RP.E_REPORT):
        per = []
        for k, conf in enumerate(inp["confs"]):
            row = []
            for t0 in range(0, RP.N_DEV, me):
                sl = slice(t0, min(t0 + me, RP.N_DEV))
                f = {key: v[sl] for key, v in G.feats_of(inp["tdv"]).items()}
                lg, _ = O.forward({key: v.copy() for key, v in states[k][e].items()}, conf, hp, f, False)
                loss, _, preds = O.ce_loss(lg, inp["tdv"]["label"][sl])
                row.append((float(loss) * (sl.stop - sl.start), int((preds == inp["tdv"]["label"][sl]).sum())))
            per.append(row)
        tiles.append(per)
    return tiles, nblk


def failing_candidates(report):
    inp, states = trained(MUTATION_CASE)
    bad = []
    for e in range(RP.E_REPORT):
        for k, conf in enumerate(inp["confs"]):
            try:
                G.check_dev(report[k:k + 1, e:e + 1], states[k][e], conf, inp["hp"], inp["tdv"], "mutation")
            except AssertionError:
                bad.append((k, e))
    return bad


def test_unmutated_report_passes():
    tiles, nblk = oracle_tiles()
    assert nblk == 3
    K = len(tiles[0])
    seen = sorted(grid_map(wg, nblk, K) for wg in range(nblk * K))
    assert seen == [(k, t) for k in range(K) for t in range(nblk)]           # the map is a bijection onto (candidate, tile)
    keep = dict(R64.RATIOS)
    try:
        assert failing_candidates(simulated_report(tiles, K, nblk)) == []
    finally:
        R64.RATIOS.clear()
        R64.RATIOS.update(keep)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_report_mutation_fails_check_dev(mutation):
    tiles, nblk = oracle_tiles()
    keep = dict(R64.RATIOS)
    try:
        bad = failing_candidates(simulated_report(tiles, len(tiles[0]), nblk, mutation))
    finally:
        R64.RATIOS.clear()
        R64.RATIOS.update(keep)
    assert bad, mutation
    if mutation == "swap_8_9":
        assert {k for k, _ in bad} == {8, 9}, bad


# ------------------------------------------------------------------------------------------------ coverage of the builds
def eval_choice(facts_and_dtypes):
    """builds.hip.h's eval_key with no switch set, for (eval facts, table dtype) pairs: the names of the builds."""
    return BH.ask([("eval", BH.facts(**f), BH.DTYPE[dtype], 0, 0, 0) for f, dtype in facts_and_dtypes])


def test_every_reachable_dev_pass_build_is_named_by_a_case():
    geometries = set()
    for R in range(1, 513):
        for C in range(1, 257, 5):
            geometries.add(tuple(sorted(G.eval_facts(O.Hyper(R=R, C=C, B=16, s_sizes=G.W_A["s"], v_sizes=G.W_A["v"])).items())))
    reachable = set(eval_choice([(dict(f), dtype) for f in sorted(geometries) for dtype in G.DTYPES]))
    hp = O.Hyper(R=512, C=256, B=16, s_sizes=G.W_A["s"], v_sizes=G.W_A["v"])
    assert G.eval_me(hp) == 16
    all_builds = {G.eval_name(b) for b in RP.ALL_BUILDS}
    named = {G.eval_name(c[7]) for c in RP.REPORT_CASES}
    assert reachable == named, (sorted(reachable - named), sorted(named - reachable))
    assert all_builds == reachable, (sorted(all_builds - reachable), sorted(reachable - all_builds))
    assert len(all_builds) == len(RP.ALL_BUILDS) == 14
    assert all_builds == {k for k in BH.ask1("tables", None) if k.startswith("k_eval<")}          # the library's table
    cases = eval_choice([(G.eval_facts(RP.report_hyper(case)), case[4]) for case in RP.REPORT_CASES])
    for case, name in zip(RP.REPORT_CASES, cases):
        assert name == G.eval_name(case[7]), (case[0], name)
    # the branches of the 1-D grid: a full group with a remainder, full groups only, a remainder of one
    b3 = {c[0]: c[5] for c in RP.REPORT_CASES if c[7][4]}
    assert b3["b3_k11"] == 11 and b3["b3_k16_mt"] == 16 and b3["b3_r72_k9"] == 9 and all(K >= 9 for K in b3.values())
    assert all(c[5] >= 9 for c in RP.REPORT_CASES)
    assert sum("lm1" in c[6] for c in RP.REPORT_CASES if c[7][4]) >= 1 and sum("lm1" in c[6] for c in RP.REPORT_CASES if c[1] <= 32) >= 1


# ------------------------------------------------------------------------------------------------ host bookkeeping
def _stats(train_loss, dev_corrects):
    s = np.zeros(len(train_loss), dtype=[("train_loss_sum", "f8"), ("dev_loss_sum", "f8"), ("train_corrects", "i8"), ("dev_corrects", "i8")])
    s["train_loss_sum"], s["dev_corrects"] = train_loss, dev_corrects
    return s


def ref_track_acc(corrects, n_dev):
    """train_searchable/ntu.py:18,82-83: best_acc = 0; per epoch, if epoch_acc > best_acc: best_acc = epoch_acc."""
    best = 0.0
    for c in corrects:
        acc = float(c) / float(n_dev)
        if acc > best:
            best = acc
    return best


def ref_track_f1(train_loss, f1s, init_f1):
    """train_searchable/mmimdb.py:18-137: best_f1 = init_f1; per epoch, a NaN train loss ends the run before the dev phase counts;
    if epoch f1 > best_f1: best_f1 = f1; at the end a NaN best becomes 0."""
    best = init_f1
    for loss, f1 in zip(train_loss, f1s):
        if not np.isfinite(loss):
            break
        if f1 > best:
            best = f1
    return 0.0 if best != best else best


def test_best_dev_accuracy_matches_the_reference_loop():
    from mfas_amd import best_dev_accuracy
    rng = np.random.default_rng(4)
    for _ in range(200):
        c = rng.integers(0, 49, size=rng.integers(1, 7))
        assert best_dev_accuracy(_stats(np.ones(len(c)), c), 48) == ref_track_acc(c, 48)
    assert best_dev_accuracy(_stats([1.0, 1.0], [0, 0]), 48) == 0.0                 # starts at 0
    assert best_dev_accuracy(_stats([1.0, 1.0, 1.0], [7, 30, 30]), 48) == 30 / 48   # strict >: a tie changes nothing


def test_best_dev_f1_matches_the_reference_loop():
    from mfas_amd.engine import F1_FIXED_POINT, best_dev_f1
    n = 40
    rng = np.random.default_rng(5)
    for _ in range(300):
        E = int(rng.integers(1, 7))
        fx = rng.integers(0, n << 32, size=E)
        loss = rng.random(E) + 0.1
        if rng.random() < 0.6:
            loss[rng.integers(E)] = [np.nan, np.inf, -np.inf][rng.integers(3)]
        init = float(rng.choice([0.0, 0.25, 0.9]))
        f1s = [float(x) / F1_FIXED_POINT / n for x in fx]
        flagged = not np.isfinite(loss).all()
        assert best_dev_f1(_stats(loss, fx), flagged, n, init) == ref_track_f1(loss, f1s, init)
        # without the flag the scan never stops: every epoch counts
        assert best_dev_f1(_stats(loss, fx), False, n, init) == ref_track_f1(np.ones(E), f1s, init)
    one = 1 << 32
    assert best_dev_f1(_stats([1.0, 1.0], [10 * one, 10 * one]), False, n, 0.25) == 0.25          # strict > from init_f1
    assert best_dev_f1(_stats([1.0, 1.0], [10 * one + 1, 10 * one + 1]), False, n, 0.25) == (10 * one + 1) / F1_FIXED_POINT / n
    assert best_dev_f1(_stats([1.0, np.nan, 1.0], [one, 30 * one, 35 * one]), True, n) == 1 / n   # stops at the first non-finite loss
    assert best_dev_f1(_stats([1.0, np.nan, 1.0], [one, 30 * one, 35 * one]), False, n) == 35 / n  # ... and only when flagged
    assert best_dev_f1(_stats([1.0], [one]), False, n, float("nan")) == 0.0                        # a NaN best becomes 0


# ------------------------------------------------------------------------------------------------ the saturation control
@pytest.mark.parametrize("name", RP.STATUS_LM1)
def test_control_bias_calibration_margin(name):
    """On every multi-label status schedule's inputs: with POISON_BIAS the reference's formula in float32 gives a non-finite loss on
    the first batch; with CONTROL_BIAS the logits stay below 16 and the float32 loss uses under a quarter of ref64's bound."""
    inp = RP.status_inputs(name, True)
    hp = inp["hp"]
    assert not np.isfinite(RP.first_batch_loss32(inp, 1, RP.poisoned(inp["p0s"][1], RP.POISON_BIAS))[0])
    p1 = RP.poisoned(inp["p0s"][1], RP.CONTROL_BIAS)
    loss32, top = RP.first_batch_loss32(inp, 1, p1)
    assert np.isfinite(loss32) and top < 16.0, (loss32, top)
    zero = {key: np.zeros_like(v) for key, v in p1.items()}
    batch = {key: v[:hp.B] for key, v in inp["ttr"].items()}
    exp = R64.train_step64({"w": p1, "m": zero, "v": zero}, inp["confs"][1], hp, batch, inp["seeds"][1], 0, inp["etas"][0], 1,
                           G.TAU_LOGITS, RP.GT.TAU_V, pos_weight=G.pos_weight(hp))
    ref, lb = exp["loss"]
    assert abs(loss32 * len(batch["label"]) - ref) * 4.0 <= lb, (name, loss32 * len(batch["label"]), ref, lb)


# ------------------------------------------------------------------------------------------------ the best-epoch rule
def test_best_epoch_rule():
    rule = RP.best_epoch_rule
    assert rule([0.2, 0.5, 0.5, 0.4], 0.0) == (1, 0.5)        # a tie keeps the earlier epoch
    assert rule([0.2, 0.1, 0.3], 0.0) == (2, 0.3)
    assert rule([0.2, 0.1, 0.2], 0.0) == (0, 0.2)
    assert rule([0.2, 0.1, 0.2], 0.2) == (-1, 0.2)            # strict >: the threshold itself is not exceeded
    assert rule([0.0, 0.0], 0.0) == (-1, 0.0)
    assert rule([0.1, 0.3], 0.25) == (1, 0.3)
    assert rule([], 0.5) == (-1, 0.5)


def test_best_epoch_rule_names_what_the_oracle_restores():
    """The float32 oracle with restore_best (train_searchable/ntu.py:17,82-86) leaves the parameters of the epoch the rule names."""
    hp = O.Hyper(R=16, C=60, B=20, bn=True, drpt=0.5, s_sizes=G.W_A["s"], v_sizes=G.W_A["v"], epochs=4)
    tup = ("rule", 16, 60, 20, G.W_A, None, True, 0.5, "")
    ttr, tdv = G.case_table(tup, hp, 43, 161, "bfloat16"), G.case_table(tup, hp, 30, 162, "bfloat16")
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, 43 / 20, 4 * 3)
    seen = set()
    for k, cells in enumerate(RP.GT.SCHED_CONFS):
        conf = np.array(cells)
        p0 = O.init_params(conf, hp, 140 + k, perturb_bn=True)
        states, _ = RP.oracle_epochs(conf, hp, p0, ttr, 11 + k, etas, 4)
        hist, params = [], {key: v.copy() for key, v in p0.items()}
        best = O.train_candidate(conf, hp, params, ttr, tdv, seed=11 + k, etas=etas, history=hist, restore_best=True)
        ep, metric = RP.best_epoch_rule([h["dev_acc"] for h in hist], 0.0)
        want = p0 if ep < 0 else states[ep]
        assert metric == best and all(np.array_equal(params[key], want[key]) for key in want), (k, ep, [h["dev_acc"] for h in hist])
        seen.add(ep)
    assert len(seen) >= 2, seen         # (the candidates do not all keep the same epoch)
