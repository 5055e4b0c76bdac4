"""CPU side of the axis tests (tests/test_gpu_axes_ref64.py judges the kernels on the GPU): three axes of the C ABI that every
other ref64 file holds at one value.

* Tap slots.  MFAS_MAX_TAPS is 8 per modality; every other file has four S and four V widths and selects slots 0..3.  TAP_CASES
  (single candidates, the entry points) and TAP_POPS (every train schedule in both order modes, a wide population) use three
  width sets: W_8 (8 + 8 slots with unused ones between used ones), W_AV (AV-MNIST's 5 + 3) and W_26 (2 + 6).
* Plain cells.  allow_plain_cell with bn = 0 and drpt = 0: a cell is [Linear, nl].  PLAIN_POPS has one population per chain family.
* Hyper-parameter scalars.  wd, beta1, beta2, adam_eps, bn_eps, bn_momentum, f1_threshold and the learning rates, in four
  SCALAR_SETS whose every field is off its default: SCALAR_POPS (every train schedule, a wide population) and SCALAR_EVAL_CASES
  (the multi-label head's dev pass).  The fourth, 'sd', has eta_max = 3e-2; the train steps of its populations, and of no other,
  are judged with ref64's batch_sum_term (tests/ref64.py::forward), both of its terms.

Here: the covering designs; the schedules the layout query can name without a device; calibration — on exactly the inputs the GPU
file uses (shared by import) the float32 oracle stays under a quarter of every unchanged tau, the train counts lie inside [lo, hi],
and ref64 alone leaves at most a quarter of a step's rows ambiguous; two tap mutations that every 4-slot input passes and the new
inputs fail; one stuck-at-default mutation per scalar field and set.

Seeds.  Entry-point case i draws from AXES_SEED0 + i, populations keep test_gpu_train_ref64.schedule_inputs' own seeds.  Every
entry meets every condition on that first draw, judged by the float32 oracle and ref64 alone; no seed was drawn again and nothing
here was fitted to an engine result.

-s prints the oracle's worst ratios per group: the figures quoted in the GPU file's docstring.
"""
import contextlib
import dataclasses
import os
from unittest import mock

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import train_cases as GT
from tests import oracle32_runs as RC
from tests.oracle32_runs import TAUS, oracle_case, oracle_steps, oracle_train_steps
from tests.axes_cases import (AXES_SEED0, BATCH_SUM_SETS, PLAIN_CONFS, PLAIN_POPS, POPS, POP_DL_SEED, POP_IDS, SCALAR_EVAL_CASES,
                              SCALAR_POPS, SCALAR_SETS, TAP_CASES, TAP_IDS, TAP_NO_BN, TAP_POPS, WIDTHS, W_26, W_8, W_AV, case_seed,
                              count_spy, pop_entry, pop_eval_table, pop_inputs, scalar_case_hyper, spec_flag)

F32 = np.float32
WORST = {}          # group -> {quantity: worst ratio of the float32 oracle}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        print("\nfloat32 oracle, worst |got - ref64| / (2^-24 M):")
        for g in sorted(WORST):
            print(f"  {g:24s} " + "  ".join(f"{q} {v:.3g}" for q, v in sorted(WORST[g].items())))


def note(group, r):
    w = WORST.setdefault(group, {})
    for q, v in r.items():
        w[q] = max(w.get(q, 0.0), v)


def assert_quarter(r, taus, tag):
    for q, tau in taus.items():
        assert r.get(q, 0.0) * 4.0 <= tau, (tag, q, r[q], tau)


SCALAR_FIELDS = ("wd", "beta1", "beta2", "adam_eps", "bn_eps", "bn_momentum", "f1_threshold", "eta_max", "eta_min")


# ------------------------------------------------------------------------------------------------ coverage
def test_tap_cases_cover_every_slot():
    """Every slot index 0..7 of each modality in at least two cases, once in cell 0 and once in a later cell; slot 7 of both
    modalities in one cell; one tap used by two cells of a candidate; no selected slot has width 0; the three width sets."""
    for kind, col in (("s", 0), ("v", 1)):
        for slot in range(8):
            cases = [c for c in TAP_CASES if any(cell[col] == slot for cell in c[5])]
            assert len(cases) >= 2, (kind, slot, [c[0] for c in cases])
            assert any(c[5][0][col] == slot for c in cases), (kind, slot, "never in cell 0")
            assert any(cell[col] == slot for c in cases for cell in c[5][1:]), (kind, slot, "never in a later cell")
    assert any(cell[0] == 7 and cell[1] == 7 for c in TAP_CASES for cell in c[5])
    assert any(len({cell[0] for cell in c[5]}) < len(c[5]) for c in TAP_CASES)
    for cid, R, C, B, w, cells, bn, drpt, extra in TAP_CASES:
        assert all(w["s"][c[0]] > 0 and w["v"][c[1]] > 0 for c in cells), cid
        assert not (bn and len(cells) > 2), cid               # (deep BatchNorm stacks: DESIGN.md section 8, out of scope)
    assert {id(c[4]) for c in TAP_CASES} == {id(W_8), id(W_AV), id(W_26)}
    assert (len(W_8["s"]), len(W_8["v"])) == (8, 8) and (len(W_AV["s"]), len(W_AV["v"])) == (5, 3) and (len(W_26["s"]), len(W_26["v"])) == (2, 6)
    for w in (W_8["s"], W_8["v"]):
        used = [j for j, x in enumerate(w) if x]
        assert any(x == 0 and used[0] < j < used[-1] for j, x in enumerate(w)) and max(w) >= 1000
    assert any(c[3] > 64 or c[1] > 256 for c in TAP_CASES)      # one wide-path case
    assert {"lm1", "multitask", "alphas"} <= {e for c in TAP_CASES for e in c[8].split(",")}


def test_populations_cover_the_design():
    names = set(GT.TRAIN_SCHEDULES)
    assert {(p[1], p[2]) for p in TAP_POPS} >= {(n, m) for n in names for m in ("shared", "per_candidate")}
    assert any(p[1] == "wide_b65" for p in TAP_POPS)
    for pid, name, mode, axis, key in TAP_POPS:
        K = pop_entry(name)[5]
        assert K >= 3 and K <= 8, pid
        inp = pop_inputs((pid, name, mode, axis, key))
        confs = [c.tolist() for c in inp["confs"]]
        w = WIDTHS[key]
        assert (inp["hp"].s_sizes, inp["hp"].v_sizes) == (w["s"], w["v"]) and inp["hp"].bn == (name not in TAP_NO_BN), pid
        assert all(w["s"][c[0]] > 0 and w["v"][c[1]] > 0 for conf in confs for c in conf), pid
        assert {len(c) for c in confs} == ({1, 2} if inp["hp"].bn else {1, 2, 3}) and {c[2] for conf in confs for c in conf} == {0, 1, 2}, pid
        if key == "w8":
            slots = [{c[0] for c in conf} | {c[1] for c in conf} for conf in confs]
            assert any(max(s) <= 3 for s in slots) and any(min(s) >= 4 for s in slots), pid
            taps = [{("s", c[0]) for c in conf} | {("v", c[1]) for c in conf} for conf in confs[:3]]
            assert any(taps[a] & taps[b] for a in range(3) for b in range(a + 1, 3) if confs[a] != confs[b]), pid
    # the gathered rows (gather_body, gather_tap_off) exist only with two candidate groups, a plan that is not resident and
    # per-candidate orders (train.hip.h: setup_gather): that one population has the 8 + 8 widths and a candidate on slots 4..7 alone
    # with s7 and v7, so the mask's high bits, the sum over S slots >= 4 and the sw[4..7] terms of a V offset all run
    gathered = [p for p in TAP_POPS if p[2] == "per_candidate" and not pop_entry(p[1])[3].get("MFAS_SAME_GROUP") == "2"
                and pop_entry(p[1])[5] >= 8 and p[1] != "persistent"]
    assert [p[1] for p in gathered] == ["two_group_ab"] and gathered[0][4] == "w8", gathered
    confs = [c.tolist() for c in pop_inputs(gathered[0])["confs"]]
    assert any(min(min(c[0], c[1]) for c in conf) >= 4 and {7} <= {c[0] for c in conf} and {7} <= {c[1] for c in conf} for conf in confs)
    assert {c[0] for conf in confs for c in conf} >= {5, 7} and {c[1] for conf in confs for c in conf} >= {4, 6, 7}
    assert sum(p[4] == "w8" for p in TAP_POPS) >= 10 and {p[4] for p in TAP_POPS} == {"w8", "wav", "w26"}
    # plain cells: one population per chain family, depths 1..4, all three nonlinearities
    assert {p[1] for p in PLAIN_POPS} == (names - {"tap_major"}) | {"wide_b65"}
    seen = [PLAIN_CONFS[k % 4] for p in PLAIN_POPS for k in range(pop_entry(p[1])[5])]
    assert {len(c) for c in seen} == {1, 2, 3, 4} and {cell[2] for c in seen for cell in c} == {0, 1, 2}
    for p in PLAIN_POPS:
        hp = pop_inputs(p)["hp"]
        assert hp.allow_plain_cell and not hp.bn and hp.drpt == 0.0 and not hp.use_dropout
    # scalars: every set on every schedule (shared), per-candidate orders on the two-group and the resident one, a wide one
    for sid in SCALAR_SETS:
        mine = {(p[1], p[2]) for p in SCALAR_POPS if p[4] == sid}
        assert mine >= {(n, "shared") for n in names} | {("two_group_ab", "per_candidate"), ("persistent", "per_candidate"), ("wide_b65", "shared")}


def test_scalar_sets_cover_the_design():
    d = O.Hyper()
    for f in SCALAR_FIELDS:
        vals = {s[f] for s in SCALAR_SETS.values()}
        assert getattr(d, f) not in vals and len(vals) >= 2, (f, vals)
    col = {f: [s[f] for s in SCALAR_SETS.values()] for f in SCALAR_FIELDS}
    assert 0.0 in col["wd"] and 0.0 in col["beta1"] and 1.0 in col["bn_momentum"] and 1e-3 in col["adam_eps"]
    assert {1e-3, 1e-2} <= set(col["bn_eps"]) and 0.5 in col["f1_threshold"] and max(col["f1_threshold"]) > 0.5
    assert max(col["eta_max"]) >= 1e-2
    assert [sid for sid, s in SCALAR_SETS.items() if s["eta_max"] >= 3e-2] == list(BATCH_SUM_SETS)     # the term where it is needed, only
    assert [p[4] for p in POPS if spec_flag(p)] == [p[4] for p in SCALAR_POPS if p[4] in BATCH_SUM_SETS] and len(BATCH_SUM_SETS) == 1
    for a in SCALAR_FIELDS:              # a site that reads a neighbouring field: some set tells every two fields apart
        for b in SCALAR_FIELDS:
            assert a == b or any(s[a] != s[b] for s in SCALAR_SETS.values()), (a, b)
    zero = [sid for sid, s in SCALAR_SETS.items() if s["eta_max"] == 0.0 and s["eta_min"] == 0.0]
    assert zero
    inp = pop_inputs(next(p for p in SCALAR_POPS if p[4] == zero[0]))
    assert not inp["etas"].any() and inp["hp"].wd > 0                       # exactly 0, with weight decay on
    inp = pop_inputs(next(p for p in SCALAR_POPS if p[4] == "sb"))
    assert inp["etas"][0] == 5e-3 and inp["ehp"].beta2 == 0.9 and inp["ehp"].bn_eps == 1e-2 and inp["ehp"].f1_threshold == 0.7
    assert all("lm1" in c[8] and c[6] and G.eval_envs(G.case_hyper(c))[1:] for c in SCALAR_EVAL_CASES)


def test_helper_defaults_are_what_the_other_files_train():
    """The optional arguments of schedule_inputs / step_etas default to the values they replaced."""
    a = GT.schedule_inputs("general_mb2", "shared")
    assert a["hp"] == O.Hyper(R=65, C=17, B=20, bn=True, drpt=0.5, s_sizes=G.W_A["s"], v_sizes=G.W_A["v"], epochs=GT.EPOCHS)
    assert [c.tolist() for c in a["confs"]] == [list(GT.SCHED_CONFS[k]) for k in range(3)]
    assert np.array_equal(a["etas"], O.eta_sequence(1e-3, 1e-6, 1, 2, a["N"] / 20, GT.EPOCHS * 2))
    t = G.case_table(("x", 65, 17, 20, G.W_A, None, True, 0.5, ""), a["hp"], a["N"], 61, "bfloat16")
    assert all(np.array_equal(t[k], a["t"][k]) for k in t)


def test_schedules_the_layout_query_can_name():
    """Without a device the layout query (256 compute units) answers for the resident, the lean and the wide flag: the populations
    that must be resident or wide are, with 8-slot widths, plain cells and every scalar set."""
    from mfas_amd.engine import plan_population
    for spec in POPS:
        pid, name = spec[0], spec[1]
        if name not in ("persistent", "wide_b65", "lean_chain"):
            continue
        inp = pop_inputs(spec)
        env, cc = pop_entry(name)[3], pop_entry(name)[4]
        with mock.patch.dict(os.environ, env):
            plan = plan_population(inp["ehp"], inp["confs"], "cuda:0", cc)
        if plan["compute_units"] != 256:
            continue
        if name == "persistent":
            assert plan["persistent"] and plan["resident_units"] > 0 and not plan["wide"], (pid, plan)
        if name == "wide_b65":
            assert plan["wide"] and not plan["persistent"], (pid, plan)
        if name == "lean_chain":
            assert plan["lean_chain"] and not plan["persistent"] and not plan["wide"], (pid, plan)


def test_plain_cells_need_the_flag():
    """The same hyper-parameters without allow_plain_cell are refused by the oracle and by the engine's validator."""
    from mfas_amd.engine import plan_population
    from tests.helpers import engine_hyper
    hp = dataclasses.replace(pop_inputs(PLAIN_POPS[0])["hp"], allow_plain_cell=False)
    with pytest.raises(ValueError, match="illegal cell variant"):
        hp.check()
    with pytest.raises(RuntimeError, match="illegal cell variant"):
        plan_population(engine_hyper(hp), [np.array(PLAIN_CONFS[0])], "cuda:0")


def case_ratios(case, dtype, seed, hp=None, steps=True):
    """oracle_case (and oracle_train_steps) of an entry-point case; hp: the case's hyper-parameters replaced."""
    patch = mock.patch.object(G, "case_hyper", lambda c: hp) if hp is not None else contextlib.nullcontext()
    with patch, count_spy() as spy:
        r = oracle_case(case, dtype, seed=seed)
        if steps:
            r.update({"train_" + q: v for q, v in oracle_train_steps(case, dtype, seed=seed).items()})
    spy.check(case[0])
    return r


def assert_case_quarter(r, tag, steps=True):
    assert_quarter(r, TAUS, tag)
    if not steps:
        return
    assert_quarter({"train_" + q: r["train_" + q] for q in GT.TAUS}, {"train_" + q: tau for q, tau in GT.TAUS.items()}, tag)
    assert r["train_count"] == 0.0, tag


@pytest.mark.parametrize("case", TAP_CASES, ids=TAP_IDS)
def test_tap_cases_calibration_margin(case):
    """The entry points and steps 1..3 of every tap case, all three table dtypes."""
    for dtype in G.DTYPES:
        r = case_ratios(case, dtype, case_seed(case[0]))
        note("tap cases", r)
        assert_case_quarter(r, (case[0], dtype))


def pop_ratios(spec, hp_of=None, etas=None):
    """Every candidate of a population on the GPU test's inputs: the float32 oracle's worst ratios over steps 1..3."""
    inp = pop_inputs(spec)
    per = inp["ehp"].order_per_candidate
    worst = {}
    for k, conf in enumerate(inp["confs"]):
        with count_spy() as spy:
            r = oracle_steps(conf, inp["hp"], inp["p0s"][k], inp["t"], inp["order"][k] if per else inp["order"], inp["etas"],
                             inp["seeds"][k], (1, 2, 3), GT.TAUS, f"{spec[0]} cand {k}", batch_sum_term=spec_flag(spec))
        worst = {q: max(worst.get(q, 0.0), v) for q, v in r.items()}
        assert not (inp["hp"].bn and len(conf) > 2), spec[0]
        spy.check(f"{spec[0]} cand {k}")
    return worst


def pop_entry_ratios(inp):
    """oracle_case's quantities for every candidate of a population, on the inputs of
    test_gpu_axes_ref64.check_population_entry_points."""
    hp, tdv = inp["hp"], pop_eval_table(inp)
    worst = {}
    for k, conf in enumerate(inp["confs"]):
        p0 = inp["p0s"][k]
        f = G.feats_of(tdv)
        lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
        r = {"forward": R64.worst_ratio(O.forward({q: v.copy() for q, v in p0.items()}, conf, hp, f, False)[0], lg, Ml)[0]}
        f = G.feats_of(tdv, 0, hp.B)
        p32 = {q: v.copy() for q, v in p0.items()}
        lg32, c32 = O.forward(p32, conf, hp, f, True, seed=inp["seeds"][k], step=3)
        lg, Ml, cache = R64.forward(p0, conf, hp, f, True, seed=inp["seeds"][k], step=3)
        r["forward_train"] = R64.worst_ratio(lg32, lg, Ml)[0]
        rng = np.random.default_rng(POP_DL_SEED + k)
        dl = (rng.standard_normal((hp.B, hp.C)) / hp.B).astype(F32)
        dl[rng.random((hp.B, hp.C)) < 0.1] *= F32(1e-3)
        g32 = O.backward(p32, hp, c32, dl)
        G64, MG = R64.backward(p0, hp, cache, dl)
        r["backward"] = max(R64.worst_ratio(g32[q], G64[q], MG[q])[0] for q in g32)
        worst = {q: max(worst.get(q, 0.0), v) for q, v in r.items()}
    return worst


@pytest.mark.parametrize("spec", PLAIN_POPS, ids=[p[0] for p in PLAIN_POPS])
def test_plain_populations_entry_points_calibration_margin(spec):
    r = pop_entry_ratios(pop_inputs(spec))
    note("plain entry points", r)
    assert_quarter(r, TAUS, spec[0])


@pytest.mark.parametrize("spec", POPS, ids=POP_IDS)
def test_populations_calibration_margin(spec):
    r = pop_ratios(spec)
    note(spec[3] + (" " + spec[4] if spec[3] == "scalar" else ""), r)
    assert_quarter(r, GT.TAUS, spec[0])
    assert r["count"] == 0.0, spec[0]


@pytest.mark.parametrize("sid", list(SCALAR_SETS))
@pytest.mark.parametrize("case", SCALAR_EVAL_CASES, ids=[c[0] for c in SCALAR_EVAL_CASES])
def test_scalar_eval_cases_calibration_margin(case, sid):
    hp = scalar_case_hyper(case, sid)
    for dtype in G.DTYPES:
        seed = AXES_SEED0 + 100 + SCALAR_EVAL_CASES.index(case)
        r = case_ratios(case, dtype, seed, hp=hp, steps=False)
        note("scalar eval " + sid, r)
        assert_case_quarter(r, (case[0], sid, dtype), steps=False)
        conf, p0 = G.case_params(case, hp, seed)
        t = G.case_table(case, hp, G.N_EVAL, seed, dtype)
        lg, Ml, _ = R64.forward(p0, conf, hp, G.feats_of(t), False)
        _, _, lo, hi = R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, z=t["multilabel"], pos_weight=G.pos_weight(hp))
        amb = int(round((hi - lo - 2 * len(lg)) / float(1 << 32)))
        assert 4 * amb <= len(lg), (case[0], sid, dtype, amb)
        lg32 = O.forward({k: v.copy() for k, v in p0.items()}, conf, hp, G.feats_of(t), False)[0]
        assert lo <= O.f1_samples_fixed(lg32, t["multilabel"], hp.f1_threshold) <= hi


# ------------------------------------------------------------------------------------------------ tap mutations
def _pad16(a):
    return np.pad(a, ((0, 0), (0, (-a.shape[1]) % 16)))


def taps_slot_mod4(feats, conf, hp):
    """Slot j read through the table pointer of slot j % 4, with slot j's own row stride: the columns that mistake would read
    (zeros where slot j % 4 is unused or ends)."""
    out = dict(feats)
    for kind, sizes in (("s", hp.s_sizes), ("v", hp.v_sizes)):
        for j in range(4, len(sizes)):
            key, src = f"{kind}{j}", f"{kind}{j % 4}"
            if key not in feats or not sizes[j]:
                continue
            n, w = feats[key].shape
            cw = w + (-w) % 16
            flat = _pad16(feats[src]).ravel() if src in feats else np.zeros(0, F32)
            flat = np.concatenate([flat, np.zeros(max(0, n * cw - flat.size), F32)])
            out[key] = flat[:n * cw].reshape(n, cw)[:, :w].astype(F32)
    return out


def taps_gathered(feats, conf, hp, limit=4):
    """A candidate's gathered rows (sweep.hip.h: gather_body writes the taps it uses, S then V in slot order, each as a [Bp][width]
    block at gather_tap_off; the feature units read them back there) with the offset summed over slots 0 .. limit - 1 only:
    blocks of slots >= limit overlap earlier ones.  limit = 8 is the kernel's own layout and returns the rows unchanged."""
    sw = [w + (-w) % 16 for w in hp.s_sizes] + [0] * (8 - len(hp.s_sizes))
    vw = [w + (-w) % 16 for w in hp.v_sizes] + [0] * (8 - len(hp.v_sizes))
    n = len(next(iter(feats.values())))
    Bp = 16 * max(1, -(-n // 16))

    def off(kind, tap):
        o = sum(sw[u] for u in range(limit) if kind == "v" or u < tap)
        return (o + sum(vw[u] for u in range(limit) if kind == "v" and u < tap)) * Bp
    used = sorted({("s", int(c[0])) for c in conf}) + sorted({("v", int(c[1])) for c in conf})
    buf = np.zeros((sum(sw) + sum(vw)) * Bp + max(sw + vw) * Bp, F32)
    for kind, tap in used:
        blk = np.zeros((Bp, (sw if kind == "s" else vw)[tap]), F32)
        a = feats[f"{kind}{tap}"]
        blk[:n, :a.shape[1]] = a
        buf[off(kind, tap):off(kind, tap) + blk.size] = blk.ravel()
    out = dict(feats)
    for kind, tap in used:
        cw = (sw if kind == "s" else vw)[tap]
        a = feats[f"{kind}{tap}"]
        out[f"{kind}{tap}"] = buf[off(kind, tap):off(kind, tap) + Bp * cw].reshape(Bp, cw)[:n, :a.shape[1]].copy()
    return out


def misreading(mutate):
    """O.forward with its taps passed through `mutate` (ref64 has its own forward: the reference is untouched)."""
    real = O.forward

    def forward(params, conf, hp, feats, train, **kw):
        return real(params, conf, hp, mutate(feats, conf, hp), train, **kw)
    return mock.patch.object(O, "forward", forward)


def test_gathered_rows_restatement_is_the_identity_at_eight_slots():
    inp = pop_inputs(TAP_POPS[0])
    f = G.feats_of(inp["t"])
    for conf in inp["confs"]:
        g = taps_gathered(f, conf, inp["hp"], limit=8)
        assert all(np.array_equal(g[k], f[k]) for k in f)


TAP_MUTATIONS = {"slot_mod4": taps_slot_mod4, "gather_off4": taps_gathered}


@pytest.mark.parametrize("mut", list(TAP_MUTATIONS))
def test_tap_mutations_pass_the_four_slot_inputs_and_fail_the_new_ones(mut):
    """The slot index taken modulo 4, and the gathered block offset summed over slots 0..3 only: on every 4-slot input (the schedule
    populations of test_gpu_train_ref64.py, three cases of test_gpu_ref64.py) the mutated float32 oracle is the unmutated one, under
    a quarter of every tau; on the new inputs every population that selects a slot >= 4 exceeds a tau."""
    mutate = TAP_MUTATIONS[mut]
    with misreading(mutate):
        for cid in ("r16b", "r65a", "r256a"):
            case = G.CASES[G.CASE_IDS.index(cid)]
            old = oracle_case(case, "bfloat16")
            old.update({"train_" + q: v for q, v in oracle_train_steps(case, GT.case_dtype(cid)).items()})
            assert_case_quarter(old, (mut, cid))
        for name in ("lean_chain", "two_group_ab"):
            inp = GT.schedule_inputs(name, "per_candidate")
            for k, conf in enumerate(inp["confs"][:3]):
                r = oracle_steps(conf, inp["hp"], inp["p0s"][k], inp["t"], inp["order"][k], inp["etas"], inp["seeds"][k], (1, 2, 3),
                                 GT.TAUS, f"{mut} {name}")
                assert_quarter(r, GT.TAUS, (mut, name, k))
        for spec in (s for s in TAP_POPS if s[2] == "per_candidate" and s[1] in ("lean_chain", "two_group_ab", "persistent", "general_mb2")):
            inp = pop_inputs(spec)
            hit, hit_high = 0, False
            for k, conf in enumerate(inp["confs"][:4]):
                r = oracle_steps(conf, inp["hp"], inp["p0s"][k], inp["t"], inp["order"][k], inp["etas"], inp["seeds"][k], (1, 2, 3),
                                 GT.TAUS, f"{mut} {spec[0]}")
                high = max(int(c[j]) for c in conf for j in (0, 1)) >= 4
                bad = {q: r[q] for q, tau in GT.TAUS.items() if not r[q] <= tau}
                if mut == "slot_mod4":
                    assert bool(bad) == high, (mut, spec[0], k, r)
                hit += bool(bad)
                hit_high |= bool(bad) and min(int(c[j]) for c in conf for j in (0, 1)) >= 4
            assert hit >= 1, (mut, spec[0])
            assert hit_high or spec[1] != "two_group_ab", (mut, spec[0], "the gather schedule's slots-4..7 candidate passes")
        if mut == "slot_mod4":              # (the eval forward reads the table too: tab.s[d.tap] in k_eval)
            for case in TAP_CASES:
                if max(c[j] for c in case[5] for j in (0, 1)) >= 4:
                    r = oracle_case(case, "float32", seed=case_seed(case[0]))
                    assert r["forward"] > G.TAU_LOGITS and r["backward"] > G.TAU_GRAD, (case[0], r)


# ------------------------------------------------------------------------------------------------ scalars: stuck at the default
# Recorded: what did not work as first chosen (judged by the float32 oracle and ref64 alone).
# * Set 'sb' had eta_max = 3e-2.  Three steps at that rate move the biases so far that the float32 batch sum behind the running
#   mean carries a rounding ref64's M_mu does not count (the effect tests/test_inputs_cpu.py describes for DEAD_BIAS): the oracle
#   itself reached 1.2 .. 1.8 on the running statistics of steps 2 and 3 on seven of the twelve populations, on every draw of the
#   table tried and whatever bn_momentum (0.05 .. 1.0) was.  At eta_max = 5e-3 every population keeps the quarter rule; eta_max >= 1e-2
#   is set 'sa' (1e-2).  'sb' stays at 5e-3.  Measured again with ref64's batch_sum_term on 'sb' with eta_max = 3e-2 (allowed: 1.0):
#     without the term   runstat 1.17 .. 1.77 on seven of the twelve populations (the others 0.68 .. 0.81)
#     the mean's term    0.20 .. 0.91 on eleven; general_mb2 1.33, on a running VARIANCE (cell 0, step 3: the variance's own batch
#                        sum, n terms whose mean is a variance of about 7)
#     both terms         0.20 .. 0.60 on all twelve
#   so the variance's term (n - 1) var is part of batch_sum_term, and set 'sd' (3e-2, its other fields its own) runs with it:
#   test_populations_calibration_margin holds it to the quarter rule and to the ambiguity condition like every other set.
# * Set 'sc' has every learning rate exactly 0 (the cosine schedule starts at eta_max and, at eta_max = 0, restarts at every step),
#   so its adam_eps and its eta_min cannot show: w' = w - 0 * m / (sqrt(v) / bc2s + eps).  Both separate in sets 'sa' and 'sb'.
NOT_SEPARABLE = {("sc", "adam_eps"), ("sc", "eta_min")}
POWER_SCHEDULE = "general_mb2"      # the inputs on which every field of every set must separate (R = 65, C = 17, B = 20, K = 3)


def stuck_ratios(sid, field, name=POWER_SCHEDULE):
    """The float32 oracle with `field` left at its default and the rest of set `sid` applied, against ref64 at the set's values, on
    the inputs of one schedule entry."""
    spec = next(p for p in SCALAR_POPS if p[4] == sid and p[1] == name and p[2] == "shared")
    inp = pop_inputs(spec)
    hp = inp["hp"]
    hq = dataclasses.replace(hp, **{field: getattr(O.Hyper(), field)})
    etas_q = GT.step_etas(inp["N"], hp.B, hq.eta_max, hq.eta_min)
    real = RC.oracle_step32

    def stuck(st, conf, hp_, batch, seed, step, eta, t, *a, **kw):
        return real(st, conf, hq, batch, seed, step, etas_q[step], t, *a, **kw)
    worst = {}
    with mock.patch.object(RC, "oracle_step32", stuck):
        for k, conf in enumerate(inp["confs"]):
            r = oracle_steps(conf, hp, inp["p0s"][k], inp["t"], inp["order"], inp["etas"], inp["seeds"][k], (1, 2, 3), GT.TAUS,
                             f"{sid} {field}", batch_sum_term=spec_flag(spec))
            worst = {q: max(worst.get(q, 0.0), v) for q, v in r.items()}
    return worst


@pytest.mark.parametrize("field", [f for f in SCALAR_FIELDS if f != "f1_threshold"])
@pytest.mark.parametrize("sid", list(SCALAR_SETS))
def test_scalar_stuck_at_its_default_exceeds_a_tau(sid, field):
    """A kernel that keeps a constant where it should read the field: over a tau on steps 1..3 of POWER_SCHEDULE's inputs, for
    every field of every set.  (Set 'sc' has eta_max = eta_min = 0; a learning rate stuck at its default moves w, which ref64 at
    the set's values holds bit-identical.)"""
    r = stuck_ratios(sid, field)
    bad = {q: round(r[q], 2) for q, tau in GT.TAUS.items() if not r[q] <= tau}
    print(f"\nstuck {sid} {field}: {({q: round(v, 3) for q, v in r.items()})}")
    if (sid, field) in NOT_SEPARABLE:
        assert not bad and r["w"] == 0.0, (sid, field, r)
        return
    assert bad, (sid, field, r)
    want = {"bn_momentum": {"runstat"}, "eta_max": {"w"}, "eta_min": {"w"}, "adam_eps": {"w"}}.get(field)
    assert want is None or want & set(bad), (sid, field, bad)


@pytest.mark.parametrize("sid", list(SCALAR_SETS))
@pytest.mark.parametrize("case", SCALAR_EVAL_CASES, ids=[c[0] for c in SCALAR_EVAL_CASES])
def test_f1_threshold_stuck_at_its_default_leaves_the_interval(case, sid):
    """The dev pass's F1 sum at the default threshold 0.3 lies outside ref64's [lo, hi] at the set's threshold; so does the logit
    check for a bn_eps stuck at 1e-5 (k_eval reads both)."""
    hp = scalar_case_hyper(case, sid)
    seed = AXES_SEED0 + 100 + SCALAR_EVAL_CASES.index(case)
    conf, p0 = G.case_params(case, hp, seed)
    t = G.case_table(case, hp, G.N_EVAL, seed, "bfloat16")
    f = G.feats_of(t)
    lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
    _, _, lo, hi = R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, z=t["multilabel"], pos_weight=G.pos_weight(hp))
    lg32 = O.forward({k: v.copy() for k, v in p0.items()}, conf, hp, f, False)[0]
    assert lo <= O.f1_samples_fixed(lg32, t["multilabel"], hp.f1_threshold) <= hi
    assert not lo <= O.f1_samples_fixed(lg32, t["multilabel"], O.Hyper().f1_threshold) <= hi
    hq = dataclasses.replace(hp, bn_eps=O.Hyper().bn_eps)
    bad = O.forward({k: v.copy() for k, v in p0.items()}, conf, hq, f, False)[0]
    assert R64.worst_ratio(bad, lg, Ml)[0] > G.TAU_LOGITS


# ------------------------------------------------------------------------------------------------ the host side of the scalars
def test_adam_step_scalars_equal_the_oracles_bit_for_bit():
    from mfas_amd.scheduler import adam_step_scalars
    T = 2000
    etas = O.eta_sequence(3e-2, 1e-5, 1, 2, 37.5, T)
    for sid, s in list(SCALAR_SETS.items()) + [("default", dict(beta1=0.9, beta2=0.999))]:
        hp = dataclasses.replace(O.Hyper(), beta1=s["beta1"], beta2=s["beta2"])
        got = adam_step_scalars(etas, s["beta1"], s["beta2"])
        assert got.dtype == F32 and got.shape == (T, 2)
        want = np.array([O.adam_scalars(float(etas[t - 1]), t, hp) for t in range(1, T + 1)], F32)
        assert got.tobytes() == want.tobytes(), sid
    assert not adam_step_scalars(np.zeros(5), 0.0, 0.99)[:, 0].any()


def test_adam_hyper_carries_the_optimizers_fields():
    import torch
    from mfas_amd import Hyper
    from mfas_amd.train_ntu import _adam_hyper
    p = torch.nn.Parameter(torch.zeros(3))
    for s in SCALAR_SETS.values():
        opt = torch.optim.Adam([p], lr=1e-3, betas=(s["beta1"], s["beta2"]), eps=s["adam_eps"], weight_decay=s["wd"])
        hp = _adam_hyper(Hyper(), opt)
        assert (hp.wd, hp.beta1, hp.beta2, hp.adam_eps) == (s["wd"], s["beta1"], s["beta2"], s["adam_eps"])
    d = Hyper()
    assert _adam_hyper(Hyper(), None) == d and _adam_hyper(Hyper(), torch.optim.Adam([p], weight_decay=1e-4)) == d
