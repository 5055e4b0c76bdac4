"""CPU side of the value-domain tests (tests/test_gpu_inputs_ref64.py judges the kernels on the GPU):

* INPUT_CASES: (base case of ref64_cases.CASES or wide_cases.WIDE_CASES, transform of tests/input_edges.py, table
  dtype) — a covering design, checked by test_input_cases_cover_the_design;
* calibration: on exactly the inputs the GPU test uses, the float32 oracle stays under a quarter of every existing tau (no tau
  changes, none per case), the counts lie inside [lo, hi], and ref64 marks at most a quarter of the rows of any pass ambiguous;
* mutations: float32 results that are wrong in a way only these values expose stay under tau on the untransformed inputs and
  exceed it on the transformed ones.

Seeds: case i draws its parameters, taps and orders from INPUT_SEED0 + i (the wide case keeps test_gpu_wide_ref64's own seeds).
Two bases were tried, 7000 and 7100, judged by the float32 oracle and ref64 alone: on 7000 one element of r65a-dup reaches 1.002 of
the allowed 1.0 on the train running statistics (TAU_RUNSTAT's x4 margin is narrow, as test_gpu_train_ref64.py says of its own
base); on 7100 every condition holds for every case.

The ambiguity condition is held on the eval pass of every case and on every train step, except where no seed can meet it
(ambiguity_exempt): under train-mode BatchNorm ref64's magnitude grows by about rstd per cell, so the four BatchNorm cells of r16b
(on the untransformed inputs too) and the transforms that take a batch variance towards 0 ('dup', 'offset', 'dead') under
BatchNorm, 'deadrelu' and 'bigmean' with them, leave most rows of a train batch ambiguous on every seed (test_ambiguity_exemptions_do_not_depend_on_the_seed;
DESIGN.md section 8).  Three entries needed another draw to meet it (SEED_OVERRIDE); r65a-scaled and the wide w65-tiny met it on
none of 60 seeds and were replaced by r32a-scaled and the wide w256-bighead.

DEAD_BIAS (tests/input_edges.py) = 64, calibrated here.  Its size is not what limits it: a first cell with a ReLU and a bias of
+D brings the oracle to 1.1 .. 2.0 on the running mean at D = 8, 16 and 64 alike (the float32 batch sum of n values near D carries a
rounding of its own that ref64's M_mu does not count), so the BatchNorm cases of 'dead' have a sigmoid first cell (r16b, r129a,
r17b; their later ReLU cells are dead too), where 64 keeps the margin; r32a / r65a / r256a / r16a do not, at any D.

'dead' conflates two things, and only one of them needs that rounding counted.  'deadrelu' (the -64 half alone) keeps the margin
under the unchanged ref64 on a ReLU FIRST cell under BatchNorm, and runs so: the lean chain (l16c, resident at one candidate), the
general chain at 4, 2 and 1 m-blocks (r16a, r32a, r256a: also R >= 256) and the wide path (w65).  'bigmean' (the +64 half alone) on
the same five bases, and 'dup' on the wide w65 (64 identical rows: 2.19 / 3.87 on the running statistics without it), are judged
with ref64's batch_sum_term (FLAGGED; tests/ref64.py::forward derives it), under the same taus.  What the term costs is measured in
test_batch_sum_term_only_loosens_and_by_at_most_n, what the flagged entries still see in
test_value_mutations_on_the_split_dead_transforms.  l16c is a base case of this file alone (EXTRA_CASES says why).
"""
import contextlib
from unittest import mock

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import input_edges as IE
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import train_cases as GT
from tests import wide_cases as GW
from tests.oracle32_runs import TAUS, oracle_case, oracle_train_steps
from tests.wide_oracle32 import wide_oracle_case
from tests.input_cases import (EXTRA_CASES, FLAGGED, INPUT_CASES, INPUT_IDS, INPUT_SEED0, POP_CASES, base_case, entry_flag, entry_seed,
                               flagged, is_wide, make_edit)

F32 = np.float32


def ambiguity_exempt(cid, how, hp):
    """Train steps on which no seed can bring ref64's count interval under a quarter of the batch: under train-mode BatchNorm
    its magnitude grows by about rstd per cell, so the four BatchNorm cells of r16b (on the untransformed inputs too), and the
    transforms that take a column's batch variance towards 0 ('dup', 'offset', 'dead', 'deadrelu': rstd up to 1 / sqrt(eps) =
    316) or that are judged with the batch-sum term ('bigmean': M_mu of the +64 columns is 64 (n - 1))."""
    return hp.bn and (cid == "r16b" or how in ("dup", "offset", "dead", "deadrelu", "bigmean"))


def ambiguous_rows(lo, hi, n, hp):
    """The number of rows dev_stats let go either way, from the interval it returned."""
    return int(round((hi - lo - 2 * n) / float(1 << 32))) if hp.loss_mode == 1 else hi - lo


def check_inputs_conditions(conf, hp, p, t, tag):
    """Conditions on the inputs alone (reference only): at most a quarter of the rows of a pass ambiguous; a multi-label head's
    float32 logits below 16 in magnitude (above, the reference's own float32 loss starts to saturate: the status tests' subject)."""
    f = G.feats_of(t)
    lg, Ml, _ = R64.forward(p, conf, hp, f, False)
    n = len(lg)
    _, _, lo, hi = R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, labels=t["label"], vlogit=f.get("vlogit"), slogit=f.get("slogit"),
                                 z=t.get("multilabel"), pos_weight=G.pos_weight(hp))
    amb = ambiguous_rows(lo, hi, n, hp)
    assert 4 * amb <= n, (tag, "ambiguous rows", amb, n)
    if hp.loss_mode == 1:
        lg32 = O.forward({k: v.copy() for k, v in p.items()}, conf, hp, f, False)[0]
        assert np.abs(lg32).max() < 16.0, (tag, float(np.abs(lg32).max()))
    return amb


def assert_first_cell_column_is_dead(conf, hp, p, t, tag):
    """'deadrelu': the first cell is a ReLU and its first r = 0 mod 3 column is exactly 0 on every row of the first batch, batch
    variance exactly 0, in ref64's own train-mode forward."""
    assert hp.bn and int(conf[0][2]) == 0, tag
    col = int(IE.dead_columns(conf, hp, 0)[0])
    c = R64.forward(p, conf, hp, G.feats_of(t, 0, min(hp.B, len(t["label"]))), True)[2]["cells"][0]
    assert c["var"][col] == 0.0 and not c["a"][:, col].any() and (c["y"][:, col] < -DEAD_MARGIN).all(), (tag, col, c["var"][col])


DEAD_MARGIN = 32.0      # a dead column's pre-activations lie below -32: far from the kink, on every row


def entry_ratios(i):
    """All nine quantities of INPUT_CASES[i] for the float32 oracle, on the GPU test's inputs; also asserts the input conditions."""
    cid, how, dtype = INPUT_CASES[i]
    edit = make_edit(how)
    flag = entry_flag(i)
    counts = []
    real = R64.train_step64

    def spy(state, conf, hp, batch, *a, **kw):
        exp = real(state, conf, hp, batch, *a, **kw)
        counts.append((exp["count"], len(batch["label"]), hp))
        return exp

    def checked(conf, hp, p0, t, dt):
        p, t2 = edit(conf, hp, p0, t, dt)
        check_inputs_conditions(conf, hp, p, t2, INPUT_IDS[i])
        if how == "deadrelu" and (not is_wide(cid) or conf.tolist() == base_case(cid)[5]):
            assert_first_cell_column_is_dead(conf, hp, p, t2, INPUT_IDS[i])
        return p, t2

    with mock.patch.object(R64, "train_step64", spy):
        if is_wide(cid):
            case = base_case(cid, dtype)
            seed = GW.SEED0 + GW.WIDE_IDS.index(cid)
            worst = {}
            for k, cells in enumerate(GW.case_confs(case)):
                r = wide_oracle_case(case, k, cells, edit=checked, batch_sum_term=flag)
                r.update({"train_" + q: v for q, v in oracle_train_steps(GW.base_case(case, cells), dtype, seed=seed, edit=checked,
                                                                           batch_sum_term=flag).items()})
                worst = {q: max(worst.get(q, 0.0), v) for q, v in r.items()}
        else:
            case = base_case(cid)
            worst = oracle_case(case, dtype, seed=entry_seed(i), edit=checked, batch_sum_term=flag)
            worst.update({"train_" + q: v for q, v in oracle_train_steps(case, dtype, seed=entry_seed(i), edit=checked,
                                                                           batch_sum_term=flag).items()})
    for (lo, hi), n, hp in counts:
        assert ambiguity_exempt(cid, how, hp) or 4 * ambiguous_rows(lo, hi, n, hp) <= max(n, 4), (INPUT_IDS[i], "ambiguous rows in a train step", lo, hi, n)
    return worst


# The float32 oracle's worst ratio per transform over INPUT_CASES (what the test below asserts on, DEAD_BIAS = 64), under tau / 4:
#   how        forward fwd_train backward run_stats train m   v       w     runstat loss
#   (tau / 4)     1.5     1.5     5       1       5       0.25    5       1      0.25
#   scaled       0.14    0.18    3.66    0.54    0.81    0.18    4.04    0.80   0.001
#   tiny         0.81    0.77    3.15    0.79    0.98    0.17    4.23    0.79   0.010
#   sparse       0.08    0.16    2.57    0.83    0.89    0.18    4.08    0.78   0.008
#   offset       0.08    0.10    2.04    0.74    0.87    0.16    3.56    0.77   0.001
#   dup          0.05    0.15    2.30    0.80    0.92    0.18    4.16    0.82   0.002
#   onelabel     0.19    0.12    2.91    0.81    0.71    0.17    3.83    0.82   0.003
#   dead         0.51    0.74    3.02    0.77    0.79    0.17    3.66    0.81   0.004
#   bighead      0.17    0.14    3.46    0.80    0.86    0.18    4.13    0.76   0.002
#   mlrows       0.17    0.32    2.50    0.60    0.92    0.18    4.12    0.79   0.002
#   deadrelu     0.05    0.009   2.20    0.80    0.87    0.17    3.92    0.82   < 0.001
#   bigmean      0.62    0.023   1.58    0.81    0.73    0.17    3.65    0.82   < 0.001      (judged with batch_sum_term)
#   ('dup' with the wide w65 entry, judged with batch_sum_term: forward 0.11, the other columns as above; without the term that
#    entry is at 2.19 on the running statistics and 3.87 on the train runstat)


@pytest.mark.parametrize("i", range(len(INPUT_CASES)), ids=INPUT_IDS)
def test_input_cases_calibration_margin(i):
    """The float32 oracle on the transformed inputs stays under a quarter of every unchanged tau; the train count is inside
    [lo, hi]; ref64 leaves at most a quarter of the rows of any pass ambiguous."""
    r = entry_ratios(i)
    for q, tau in TAUS.items():
        assert r.get(q, 0.0) * 4.0 <= tau, (INPUT_IDS[i], q, r[q], tau)
    for q, tau in GT.TAUS.items():
        assert r["train_" + q] * 4.0 <= tau, (INPUT_IDS[i], q, r["train_" + q], tau)
    assert r["train_count"] == 0.0, INPUT_IDS[i]


@pytest.mark.parametrize("cid,how", [("r16b", None), ("r32a", "offset"), ("r65a", "dup"), ("r129a", "dead"), ("r32a", "deadrelu"),
                                     ("r32a", "bigmean")])
def test_ambiguity_exemptions_do_not_depend_on_the_seed(cid, how):
    """Why ambiguity_exempt exempts what it does: on each of eight seeds ref64 leaves more than a quarter of the first full train
    batch ambiguous — on the untransformed r16b, and on a BatchNorm case under each of 'offset', 'dup', 'dead', 'deadrelu' and
    'bigmean' (the last with the batch-sum term, as its entries are judged; 8 .. 16 of 20 rows without it)."""
    case = base_case(cid)
    hp = G.case_hyper(case)
    assert ambiguity_exempt(cid, how, hp)
    for seed in range(INPUT_SEED0, INPUT_SEED0 + 8):
        conf, p = G.case_params(case, hp, seed)
        t = G.case_table(case, hp, hp.B, seed, "float32")
        if how:
            p, t = make_edit(how)(conf, hp, p, t, "float32")
        zero = {k: np.zeros_like(v) for k, v in p.items()}
        lo, hi = R64.train_step64({"w": p, "m": zero, "v": zero}, conf, hp, t, seed, 0, 1e-3, 1, G.TAU_LOGITS, GT.TAU_V,
                                   batch_sum_term=flagged(cid, how))["count"]
        assert 4 * (hi - lo) > hp.B, (cid, how, seed, lo, hi)


def test_input_cases_cover_the_design():
    # (nine transforms in at most 40 entries, before 'deadrelu' and 'bigmean'; eleven now, in proportion)
    assert 30 <= len(INPUT_CASES) <= 48 and len(set(INPUT_CASES)) == len(INPUT_CASES)
    per = {how: [(base_case(c, dt), dt) for c, h, dt in INPUT_CASES if h == how] for how in IE.HOWS}
    for how, lst in per.items():
        assert len(lst) >= 3, how
        bn = [c[6] for c, _ in lst]
        assert any(bn) and (not all(bn) or how in ("dup", "dead", "deadrelu", "bigmean")), how
        if how in ("dup", "dead", "deadrelu", "bigmean"):
            assert sum(bn) >= 2, how
        assert {dt for _, dt in lst} == set(G.DTYPES), how
        lm1 = ["lm1" in c[8] for c, _ in lst]
        assert not (how == "bighead" and any(lm1)) and not (how == "mlrows" and not all(lm1)), how
    ids = {c for c, _, _ in INPUT_CASES}
    assert ids & {"r16a", "r16b"}                                                       # the lean chain
    assert ids & {"r65a", "r80a"} and ids & {"r32a", "r129a"} and ids & {"r33a", "r17a"}    # the general chain, 1 / 2 / 4 m-blocks
    extras = set().union(*[set(base_case(c)[8].split(",")) for c in ids])
    assert {"multitask", "alphas", "lm1"} <= extras
    assert ids & {"r17a", "r80a"}
    assert any(base_case(c)[1] >= 256 for c in ids) and any(is_wide(c) for c in ids)
    assert all(is_wide(c) or c in G.CASE_IDS or c in EXTRA_CASES for c in ids)
    # BatchNorm and a ReLU first cell in every entry of the two halves of 'dead' and in the wide 'dup'; every BatchNorm transcription
    # under each half: the lean chain (resident at one candidate), the general chain at 1 / 2 / 4 m-blocks, R >= 256, the wide path
    from tests.wide_plans import plan
    for how in ("deadrelu", "bigmean"):
        mine = [(c, base_case(c)) for c, h, _ in INPUT_CASES if h == how]
        assert all(bc[6] and bc[5][0][2] == 0 for _, bc in mine), how
        narrow = [bc for c, bc in mine if not is_wide(c)]
        plans = [plan(G.case_hyper(bc), [bc[5]]) for bc in narrow]
        assert any(p[5] == 1 and p[0] == 1 for p in plans), how
        general = {-(-bc[3] // 16) if bc[3] <= 32 else 4 for bc, p in zip(narrow, plans) if p[5] == 0}
        assert general == {1, 2, 4}, (how, general)
        assert any(bc[1] >= 256 for bc in narrow) and any(is_wide(c) and bc[3] == 64 for c, bc in mine), how
        assert all((INPUT_IDS[i] in FLAGGED) == (how == "bigmean") for i, e in enumerate(INPUT_CASES) if e[1] == how), how
    wdup = [i for i, e in enumerate(INPUT_CASES) if e[1] == "dup" and is_wide(e[0])]
    assert wdup and all(base_case(INPUT_CASES[i][0])[6] and base_case(INPUT_CASES[i][0])[3] == 64 and entry_flag(i) for i in wdup)
    assert FLAGGED == {INPUT_IDS[i] for i, e in enumerate(INPUT_CASES) if e[1] == "bigmean"} | {INPUT_IDS[i] for i in wdup}
    for cid, bc in EXTRA_CASES.items():     # (a base case of this file is one the lean chain runs)
        assert plan(G.case_hyper(bc), [bc[5]])[5] == 1 and cid not in G.CASE_IDS, cid


@pytest.mark.parametrize("name,how,k", POP_CASES, ids=[f"{n}-{h}" for n, h, _ in POP_CASES])
def test_population_cases_calibration_margin(name, how, k):
    """The transformed candidate of each population case: the float32 oracle under a quarter of every tau on steps 1..3."""
    from tests.oracle32_runs import oracle_steps
    inp = GT.schedule_inputs(name, "shared")
    hp, conf = inp["hp"], inp["confs"][k]
    assert how != "dead" or int(conf[0][2]) == 1
    p = IE.edge_params(inp["p0s"][k], hp, conf, how)
    if how == "deadrelu":
        assert_first_cell_column_is_dead(conf, hp, p, GT.batch_of(inp["t"], inp["order"], hp.B, 1)[0], f"{name} {how}")
        if name == "chain_split":
            assert not hp.alphas and 113 <= hp.R <= 128 and hp.B <= 16
    r = oracle_steps(conf, hp, p, inp["t"], inp["order"], inp["etas"], inp["seeds"][k], (1, 2, 3), GT.TAUS, f"{name} {how}")
    for q, tau in GT.TAUS.items():
        assert r[q] * 4.0 <= tau, (name, how, q, r[q], tau)
    assert r["count"] == 0.0


# ------------------------------------------------------------------------------------------------ mutations
def forward32(params, conf, hp, feats, train, seed=0, step=0, masks=None, mut=""):
    """O.forward restated so that the batch statistics are in reach: mut = 'var_e2' (the batch variance as E[a^2] - mean^2 in
    float32, clamped at 0), 'rstd_clamp' / 'var_floor' (rstd from a variance clamped to at least 1e-3 / 1e-6), 'var_clamp5' (the
    batch variance itself clamped to at least 1e-5: rstd and the running variance both read it), 'rstd_var0' (a var == 0 shortcut:
    xhat = 0 without eps), 'mean_bf16' (the batch mean stored in bfloat16), 'gate_bn' (the first cell's ReLU gate read from the
    BatchNorm output instead of the activation).  mut = '' is O.forward bit for bit."""
    cache = {"cells": [], "conf": conf}
    out = None
    for i in range(len(conf)):
        s = feats[f"s{int(conf[i][0])}"].astype(F32, copy=False)
        v = feats[f"v{int(conf[i][1])}"].astype(F32, copy=False)
        c = {}
        if hp.alphas:
            sg = O._sigmoid(params[f"alphas.{i}.alpha_x"])[0]
            c.update(sg=sg, s_raw=s, v_raw=v)
            s, v = s * sg, v * (F32(1.0) - sg)
        x = np.concatenate([s, v] if i == 0 else [s, v, out], axis=1)
        y = (x @ params[f"fusion_layers.{i}.0.weight"].T + params[f"fusion_layers.{i}.0.bias"]).astype(F32)
        nl = int(conf[i][2])
        a = O._act(y, nl)
        c.update(x=x, y=y, a=a, nl=nl)
        z = a
        if hp.bn:
            g, be = params[f"fusion_layers.{i}.2.weight"], params[f"fusion_layers.{i}.2.bias"]
            if train:
                mu = a.mean(axis=0, dtype=F32)
                if mut == "mean_bf16":
                    mu = O.bf16_round(mu)
                var = ((a - mu) ** 2).mean(axis=0, dtype=F32)
                if mut == "var_clamp5":
                    var = np.maximum(var, F32(1e-5))
                if mut == "var_e2":
                    var = np.maximum((a * a).mean(axis=0, dtype=F32) - mu * mu, F32(0)).astype(F32)
                vr = np.maximum(var, F32({"rstd_clamp": 1e-3, "var_floor": 1e-6}[mut])) if mut in ("rstd_clamp", "var_floor") else var
                rstd = (F32(1.0) / np.sqrt(vr + F32(hp.bn_eps))).astype(F32)
                if mut == "rstd_var0":
                    rstd = np.where(var == 0, F32(0), rstd)
                xhat = ((a - mu) * rstd).astype(F32)
                c.update(mu=mu, var=var, rstd=rstd, xhat=xhat, n=a.shape[0])
            else:
                rm, rv = params[f"fusion_layers.{i}.2.running_mean"], params[f"fusion_layers.{i}.2.running_var"]
                xhat = ((a - rm) / np.sqrt(rv + F32(hp.bn_eps))).astype(F32)
            z = (xhat * g + be).astype(F32)
            if mut == "gate_bn" and train and i == 0 and nl == 0:
                c["a"] = z          # (O.backward gates a ReLU on the cached activation)
        if hp.use_dropout and train:
            keep = masks[i] if masks is not None else O.dropout_keep(seed, step, i, z.shape[0], hp.R, hp.drpt)
            scale = F32(1.0 / (1.0 - hp.drpt))
            c.update(keep=keep, scale=scale)
            z = np.where(keep, z * scale, F32(0)).astype(F32)
        out = z
        cache["cells"].append(c)
    logits = (out @ params["central_classifier.weight"].T + params["central_classifier.bias"]).astype(F32)
    cache["out"] = out
    return logits, cache


def ce_loss_mut(mut, C_pad_logit=F32(0)):
    """O.ce_loss with a softmax that goes wrong only on large logits: 'no_rowmax' (no row-max subtraction), 'pad_in_softmax' (the
    first padded class column, logit 0, joins the maximum and the sum), 'pad_in_max' (it joins the maximum only)."""
    def ce_loss(logits, labels):
        Bn = logits.shape[0]
        with np.errstate(all="ignore"):
            mx = logits.max(axis=1, keepdims=True)
            if mut == "no_rowmax":
                mx = np.zeros_like(mx)
            if mut in ("pad_in_softmax", "pad_in_max"):
                mx = np.maximum(mx, C_pad_logit)
            ex = np.exp(logits - mx, dtype=F32)
            se = ex.sum(axis=1, keepdims=True, dtype=F32)
            if mut == "pad_in_softmax":
                se = (se + np.exp(C_pad_logit - mx, dtype=F32)).astype(F32)
            logp = (logits - mx - np.log(se, dtype=F32)).astype(F32)
            loss = F32(-logp[np.arange(Bn), labels].mean(dtype=F32))
            d = (ex / se).astype(F32)
            d[np.arange(Bn), labels] -= F32(1.0)
            d = (d / F32(Bn)).astype(F32)
        return loss, d, O.predict(logits)
    return ce_loss


def sigmoid_naive(x):
    """O._sigmoid as e^x / (1 + e^x): the same value to rounding while e^x is finite, inf / inf from x = 88.8 on."""
    with np.errstate(all="ignore"):
        e = np.exp(x, dtype=F32)
        return (e / (F32(1.0) + e)).astype(F32)


def patched(mut):
    if not mut:
        return contextlib.nullcontext()
    if mut == "sig_naive":
        return mock.patch.object(O, "_sigmoid", sigmoid_naive)
    if mut in ("var_e2", "rstd_clamp", "var_floor", "var_clamp5", "rstd_var0", "mean_bf16", "gate_bn"):
        return mock.patch.object(O, "forward", lambda *a, **kw: forward32(*a, mut=mut, **kw))
    return mock.patch.object(O, "ce_loss", ce_loss_mut(mut))


def entry_index(cid, how):
    return next(i for i, e in enumerate(INPUT_CASES) if e[0] == cid and e[1] == how)


def train_ratios(cid, how, mut, extra_edit=None):
    """Steps 1..3 of the float32 oracle with mutation `mut` on INPUT_CASES' (cid, how) entry (how None: the base case's
    untransformed inputs, same seed)."""
    i = next(j for j, e in enumerate(INPUT_CASES) if e[0] == cid and (how is None or e[1] == how))
    dtype = INPUT_CASES[i][2]
    edit = make_edit(how) if how else None
    if extra_edit is not None:
        inner = edit
        edit = (lambda conf, hp, p0, t, dt: extra_edit(conf, hp, *inner(conf, hp, p0, t, dt), dt))
    with patched(mut):
        return oracle_train_steps(base_case(cid), dtype, seed=entry_seed(i), edit=edit)


def train_ratios_at(i, transformed, mut):
    """Steps 1..3 of the float32 oracle with mutation `mut` on INPUT_CASES[i] as the GPU test judges it (its seed, table dtype
    and batch_sum_term), or, transformed False, on the same draw untransformed and judged without the term, as the files that run
    the untransformed inputs judge them.  A wide entry: the case's own cells (candidate 0)."""
    cid, how, dtype = INPUT_CASES[i]
    edit = make_edit(how) if transformed else None
    flag = transformed and entry_flag(i)
    with patched(mut):
        if is_wide(cid):
            case = base_case(cid, dtype)
            return oracle_train_steps(GW.base_case(case), dtype, seed=GW.SEED0 + GW.WIDE_IDS.index(cid), edit=edit, batch_sum_term=flag)
        return oracle_train_steps(base_case(cid), dtype, seed=entry_seed(i), edit=edit, batch_sum_term=flag)


def over(r):
    return {q: round(r[q], 2) for q, tau in GT.TAUS.items() if not r[q] <= tau}


def under(r):
    return all(r[q] <= tau for q, tau in GT.TAUS.items()) and r["count"] == 0.0


def test_forward32_is_the_oracle():
    case = base_case("r16b")
    hp = G.case_hyper(case)
    conf, p = G.case_params(case, hp, 9)
    f = G.feats_of(G.case_table(case, hp, hp.B, 9, "float32"))
    for train in (False, True):
        a, ca = O.forward({k: v.copy() for k, v in p.items()}, conf, hp, f, train, seed=4, step=3)
        b, cb = forward32(p, conf, hp, f, train, seed=4, step=3)
        assert np.array_equal(a, b)
        if train:
            assert all(np.array_equal(x["xhat"], y["xhat"]) and np.array_equal(x["var"], y["var"]) for x, y in zip(ca["cells"], cb["cells"]))
    lg = (3 * np.random.default_rng(0).standard_normal((20, 60))).astype(F32)
    lab = np.arange(20) % 60
    for x, y in zip(O.ce_loss(lg, lab), ce_loss_mut("")(lg, lab)):
        assert np.array_equal(x, y)


# (mutation, base case, transform it must fail on)
TRAIN_MUTATIONS = [
    ("no_rowmax", "r33a", "bighead"), ("no_rowmax", "r256a", "bighead"),
    ("var_e2", "r32a", "offset"), ("var_e2", "r16b", "dead"),
    ("var_floor", "r32a", "tiny"),
    ("var_e2", "r65a", "dup"), ("sig_naive", "r33a", "scaled"),
]


@pytest.mark.parametrize("mut,cid,how", TRAIN_MUTATIONS, ids=[f"{m}-{c}-{h}" for m, c, h in TRAIN_MUTATIONS])
def test_value_mutations_of_a_train_step(mut, cid, how):
    """A train step that is wrong only on such values: under every tau on the base case's untransformed inputs (so no earlier
    test sees it), over a tau on the transformed ones.  Worst ratios of the float32 oracle with the mutation, old inputs -> new
    inputs (quantities as in GT.TAUS; the test prints them with -s):

      no_rowmax  softmax and CE without the row-max subtraction
                 r33a  old m 0.68 w 3.58 loss 0.002    bighead: exp overflows, m / v / w / loss non-finite
                 r256a old m 0.71 w 3.65 runstat 0.83  bighead: the same, runstat too
      var_e2     batch variance as E[a^2] - mean^2 in float32 (clamped at 0)
                 r32a  old runstat 0.72                offset: runstat 31.8
                 r16b  old runstat 0.82                dead: runstat 4.37 (a sigmoid column at 1: E[a^2] - mean^2 is rounding of 1)
                 r65a  old runstat 0.65                dup: runstat 9.81 (identical rows: the true variance is 0, E[a^2] - mean^2
                                                       is the rounding of a^2; r16a-dup and r129a-dup do not see it)
      sig_naive  sigmoid as e^x / (1 + e^x)  (for 'scaled', which the softmax mutation cannot reach)
                 r33a  old m 0.68 w 3.33 loss 0.002    scaled: the first cell's sigmoid sees pre-activations above 88.8, e^x is
                                                       inf and inf / inf poisons m / v / w and the count (r65a- and r16a-scaled,
                                                       whose sigmoid cells sit behind a BatchNorm, do not see it)
      var_floor  rstd from max(var, 1e-6)  (replaces the clamp at 1e-3, see test_recorded_findings_about_the_asked_mutations)
                 r32a  old runstat 0.74 (bit-identical to unmutated: no old variance is below 1e-6)
                                                       tiny: runstat 33.4 (first-cell variances of about 1e-8)
    """
    old = train_ratios(cid, None, mut)
    new = train_ratios(cid, how, mut)
    print(f"\n{mut} {cid}: old {({q: round(v, 3) for q, v in old.items()})}\n   {how}: {({q: round(v, 3) for q, v in new.items()})}")
    assert under(old), (mut, cid, "fails on the untransformed inputs already", old)
    assert over(new), (mut, cid, how, new)


def test_recorded_findings_about_the_asked_mutations():
    """Two of the mutations as first asked for do not separate old from new inputs; measured with the float32 oracle:

    * rstd from a variance clamped to at least 1e-3, against 'dup': it already FAILS on the untransformed inputs (r65a: runstat
      84, r16a: runstat 928, m 63 — old first-cell variances go down to 4e-4), and 'dup' cannot see it at all on r65a (m 0.92,
      runstat 0.80): with identical rows xhat is 0, and every weight gradient behind a BatchNorm is x0 (x) sum_rows(d_z - mean d_z),
      which is 0 whatever rstd is.  Replaced by the floor at 1e-6 against 'tiny', and for 'dup' itself by var_e2 on r65a (above):
      what identical rows expose is the variance, through the running statistics, not rstd.
    * softmax without the row-max subtraction, against 'scaled': logits reach 40, exp(40) = 2.4e17 is an ordinary float32 and
      the quotient is as accurate as with the subtraction (r33a: m 0.68 -> 0.68, r16a: m 0.61 -> 0.59).  It is asserted against
      'bighead' only; 'scaled' would need logits above 88.  What 'scaled' does expose is an exp of a large PRE-ACTIVATION:
      sig_naive on r33a (above)."""
    assert not under(train_ratios("r65a", None, "rstd_clamp"))
    assert under(train_ratios("r65a", "dup", "rstd_clamp"))
    assert under(train_ratios("r33a", "scaled", "no_rowmax"))


# (mutation, base case, transform): the entries that split 'dead' in two, each judged as the GPU test judges it
SPLIT_MUTATIONS = [("var_e2", c, "bigmean") for c in ("l16c", "r16a", "r32a", "r256a", "w65")] + [("var_clamp5", "r16a", "deadrelu")]


@pytest.mark.parametrize("mut,cid,how", SPLIT_MUTATIONS, ids=[f"{m}-{c}-{h}" for m, c, h in SPLIT_MUTATIONS])
def test_value_mutations_on_the_split_dead_transforms(mut, cid, how):
    """As test_value_mutations_of_a_train_step, on the entry's own draw: under every tau on the untransformed inputs judged
    without the batch-sum term, over a tau on the transformed ones judged as the GPU test judges them ('bigmean': with the term).
    Worst ratios of the mutated float32 oracle, old -> new (the test prints them with -s):

      var_e2      batch variance as E[a^2] - mean^2: a column of values near 64 with a spread of 1 loses the variance to the rounding
                  of 4096.  The term loosens M_var (through M_mu and by (n - 1) var), and the mutation still leaves tau by x5 .. x28:
                  l16c old runstat 0.69 -> bigmean 19.4    r16a 0.70 -> 22.6    r32a 0.83 -> 111.4    r256a 0.84 -> 79.4
                  w65 (the wide path, 64 rows) 0.69 -> 23.0
      var_clamp5  the batch variance clamped to at least 1e-5, for rstd and for the running variance alike
                  r16a old runstat 3.13, loss 0.34 (inside tau 4 and 1, though not by the x4 of an unmutated oracle: the draw has a
                  variance below 1e-5 of its own in one step) -> deadrelu 35.0 (a dead column's running variance must move by
                  exactly the momentum step towards 0; the clamp leaves 1e-5 n / (n - 1) of it)
    """
    i = entry_index(cid, how)
    old = train_ratios_at(i, False, mut)
    new = train_ratios_at(i, True, mut)
    print(f"\n{mut} {INPUT_IDS[i]}: old {({q: round(v, 3) for q, v in old.items()})}\n   new: {({q: round(v, 3) for q, v in new.items()})}")
    assert under(old), (mut, cid, "fails on the untransformed inputs already", old)
    assert under(train_ratios_at(i, True, "")), (cid, how, "the unmutated oracle")
    assert over(new), (mut, cid, how, new)


def test_recorded_findings_about_the_split_dead_mutations():
    """Mutations proposed for 'deadrelu', 'bigmean' and the wide 'dup' that do not separate old from new inputs, measured with the
    float32 oracle on the entries' own draws:

    * the batch mean stored in bfloat16: it FAILS on the untransformed inputs of every base (runstat 1900 .. 14000: 2^-9 of a mean
      against a bound of a few 2^-24), so nothing about 'bigmean' is needed to see it; with the term it still fails there (1700 ..
      6300), i.e. the term costs no power against an error of that size;
    * a var == 0 shortcut that sets xhat = 0 without eps: invisible on 'deadrelu' and on the wide 'dup' (and everywhere else).
      With a zero-variance column a - mean is exactly 0, so xhat is 0 whatever rstd is, and the backward of a dead ReLU column is
      gated off; rstd of such a column reaches no output.  What a zero-variance column does pin is the variance itself, through
      the running variance: var_clamp5 above;
    * var_clamp5 on the other 'deadrelu' bases (l16c, r32a, r256a, w65): it fails on their UNTRANSFORMED draws already (runstat 15
      .. 38): a variance below 1e-5 occurs by itself in their three steps (the first 16 rows of r256a's table leave ten first-cell ReLU
      columns at 0 on every row), so against this mutation those entries add dead columns 0, 3, 6, .. of the FIRST cell on
      every batch and schedule, not a new kind of value; r16a's draw stays inside tau;
    * the first cell's ReLU gate read from the BatchNorm output: fails on the untransformed inputs of every base (m 26 .. 1e15:
      the sign of (a - mean) rstd gamma + beta has little to do with the sign of the pre-activation);
    * var_e2 on 'deadrelu' (E[0] - 0^2 is exact) and on the wide 'dup' (w65: activations of about 1, the rounding of a^2 stays
      inside the running variance's absolute allowance; r65a-dup above sees it): under every tau."""
    dr, bm = entry_index("r16a", "deadrelu"), entry_index("r32a", "bigmean")
    wd = next(i for i, e in enumerate(INPUT_CASES) if e[0] == "w65" and e[1] == "dup")
    assert not under(train_ratios_at(bm, False, "mean_bf16")) and not under(train_ratios_at(bm, True, "mean_bf16"))
    for i in (dr, wd):
        assert under(train_ratios_at(i, True, "rstd_var0")) and under(train_ratios_at(i, True, "var_e2"))
    for cid in ("l16c", "r32a", "r256a", "w65"):
        assert not under(train_ratios_at(entry_index(cid, "deadrelu"), False, "var_clamp5")), cid
    assert not under(train_ratios_at(dr, False, "gate_bn")) and not under(train_ratios_at(bm, False, "gate_bn"))


# ------------------------------------------------------------------------------------------------ what the batch-sum term costs
def batch_sum_term_cost():
    """M with batch_sum_term over M without it, elementwise, on the UNTRANSFORMED base draw of every new entry (the first train
    batch, dropout step 3, an arbitrary dL/dlogits): {quantity: ratios of all elements of all draws}."""
    acc = {"forward_train": [], "gradients": [], "running_mean": [], "running_var": []}
    for i, (cid, how, dtype) in enumerate(INPUT_CASES):
        if how not in ("deadrelu", "bigmean") and not entry_flag(i):
            continue
        case, seed = (GW.base_case(base_case(cid, dtype)), GW.SEED0 + GW.WIDE_IDS.index(cid)) if is_wide(cid) else (base_case(cid), entry_seed(i))
        hp = G.case_hyper(case)
        conf, p = G.case_params(case, hp, seed)
        f = G.feats_of(G.case_table(case, hp, G.N_EVAL, seed, dtype), 0, hp.B)
        dl = (np.random.default_rng(seed).standard_normal((hp.B, hp.C)) / hp.B).astype(F32)
        m = []
        for flag in (False, True):
            _, Ml, cache = R64.forward(p, conf, hp, f, True, seed=seed, step=3, batch_sum_term=flag)
            m.append((Ml, R64.backward(p, hp, cache, dl)[1], R64.running_stats(p, hp, cache)[1]))
        (Ml0, MG0, Mr0), (Ml1, MG1, Mr1) = m
        acc["forward_train"].append((Ml1 / Ml0).ravel())
        for k in MG0:       # (an element without any magnitude, a dropped unit's, has none with the term either)
            assert not MG1[k][MG0[k] == 0].any(), (INPUT_IDS[i], k)
            acc["gradients"].append((MG1[k][MG0[k] > 0] / MG0[k][MG0[k] > 0]).ravel())
        acc["running_mean"] += [(Mr1[k] / Mr0[k]).ravel() for k in Mr0 if k.endswith("mean")]
        assert all((Mr1[k] <= hp.B * Mr0[k]).all() for k in Mr0 if k.endswith("mean")), INPUT_IDS[i]
        acc["running_var"] += [(Mr1[k] / Mr0[k]).ravel() for k in Mr0 if k.endswith("var")]
    return {q: np.concatenate(v) for q, v in acc.items()}


def test_batch_sum_term_only_loosens_and_by_at_most_n():
    """The term only adds to M (no comparison tightens), and the running mean's M grows by less than the factor n: M_a >= |a|
    for every nonlinearity, so (n - 1) mean|a| <= (n - 1) mean(M_a).  Measured, M with the term / M without, over the eleven
    untransformed base draws (what a flagged comparison can still see is tau times these; the test prints them with -s):

      quantity        worst      median
      running mean    5.3        1.45
      running var     2.6        1.34
      forward_train   2.9        1.44
      gradients       9.5e4      1.44     (the worst: fusion-bias gradients under BatchNorm, which cancel to a round-off-sized M)

    An error of a few 2^-24 of a column's mean or variance, which the unflagged rule catches, can pass a flagged one; one of 2^-9 of
    the mean or of the whole variance cannot (mean_bf16, var_e2, var_clamp5 above)."""
    r = batch_sum_term_cost()
    for q, a in r.items():
        print(f"\nbatch_sum_term M ratio {q}: worst {a.max():.4g} median {np.median(a):.3g}")
        assert np.isfinite(a).all() and (a >= 1.0).all(), q          # (the factor n on the running mean: asserted per draw)


def big_shifted_head(conf, hp, p, t, dtype):
    """'bighead', then the head bias shifted by -300: every valid logit is negative."""
    q, t = make_edit("bighead")(conf, hp, p, t, dtype)
    q["central_classifier.bias"] = (q["central_classifier.bias"] - F32(300)).astype(F32)
    return q, t


@pytest.mark.parametrize("cid", ["r33a", "r256a"])       # C = 2 (no BatchNorm, multitask) and C = 17 (BatchNorm)
def test_mutation_padded_class_column_joins_the_row_maximum(cid):
    """The mutation as first asked for — class column C, the first padded one, joins the softmax with logit 0 — already fails on
    the untransformed inputs (their logits are below 1, so a further class at 0 takes a share of every row: r33a m 32446, v 659361,
    loss 27710; r256a loss 1.96), which this test asserts; it is replaced by the padded column joining only the row MAXIMUM.  On
    the old inputs that moves the maximum by less than 1 and changes nothing beyond rounding (under every tau); with 'onelabel' +
    'bighead' and the head bias shifted by -300 every valid logit is negative, the maximum is the padded 0, every exp underflows
    and loss, m, v and w are non-finite.  (On r16b, four BatchNorm cells, neither form is seen on the old inputs, whatever the
    values: ref64's train-mode magnitude has grown to 2e7 by the head.  DESIGN.md section 8.)"""
    assert not under(train_ratios(cid, None, "pad_in_softmax"))
    old = train_ratios(cid, None, "pad_in_max")
    assert under(old), old
    ok = train_ratios(cid, "onelabel", "", extra_edit=big_shifted_head)
    assert under(ok), ok            # (the shifted big head alone is inside every tau)
    new = train_ratios(cid, "onelabel", "pad_in_max", extra_edit=big_shifted_head)
    assert over(new) and not np.isfinite(new["loss"]), new


def eval_pair(cid, how):
    i = entry_index(cid, how)
    dtype = INPUT_CASES[i][2]
    case = base_case(cid)
    hp = G.case_hyper(case)
    conf, p0 = G.case_params(case, hp, entry_seed(i))
    t0 = G.case_table(case, hp, G.N_EVAL, entry_seed(i), dtype)
    p, t = make_edit(how)(conf, hp, p0, t0, dtype)
    return hp, conf, p0, t0, p, t


def f1_fixed_empty_scores_one(logits, z, th):
    """O.f1_samples_fixed with a row of empty prediction and empty target scored 1 instead of 0."""
    pr = O._sigmoid(logits.astype(F32)) > F32(th)
    empty = int(((pr.sum(1) + (z > 0.5).sum(1)) == 0).sum())
    return O.f1_samples_fixed(logits, z, th) + (empty << 32)


@pytest.mark.parametrize("cid", ["r17a", "r80a"])
def test_mutation_f1_of_an_empty_row_scored_one(cid):
    """Old inputs: no row has an empty target set (0.8^C), the mutated sum equals the oracle's and lies in [lo, hi].  'mlrows':
    row 0 has no target and predicts nothing; the mutated sum is 2^32 above hi."""
    hp, conf, p0, t0, p, t = eval_pair(cid, "mlrows")
    for params, tab, inside in ((p0, t0, True), (p, t, False)):
        f = G.feats_of(tab)
        lg, Ml, _ = R64.forward(params, conf, hp, f, False)
        _, _, lo, hi = R64.dev_stats(lg, Ml, hp, G.TAU_LOGITS, z=tab["multilabel"], pos_weight=G.pos_weight(hp))
        lg32 = O.forward({k: v.copy() for k, v in params.items()}, conf, hp, f, False)[0]
        assert lo <= O.f1_samples_fixed(lg32, tab["multilabel"], hp.f1_threshold) <= hi
        bad = f1_fixed_empty_scores_one(lg32, tab["multilabel"], hp.f1_threshold)
        assert (lo <= bad <= hi) == inside, (cid, inside, lo, bad, hi)
        if not inside:
            assert not (tab["multilabel"][0] > 0.5).any() and bad - hi >= (1 << 32) - 2 * len(lg)


@pytest.mark.parametrize("cid", ["r16b", "r80a", "r33a"])
def test_mutation_negative_zero_read_as_a_value(cid):
    """-0.0 taps read as 2.0 (the sign bit of a 16-bit value taken for a payload bit).  The old inputs hold no -0.0: the mutated
    read is the same read (ratio unchanged, under tau / 4).  On 'sparse' every seventh column is -0.0 and the logits leave tau by
    orders of magnitude."""
    hp, conf, p0, t0, p, t = eval_pair(cid, "sparse")
    for params, tab, fails in ((p0, t0, False), (p, t, True)):
        f = G.feats_of(tab)
        lg, Ml, _ = R64.forward(params, conf, hp, f, False)
        f2 = {k: (np.where((v == 0) & np.signbit(v), F32(2.0), v) if IE.is_tap(k) else v) for k, v in f.items()}
        assert any(np.signbit(v[v == 0]).any() for k, v in f.items() if IE.is_tap(k)) == fails
        r = R64.worst_ratio(O.forward({k: v.copy() for k, v in params.items()}, conf, hp, f2, False)[0], lg, Ml)[0]
        print(f"\nnegzero {cid} {'sparse' if fails else 'old'}: {r:.3g}")
        assert (r > G.TAU_LOGITS) == fails and (fails or r * 4 <= G.TAU_LOGITS), (cid, fails, r)


def test_rne_bf16_reference_of_the_pool_test():
    """The rounding reference of tests/test_gpu_pool_ref64.py: float64 -> bf16 in one rounding, ties to even."""
    from tests.pool_cases import rne16, rne_bf16
    one, ulp = 1.0, 2.0 ** -7
    assert rne_bf16(one + 0.5 * ulp) == one and rne_bf16(one + 1.5 * ulp) == one + 2 * ulp
    assert rne_bf16(one + 0.5 * ulp + 2.0 ** -40) == one + ulp          # (a float32 step in between would have made it a tie)
    assert rne_bf16(-(one + 0.5 * ulp)) == -one and rne_bf16(0.0) == 0.0
    x = np.random.default_rng(0).standard_normal(4096).astype(F32)
    assert np.array_equal(rne_bf16(x.astype(np.float64)), O.bf16_round(x).astype(np.float64))
    assert rne16(1.0 + 2.0 ** -11, "float16") == 1.0 and rne16(1.0 + 3 * 2.0 ** -11, "float16") == 1.0 + 2.0 ** -9
    assert rne16(1.0 + 2.0 ** -11 + 2.0 ** -40, "float16") == 1.0 + 2.0 ** -10
