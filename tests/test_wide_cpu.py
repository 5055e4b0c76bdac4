"""CPU checks for the wide path (tests/test_gpu_wide_ref64.py judges the kernels on the GPU):

* calibration: on every wide case shape the float32 oracle stays under a quarter of each tau, single passes and train steps;
* accepted shapes are untouched: the layout query answers for every case of test_gpu_ref64.py::CASES and for the BASELINE
  geometries exactly what the library answered before the wide path existed (tuples recorded from a build of the parent commit),
  with the wide bit clear;
* the layout query answers for every wide case, without a device;
* three ways a step that walks the batch in pieces goes wrong each exceed their tau against ref64."""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import train_cases as GT
from tests import wide_cases as GW
from tests.helpers import CONFS, engine_hyper
from tests.oracle32_runs import oracle_train_steps
from tests.wide_oracle32 import F32, PINNED_BASELINE, PINNED_CASES, wide_oracle_case
from tests.wide_plans import baseline_geometries, plan


def wide_ratios(case):
    worst = {}
    for k, cells in enumerate(GW.case_confs(case)):
        r = wide_oracle_case(case, k, cells)
        r.update({"train_" + q: v for q, v in oracle_train_steps(GW.base_case(case, cells), case[9],
                                                                   seed=GW.SEED0 + GW.WIDE_IDS.index(case[0])).items()})
        worst = {q: max(worst.get(q, 0.0), v) for q, v in r.items()}
    return worst


@pytest.mark.parametrize("case", GW.WIDE_CASES, ids=GW.WIDE_IDS)
def test_wide_float32_oracle_calibration_margin(case):
    """Every candidate configuration of the case, the case's table dtype: single passes and steps 1..3 stay under a quarter of
    the tau the GPU test applies to the case (GW.case_taus: the project's taus, or the case's own where they are recorded)."""
    r = wide_ratios(case)
    single, train = GW.case_taus(case[0])
    for q, tau in single.items():
        assert r.get(q, 0.0) * 4.0 <= tau, (case[0], q, r[q], tau)
    for q, tau in train.items():
        assert r["train_" + q] * 4.0 <= tau, (case[0], q, r["train_" + q], tau)
    assert r["train_count"] == 0.0, case[0]


def test_wide_cases_cover_the_design():
    why = {c[0]: GW.legacy_refusal(c, GW.case_confs(c)) for c in GW.WIDE_CASES}
    assert all(why.values()) and set(why.values()) == {"B>64", "C_padded", "lds"}, why
    for wset in (G.W_A, G.W_B, G.W_C):
        assert sum(c[4] is wset for c in GW.WIDE_CASES) >= 3
    for dt in G.DTYPES:
        assert sum(c[9] == dt for c in GW.WIDE_CASES) >= 3
    for c in GW.WIDE_CASES:
        confs = GW.case_confs(c)
        assert len({len(x) for x in confs}) == GW.K == len(confs), c[0]
        assert 2 <= GT.ragged_rows(c[3]) <= c[3] - 1, c[0]
        assert all(c[4]["s"][cell[0]] > 0 and c[4]["v"][cell[1]] > 0 for conf in confs for cell in conf), c[0]


def test_accepted_shapes_keep_their_plan():
    assert set(PINNED_CASES) == set(G.CASE_IDS)
    for case in G.CASES:
        got = plan(G.case_hyper(case), [case[5]])
        assert got[:6] == PINNED_CASES[case[0]] and got[6] == 0, (case[0], got)
    geos = baseline_geometries()
    assert set(PINNED_BASELINE) == {g[0] for g in geos}
    for name, hp, confs in geos:
        got = plan(hp, confs)
        assert got[:6] == PINNED_BASELINE[name] and got[6] == 0, (name, got)


@pytest.mark.parametrize("case", GW.WIDE_CASES, ids=GW.WIDE_IDS)
def test_plan_query_answers_for_wide_cases(case):
    """No device is needed (none is touched): wide, launch per phase, nothing resident, feature chunks of at most 128 columns."""
    got = plan(G.case_hyper(GW.base_case(case)), GW.case_confs(case))
    assert got[6] == 1 and got[:4] == (0, 0, 0, 1) and got[5] == 0 and 16 <= got[4] <= 128, (case[0], got)


def test_limits_that_remain():
    from mfas_amd.engine import plan_population
    for bad in (dict(B=129), dict(B=1), dict(R=513), dict(C=257)):
        hp = O.Hyper(**{**dict(R=16, C=60, B=20, bn=True, drpt=0.5), **bad})
        with pytest.raises(RuntimeError):
            plan_population(engine_hyper(hp), [np.array(CONFS["l1"])], "cuda:0", 0)


# ------------------------------------------------------------------------------------------------ mutations of a wide step
SLICE = 64      # batch rows a wide sweep unit stages at a time


def forward_train32(params, conf, hp, feats, seed, step, mut=""):
    """O.forward in train mode, restated so that the places where a batch walked in pieces can go wrong are in reach:
    mut = 'var_per_slice' (the BN variance of each 64-row slice instead of the batch's), 'inv_bp' (1 / nvalid taken from the padded
    batch), 'drop_row_in_slice' (dropout indexed by the row inside its slice).  mut = '' is O.forward bit for bit."""
    out, n = None, len(feats["s0"])
    npad = -(-n // 16) * 16
    for i in range(len(conf)):
        s = feats[f"s{int(conf[i][0])}"].astype(F32, copy=False)
        v = feats[f"v{int(conf[i][1])}"].astype(F32, copy=False)
        x = np.concatenate([s, v] if i == 0 else [s, v, out], axis=1)
        y = (x @ params[f"fusion_layers.{i}.0.weight"].T + params[f"fusion_layers.{i}.0.bias"]).astype(F32)
        z = a = O._act(y, int(conf[i][2]))
        if hp.bn:
            g, be = params[f"fusion_layers.{i}.2.weight"], params[f"fusion_layers.{i}.2.bias"]
            mu = a.mean(axis=0, dtype=F32)
            d2 = (a - mu) ** 2
            var = d2.mean(axis=0, dtype=F32)
            if mut == "inv_bp":
                mu = (a.sum(axis=0, dtype=F32) / F32(npad)).astype(F32)
                var = (((a - mu) ** 2).sum(axis=0, dtype=F32) / F32(npad)).astype(F32)
            if mut == "var_per_slice":
                var = np.concatenate([np.broadcast_to(d2[r:r + SLICE].mean(axis=0, dtype=F32), d2[r:r + SLICE].shape)
                                      for r in range(0, n, SLICE)])
            rstd = (F32(1.0) / np.sqrt(var + F32(hp.bn_eps))).astype(F32)
            z = (((a - mu) * rstd).astype(F32) * g + be).astype(F32)
        if hp.use_dropout:
            keep = O.dropout_keep(seed, step, i, n, hp.R, hp.drpt)
            if mut == "drop_row_in_slice":
                keep = np.concatenate([keep[:min(SLICE, n - r)] for r in range(0, n, SLICE)])
            z = np.where(keep, z * F32(1.0 / (1.0 - hp.drpt)), F32(0)).astype(F32)
        out = z
    return (out @ params["central_classifier.weight"].T + params["central_classifier.bias"]).astype(F32)


@pytest.mark.parametrize("mut", ["var_per_slice", "inv_bp", "drop_row_in_slice"])
def test_wide_step_mutations(mut):
    case = GW.base_case(GW.WIDE_CASES[GW.WIDE_IDS.index("wb100")])      # B = 100: slices of 64 + 36 rows, 112 padded rows
    hp = G.case_hyper(case)
    hp.drpt = 0.5
    conf, p = G.case_params(case, hp, 9)
    f = G.feats_of(G.case_table(case, hp, hp.B, 9, "float32"))
    lg, Ml, _ = R64.forward(p, conf, hp, f, True, seed=4, step=3)
    ok = forward_train32(p, conf, hp, f, 4, 3)
    assert np.array_equal(ok, O.forward({k: v.copy() for k, v in p.items()}, conf, hp, f, True, seed=4, step=3)[0])
    R64.assert_close64(ok, lg, Ml, G.TAU_LOGITS / 4, "unmutated")
    with pytest.raises(AssertionError):
        R64.assert_close64(forward_train32(p, conf, hp, f, 4, 3, mut), lg, Ml, G.TAU_LOGITS, mut)
