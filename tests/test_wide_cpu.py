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
from tests import test_gpu_ref64 as G
from tests import test_gpu_train_ref64 as GT
from tests import test_gpu_wide_ref64 as GW
from tests.helpers import CONFS, engine_hyper
from tests.test_ref64_cpu import oracle_train_steps

F32 = np.float32


# ------------------------------------------------------------------------------------------------ calibration
def wide_oracle_case(case, k, cells, edit=None, batch_sum_term=False):
    """The float32 oracle and ref64 on the inputs test_gpu_wide_ref64 gives the engine for candidate k: worst ratio per quantity
    (test_ref64_cpu.py::oracle_case for a batch that may be larger than the 83-row dev table; edit and batch_sum_term as there)."""
    bc, dtype = GW.base_case(case, cells), case[9]
    hp = G.case_hyper(bc)
    seed = GW.SEED0 + GW.WIDE_IDS.index(case[0])
    conf, p0 = G.case_params(bc, hp, seed + 10 * k)
    t = G.case_table(bc, hp, G.N_EVAL, seed, dtype)
    tb = t if hp.B <= G.N_EVAL else G.case_table(bc, hp, hp.B, seed + 5, dtype)
    if edit is not None:
        p_in = p0
        p0, t = edit(conf, hp, p_in, t, dtype)
        tb = t if hp.B <= G.N_EVAL else edit(conf, hp, p_in, tb, dtype)[1]
    out = {}
    f = G.feats_of(t)
    lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
    out["forward"] = R64.worst_ratio(O.forward({kk: v.copy() for kk, v in p0.items()}, conf, hp, f, False)[0], lg, Ml)[0]
    for nb in (hp.B, hp.B - 3):
        f = G.feats_of(tb, 0, nb)
        p32 = {kk: v.copy() for kk, v in p0.items()}
        lg32, cache32 = O.forward(p32, conf, hp, f, True, seed=seed + 3 * k, step=3)
        lg, Ml, cache = R64.forward(p0, conf, hp, f, True, seed=seed + 3 * k, step=3, batch_sum_term=batch_sum_term)
        out["forward_train"] = max(out.get("forward_train", 0.0), R64.worst_ratio(lg32, lg, Ml)[0])
        rng = np.random.default_rng(seed + k)
        dl = (rng.standard_normal((nb, hp.C)) / nb).astype(F32)
        dl[rng.random((nb, hp.C)) < 0.1] *= F32(1e-3)
        g32 = O.backward(p32, hp, cache32, dl)
        G64, MG = R64.backward(p0, hp, cache, dl)
        out["backward"] = max([out.get("backward", 0.0)] + [R64.worst_ratio(g32[kk], G64[kk], MG[kk])[0] for kk in g32])
        if hp.bn:
            O.bn_update_running(p32, hp, cache32)
            rs, Mrs = R64.running_stats(p0, hp, cache)
            out["running_stats"] = max([out.get("running_stats", 0.0)] + [R64.worst_ratio(p32[kk], rs[kk], Mrs[kk])[0] for kk in rs])
    return out


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


# ------------------------------------------------------------------------------------------------ the layout query
def plan(hp, confs, chunk_cols=0):
    from mfas_amd.engine import plan_population
    d = plan_population(engine_hyper(hp) if isinstance(hp, O.Hyper) else hp, [np.array(c) for c in confs], "cuda:0", chunk_cols)
    return (int(d["persistent"]), d["resident_units"], d["resident_workgroups"], d["units_per_workgroup"], d["chunk_cols"],
            int(d["lean_chain"]), int(d["wide"]))


def baseline_geometries():
    """(name, hyper, configurations): the search default (R = 16, B = 20), the headline (R = 128, B = 16), the MM-IMDB one."""
    from mfas_amd import Hyper
    from mfas_amd.mmimdb_searchable import MM_IMAGE_SIZES, MM_TEXT_SIZES
    c4 = [CONFS["c4"]]
    out = []
    for K in (1, 16, 64):
        out.append((f"r16_b20_k{K}", O.Hyper(R=16, C=60, B=20, bn=False, drpt=0.5), c4 * K))
        out.append((f"r128_b16_k{K}", O.Hyper(R=128, C=60, B=16, bn=False, drpt=0.5), c4 * K))
        out.append((f"mmimdb_k{K}", Hyper(R=128, C=23, B=32, bn=True, drpt=0.5, loss_mode=1, s_sizes=MM_TEXT_SIZES, v_sizes=MM_IMAGE_SIZES),
                    [CONFS["l2"]] * K))
    return out


# (persistent, resident units, resident workgroups, units per workgroup, chunk columns, lean chain) of mfas_population_plan on a
# device-less host (256 compute units assumed), recorded from a build of the parent commit; the new library gave the same.
PINNED_CASES = {
    "r1a": (1, 4, 4, 1, 256, 1), "r1b": (1, 2, 2, 1, 256, 1), "r16a": (0, 0, 0, 1, 64, 0), "r16b": (1, 14, 14, 1, 256, 1),
    "r17a": (0, 0, 0, 1, 64, 0), "r17b": (0, 0, 0, 1, 64, 0), "r32a": (0, 0, 0, 1, 64, 0), "r32b": (0, 0, 0, 1, 64, 0),
    "r33a": (0, 0, 0, 1, 64, 0), "r33b": (0, 0, 0, 1, 64, 0), "r65a": (0, 0, 0, 1, 64, 0), "r65b": (0, 0, 0, 1, 64, 0),
    "r80a": (0, 0, 0, 1, 64, 0), "r80b": (0, 0, 0, 1, 64, 0), "r128a": (0, 0, 0, 1, 64, 0), "r128b": (0, 0, 0, 1, 64, 0),
    "r129a": (0, 0, 0, 1, 64, 0), "r129b": (0, 0, 0, 1, 64, 0), "r256a": (0, 0, 0, 1, 64, 0), "r256b": (0, 0, 0, 1, 64, 0),
    "r257a": (0, 0, 0, 1, 64, 0), "r257b": (0, 0, 0, 1, 64, 0), "r300": (0, 0, 0, 1, 64, 0), "r320a": (0, 0, 0, 1, 64, 0),
    "r320b": (0, 0, 0, 1, 64, 0), "r448a": (0, 0, 0, 1, 64, 0), "r448b": (0, 0, 0, 1, 64, 0), "r449a": (0, 0, 0, 1, 64, 0),
    "r449b": (0, 0, 0, 1, 64, 0), "r512a": (0, 0, 0, 1, 64, 0), "r512b": (0, 0, 0, 1, 64, 0),
}
PINNED_BASELINE = {
    "r16_b20_k1": (1, 30, 30, 1, 256, 1), "r128_b16_k1": (0, 0, 0, 1, 64, 0), "mmimdb_k1": (0, 0, 0, 1, 64, 0),
    "r16_b20_k16": (1, 480, 240, 2, 256, 1), "r128_b16_k16": (0, 0, 0, 1, 128, 0), "mmimdb_k16": (0, 0, 0, 1, 64, 0),
    "r16_b20_k64": (0, 0, 0, 1, 128, 1), "r128_b16_k64": (0, 0, 0, 1, 64, 0), "mmimdb_k64": (0, 0, 0, 1, 64, 0),
}


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
