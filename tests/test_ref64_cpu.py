"""CPU checks of the float64 reference (tests/ref64.py) and of its comparison rule, before any GPU result is judged by it:

* ref64 reproduces the G23 goldens of the unchanged reference (the tolerances of test_oracle_golden.py);
* calibration: the float32 oracle passes assert_close64 with a margin of at least x4 on every GPU case shape
  (tests/test_gpu_ref64.py::CASES, all three table dtypes);
* mutations: float32 results that are subtly wrong in the ways a kernel goes wrong fail the rule;
* the GPU cases form a covering design (every value of every axis at least twice)."""
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import train_cases as GT
from tests.helpers import load_npz
from tests.oracle32_runs import F32, MUT_CE, TAUS, oracle_case, oracle_train_steps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ pin to the G23 goldens
def test_ref64_matches_g23_goldens():
    from tests.golden_cases import CONFS, VARIANTS, check
    g = load_npz(os.path.join(GOLDEN, "g23_forward_backward.npz"))
    t = O.synth_table(16, 11, snr=0.3, with_logits=True)
    labels = t["label"]
    n = 0
    for name in g["names"]:
        cname, vname, R, seed = str(name).split("/")
        R, seed = int(R), int(seed)
        kw, train = VARIANTS[vname]
        hp = O.Hyper(R=R, B=16, **kw)
        conf = np.array(CONFS[cname])
        params = O.init_params(conf, hp, seed, perturb_bn=True)
        pre = f"{cname}/{vname}/{R}/"
        logits, _, cache = R64.forward(params, conf, hp, t, train)
        np.testing.assert_allclose(logits, g[pre + "logits"], rtol=2e-4, atol=2e-5, err_msg=pre)
        loss = R64.ce_loss(logits, labels)
        preds = np.argmax(logits, 1)
        if hp.multitask:
            np.testing.assert_allclose(loss, g[pre + "loss_central"], rtol=1e-5)
            np.testing.assert_allclose(R64.multitask_loss(logits, t["vlogit"], t["slogit"], labels), g[pre + "loss"], rtol=1e-5)
            preds = np.argmax(logits + t["vlogit"] + t["slogit"], 1)
        else:
            np.testing.assert_allclose(loss, g[pre + "loss"], rtol=1e-5)
        assert np.array_equal(preds, g[pre + "preds"]), pre
        if train:
            sm = np.exp(logits - logits.max(1, keepdims=True))
            sm /= sm.sum(1, keepdims=True)
            dl = sm.copy()
            dl[np.arange(16), labels] -= 1.0
            grads, _ = R64.backward(params, hp, cache, dl / 16.0)
            for k, v in grads.items():
                check(g, pre + "grad/" + k, v, rtol=2e-3, atol=2e-7, scale_atol=1e-3)
            rs, _ = R64.running_stats(params, hp, cache)
            for k, v in rs.items():
                np.testing.assert_allclose(v, g[pre + "after/" + k], rtol=1e-5, atol=1e-6)
        n += 1
    assert n >= 40


def test_bce_and_f1_match_the_oracle():
    rng = np.random.default_rng(3)
    lg = (3 * rng.standard_normal((40, 23))).astype(F32)
    z = (rng.random((40, 23)) < 0.2).astype(F32)
    w = O.mm_pos_weight()
    np.testing.assert_allclose(R64.bce_loss(lg, z, w), O.bce_loss(lg, z, w)[0], rtol=1e-5)
    assert abs(R64.f1_rows(lg, z, 0.3).sum() * 2.0 ** 32 - O.f1_samples_fixed(lg, z, 0.3)) <= 40


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_float32_oracle_calibration_margin(case):
    for dtype in G.DTYPES:
        for q, r in oracle_case(case, dtype).items():
            assert r * 4.0 <= TAUS[q], (case[0], dtype, q, r, TAUS[q])


def test_gpu_cases_cover_every_axis_value_twice():
    axes = {
        "R": [1, 16, 17, 32, 33, 65, 80, 128, 129, 256, 257, 320, 448, 449, 512],
        "C": [1, 2, 17, 60, 64, 65, 128],
        "B": [2, 3, 16, 17, 20, 32, 33, 64],
        "width": [1, 8, 9, 15, 17, 63, 65, 1000, 2048, 4100],
    }
    seen = {a: [] for a in axes}
    cell = {"bn": set(), "drpt": set(), "extra": set()}
    for cid, R, C, B, w, cells, bn, drpt, extra in G.CASES:
        seen["R"].append(R)
        seen["C"].append(C)
        seen["B"].append(B)
        used = {w["s"][c[0]] for c in cells} | {w["v"][c[1]] for c in cells}
        seen["width"] += sorted(used)
        assert 0 not in used, cid
        Bp = 64 if B > 32 else (32 if B > 16 else 16)
        assert -(-C // 16) * 16 <= 8 * min(16, 512 // Bp), cid        # the validator's C_padded limit
        cell["bn"].add(bn)
        cell["drpt"].add(drpt)
        cell["extra"] |= set(filter(None, extra.split(",")))
    for a, vals in axes.items():
        for v in vals:
            assert seen[a].count(v) >= 2, (a, v, seen[a].count(v))
    assert sum(0 in c[4]["s"] + c[4]["v"] for c in G.CASES) >= 2      # an unused width-0 slot next to the taps in use
    assert cell["bn"] == {True, False} and cell["drpt"] == {0.0, 0.5, 0.9}
    assert cell["extra"] == {"alphas", "sig1", "multitask", "lm1"}


# ------------------------------------------------------------------------------------------------ mutations
def _trunc16(a):
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return (u & np.uint32(0xFFFFFF00)).view(F32)


def _eval_pair(R=80, C=60, N=83, cells=((2, 3, 0),), bn=False, dtype="bfloat16", seed=5):
    case = ("mut", R, C, 16, G.W_A, [list(c) for c in cells], bn, 0.5, "")
    hp = G.case_hyper(case)
    conf, p = G.case_params(case, hp, seed)
    t = G.case_table(case, hp, N, seed, dtype)
    f = G.feats_of(t)
    lg, Ml, _ = R64.forward(p, conf, hp, f, False)
    return hp, conf, p, t, f, lg, Ml


def _fails(got, ref, M, tau):
    with pytest.raises(AssertionError):
        R64.assert_close64(got, ref, M, tau, "mutation")


@pytest.mark.parametrize("R,cells", G.B3_CASES)
def test_one_layer_calibration_margin(R, cells):
    for dtype in ("bfloat16", "float32"):
        hp, conf, p, t = G.one_layer_setup(R, cells, 77, dtype)
        f = G.feats_of(t)
        lg, Ml, _ = R64.forward(p, conf, hp, f, False)
        R64.assert_close64(O.forward(p, conf, hp, f, False)[0], lg, Ml, G.TAU_ONE_LAYER / 4, f"one-layer R{R} {dtype}")


@pytest.mark.parametrize("R,cells", G.B3_CASES)
def test_mutation_b3_without_lo_term(R, cells):
    """Weights cut to 16 significant bits before the product (bf16 x 3 without its lo term), bf16 tables, the B3 shapes of
    test_gpu_ref64.py.  The cut is a relative error of up to 2^-16 per weight with the weight's sign."""
    hp, conf, p, t = G.one_layer_setup(R, cells, 77, "bfloat16")
    f = G.feats_of(t)
    lg, Ml, _ = R64.forward(p, conf, hp, f, False)
    q = {k: (_trunc16(v) if k.startswith("fusion") and k.endswith("0.weight") else v) for k, v in p.items()}
    _fails(O.forward(q, conf, hp, f, False)[0], lg, Ml, G.TAU_ONE_LAYER)


def test_mutation_tile_rows_from_wrong_sample():
    hp, conf, p, t, f, lg, Ml = _eval_pair(R=33, cells=((0, 1, 0), (3, 2, 1)), bn=True, dtype="float32")
    f2 = {k: v.copy() for k, v in f.items()}
    for k in f2:                        # rows 16..31 (the second 16-row tile) read sample r + 1
        if k[0] in "sv":
            f2[k][16:32] = f[k][17:33]
    bad, _ = O.forward(p, conf, hp, f2, False)
    _fails(bad, lg, Ml, G.TAU_LOGITS)


def test_mutation_ragged_tail_row_zeroed():
    hp, conf, p, t, f, lg, Ml = _eval_pair(R=17, N=83, cells=((1, 1, 0),), dtype="float16")
    bad, _ = O.forward(p, conf, hp, f, False)
    bad[-1] = 0.0                       # the last row of the ragged last tile (83 = 5 * 16 + 3) never written
    _fails(bad, lg, Ml, G.TAU_LOGITS)


def test_mutation_partial_column_chunk_off_by_one_block():
    """The last, partial 16-column block of a 1000-wide tap read one block to the left."""
    hp, conf, p, t, f, lg, Ml = _eval_pair(R=65, cells=((0, 3, 0),), dtype="float32")
    f2 = {k: v.copy() for k, v in f.items()}
    f2["v3"][:, 992:1000] = f["v3"][:, 976:984]
    bad, _ = O.forward(p, conf, hp, f2, False)
    _fails(bad, lg, Ml, G.TAU_LOGITS)


def test_mutation_16bit_values_rounded_twice():
    """f16 table values rounded a second time on the way in (through bfloat16)."""
    hp, conf, p, t, f, lg, Ml = _eval_pair(R=16, cells=((3, 3, 0),), dtype="float16")
    f2 = {k: (O.bf16_round(v) if k[0] in "sv" else v) for k, v in f.items()}
    bad, _ = O.forward(p, conf, hp, f2, False)
    _fails(bad, lg, Ml, G.TAU_LOGITS)


def _train_pair(bn, drpt):
    case = ("mut", 32, 17, 20, G.W_A, [[3, 3, 0], [1, 2, 1]], bn, drpt, "")
    hp = G.case_hyper(case)
    conf, p = G.case_params(case, hp, 9)
    t = G.case_table(case, hp, 20, 9, "float32")
    f = G.feats_of(t)
    return hp, conf, p, f


def test_mutation_dropout_mask_shifted_by_one_step():
    hp, conf, p, f = _train_pair(True, 0.5)
    lg, Ml, cache = R64.forward(p, conf, hp, f, True, seed=4, step=3)
    ok, _ = O.forward({k: v.copy() for k, v in p.items()}, conf, hp, f, True, seed=4, step=3)
    R64.assert_close64(ok, lg, Ml, G.TAU_LOGITS / 4, "unmutated")
    bad, _ = O.forward({k: v.copy() for k, v in p.items()}, conf, hp, f, True, seed=4, step=4)
    _fails(bad, lg, Ml, G.TAU_LOGITS)
    dl = np.random.default_rng(0).standard_normal(lg.shape).astype(F32) / 20
    G64, MG = R64.backward(p, hp, cache, dl)
    _, cache_bad = O.forward({k: v.copy() for k, v in p.items()}, conf, hp, f, True, seed=4, step=4)
    gbad = O.backward(p, hp, cache_bad, dl)
    with pytest.raises(AssertionError):
        for k in G64:
            R64.assert_close64(gbad[k], G64[k], MG[k], G.TAU_GRAD, f"mutation {k}")


def test_mutation_bn_biased_running_variance():
    hp, conf, p, f = _train_pair(True, 0.0)
    _, _, cache = R64.forward(p, conf, hp, f, True)
    rs, Mrs = R64.running_stats(p, hp, cache)
    p32 = {k: v.copy() for k, v in p.items()}
    _, c32 = O.forward(p32, conf, hp, f, True)
    O.bn_update_running(p32, hp, c32)
    for k in rs:
        R64.assert_close64(p32[k], rs[k], Mrs[k], G.TAU_RUNSTAT / 4, "unmutated")
    for i, c in enumerate(c32["cells"]):     # the biased batch variance instead of the unbiased one
        k = f"fusion_layers.{i}.2.running_var"
        biased = (p[k] + F32(hp.bn_momentum) * (c["var"] - p[k])).astype(F32)
        _fails(biased, rs[k], Mrs[k], G.TAU_RUNSTAT)


# ------------------------------------------------------------------------------------------------ one train step (tests/test_gpu_train_ref64.py)
# Calibration and power of the stepwise train() check, on the shapes, orders and learning rates the GPU test uses: the float32
# oracle takes the engine's place, teacher-forced from its own state through ref64.train_step64.


def test_train_case_dtypes_rotate():
    per = [sum(GT.case_dtype(c) == d for c in G.CASE_IDS) for d in G.DTYPES]
    assert min(per) >= 10, per
    assert GT.TAU_M == G.TAU_GRAD and GT.TAUS["runstat"] == G.TAU_RUNSTAT
    assert all(2 <= GT.ragged_rows(B) < B for B in (3, 16, 17, 20, 32, 33, 64)) and GT.ragged_rows(2) == 2


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_train_step_calibration_margin(case):
    """The float32 oracle stays under a quarter of each tau on the GPU test's own shapes, orders and steps."""
    r = oracle_train_steps(case, GT.case_dtype(case[0]))
    for q, tau in GT.TAUS.items():
        assert r[q] * 4.0 <= tau, (case[0], q, r[q], tau)
    assert r["count"] == 0.0, case[0]


MUT_LM1 = ("mut", 17, 23, 16, G.W_A, [[0, 3, 0], [1, 1, 2]], False, 0.5, "lm1")
MUTATIONS = {
    "div_B": MUT_CE,                    # the loss gradient of the ragged batch divided by B instead of nvalid
    "no_wd": MUT_CE,                    # weight decay left out of g'
    "m_no_decay": MUT_CE,               # m = (1 - beta1) g' without - m_{j-1}
    "scalars_prev": MUT_CE,             # the step scalars of step j - 1 used at step j
    "stale_forward": MUT_CE,            # batch j run with w_{j-2}
    "order_epoch0": MUT_CE,             # epoch 0's order row reused in epoch 1
    "order_other_candidate": MUT_CE,    # rows gathered by another candidate's order
    "bn_pad": MUT_CE,                   # a padded row counted in the BN batch mean
    "no_pos_weight": MUT_LM1,           # pos_weight ignored in the BCE gradient
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_train_step_mutations(mut):
    """Each way a train step goes wrong exceeds its tau on at least one checked quantity; the same setup unmutated keeps x4."""
    case = MUTATIONS[mut]
    ok = oracle_train_steps(case, "bfloat16", seed=9)
    assert all(ok[q] * 4.0 <= tau for q, tau in GT.TAUS.items()) and ok["count"] == 0.0, ok
    bad = oracle_train_steps(case, "bfloat16", mut=mut, seed=9)
    over = {q: bad[q] for q, tau in GT.TAUS.items() if bad[q] > tau}
    assert over, (mut, bad)
