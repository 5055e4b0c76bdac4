"""CPU checks of the tap-gradient reference (tests/tapgrad_ref64.py), of its tolerance and of k_tap_grad's work list, before any GPU result
is judged by them:

* the d_y recovered from ref64.backward through the identity-input cache, multiplied back by the true x, is ref64's own weight gradient;
* torch.autograd on a float64 restatement of the chain (ref64's dropout masks injected, taps as leaves) gives the ref64-derived tap
  gradients to 1e-10 relative, on every case;
* the ref64-derived values hold a golden of the unchanged reference's own tap gradients (tests/golden/g24_tap_gradients.npz);
* calibration: the float32 oracle-derived values pass |got - ref| <= tau * 2^-24 * M with a margin of at least x4 (TAU_TAP = TAU_GRAD = 20)
  on the 31 envelope cases x 3 table dtypes and on tests/tapgrad_cases.py's own;
* power: each of four wrong gradients exceeds the tau on some case;
* the work list (tap_grad_units through a g++ program, also under the address and undefined sanitizers) over the plan cases;
* the C ABI's new entry is declared, exported, bound and documented alike.

Measured worst ratios |oracle32-derived - ref64| / (2^-24 M) (tau / 4 = 5): envelope 2.1 (r512b, all three dtypes; next r448a 1.3),
new cases 1.3 (wide64; gen17a 1.2, lean3n 1.1); no further term of M was needed.  Under BatchNorm M compounds from cell to cell (ratios of
1e-3 .. 1e-6 there, and a dropped cell stays inside the tau at R = 128), so every plan kind also has a case without it.  Power, the largest
ratio each mutation reaches over the new cases: alpha scale dropped 5.6e6, second cell dropped 7.4e5, column offset + 16 1.2e8, V scale for
S 6.6e5 — each also above the tau on the lean, general, wide and resident-planned cases without BatchNorm (the two alpha ones: where the
case has alphas).

Tile offsets: a candidate's vector block is rounded to 64 floats, so a tile's plane offset is a multiple of 256 bytes (what the kernel's
16-byte loads need), not of 1 KiB; tile-to-tile strides are whole 1 KiB tiles.  The work-list check asserts exactly that.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import plan_header as PH
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import tapgrad_cases as TC
from tests import tapgrad_header as TH
from tests import tapgrad_ref64 as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("cid", ["r16b", "r65b", "r128a", "lean3a", "one"])
def test_recovered_dy_reproduces_ref64_weight_gradients(cid):
    r = TC.reference(cid)
    G64, M64 = R64.backward(r["p0"], r["hp"], r["cache"], r["dlogits"])
    for i, (d_y, M_dy) in enumerate(TG.recover_dy(r["p0"], r["hp"], r["cache"], r["dlogits"])):
        c = r["cache"]["cells"][i]
        assert d_y.shape == (r["n"], r["hp"].R)
        # (float64 sums in another order: held to 1e-12 of the element's own magnitude)
        Mw, Mb = M64[f"fusion_layers.{i}.0.weight"], M64[f"fusion_layers.{i}.0.bias"]
        assert (np.abs(d_y.T @ c["x"] - G64[f"fusion_layers.{i}.0.weight"]) <= 1e-12 * Mw).all()
        assert (np.abs(M_dy.T @ c["Mx"] - Mw) <= 1e-12 * Mw).all()
        assert (np.abs(d_y.sum(0) - G64[f"fusion_layers.{i}.0.bias"]) <= 1e-12 * Mb).all()
        assert (M_dy >= np.abs(d_y) * (1 - 1e-12)).all()


@pytest.mark.parametrize("cid", TC.ALL_IDS)
def test_autograd_of_a_float64_restatement_agrees(cid):
    r = TC.reference(cid)
    got, logits = TG.torch_tap_grads(r["p0"], r["conf"], r["hp"], r["feats"], r["dlogits"], r["cache"])
    assert np.abs(logits - r["logits"]).max() <= 1e-10 * max(np.abs(r["logits"]).max(), 1e-30)
    assert set(got) == set(r["ref"]) == set(TG.used_taps(r["conf"]))
    for name, (ref, _) in r["ref"].items():
        assert got[name].shape == ref.shape
        assert np.abs(got[name] - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-30), (cid, name)


def test_a_tap_no_cell_selects_gets_zeros_and_requests_are_independent():
    r = TC.reference("lean3a")
    some = TG.tap_grads(r["p0"], r["conf"], r["hp"], r["cache"], r["dlogits"], taps=["s3", "v1"])
    assert not some["s3"][0].any() and some["s3"][0].shape == (r["n"], 9)
    assert np.array_equal(some["v1"][0], r["ref"]["v1"][0])


# ------------------------------------------------------------------------------------------------ pin to the unchanged reference
def test_ref64_tap_gradients_match_the_reference_golden():
    """tests/golden/g24_tap_gradients.npz (make_golden_tapgrad.py: the unchanged reference in train mode, taps as leaves that require
    grad, BatchNorm without dropout, mean cross entropy of 8 rows; without and with alphas): the reference's float32 gradients are held
    to the ref64-derived ones under the same rule as the engine's, the loss gradient's own error (ce_dlogits) counted in M."""
    from tests.helpers import load_npz
    g = load_npz(os.path.join(ROOT, "tests", "golden", "g24_tap_gradients.npz"))
    conf, t, n = np.array(g["conf"]), O.synth_table(16, 11, snr=0.3, with_logits=True), 8
    assert len(g["names"]) == 2
    for name in g["names"]:
        vname, seed = str(name).split("/")
        hp = O.Hyper(R=16, B=16, bn=True, drpt=0.0, alphas="alpha" in vname)
        params = O.init_params(conf, hp, int(seed), perturb_bn=True)
        feats = {k: v[:n] for k, v in t.items() if k != "label"}
        lg, Ml, cache = R64.forward(params, conf, hp, feats, True)
        np.testing.assert_allclose(R64.ce_loss(lg, t["label"][:n]), g[f"{vname}/loss"], rtol=1e-5)
        dl, Mdl = R64.ce_dlogits(lg, Ml, t["label"][:n], n, G.TAU_LOGITS)
        ref = TG.tap_grads(params, conf, hp, cache, dl, M_dlogits=Mdl)
        assert sorted(ref) == sorted(k.split("/")[-1] for k in g if k.startswith(f"{vname}/grad/")) == ["s0", "s1", "v0"]
        for tap, (val, M) in ref.items():
            ratio = R64.assert_close64(g[f"{vname}/grad/{tap}"], val, M, TC.TAU_TAP, f"golden {vname} d {tap}")
            print(f"golden {vname} {tap}: {ratio:.3g}")


# ------------------------------------------------------------------------------------------------ the tolerance
def _oracle32_ratio(cid, dtype):
    r = TC.reference(cid, dtype)
    hp = r["hp"]
    p32 = {k: v.copy() for k, v in r["p0"].items()}
    _, cache32 = O.forward(p32, r["conf"], hp, r["feats"], True, seed=r["seed"] + r["k"], step=TC.STEP)
    g32 = TG.tap_grads32(p32, r["conf"], hp, cache32, r["dlogits"])
    return max(R64.worst_ratio(g32[name], ref, M)[0] for name, (ref, M) in r["ref"].items())


@pytest.mark.parametrize("cid", TC.ALL_IDS)
def test_float32_oracle_calibration_margin(cid):
    for dtype in (G.DTYPES if cid in G.CASE_IDS else ("float32",)):
        ratio = _oracle32_ratio(cid, dtype)
        print(f"calibration {cid} {dtype}: {ratio:.3g}")
        assert ratio * 4.0 <= TC.TAU_TAP, (cid, dtype, ratio)


@pytest.mark.parametrize("mutation", ["no_alpha", "drop_second", "shift_block", "v_scale_for_s"])
def test_wrong_gradients_exceed_the_tau(mutation):
    worst = {}
    for cid in TC.TAP_CASE_IDS:
        r = TC.reference(cid)
        bad = TG.tap_grads(r["p0"], r["conf"], r["hp"], r["cache"], r["dlogits"], mutate=mutation)
        worst[cid] = max(R64.worst_ratio(bad[name][0], ref, M)[0] for name, (ref, M) in r["ref"].items())
    print(f"power {mutation}:", " ".join(f"{k}:{v:.2g}" for k, v in worst.items()))
    assert max(worst.values()) > TC.TAU_TAP, (mutation, worst)
    # ... and on every plan kind: the lean chain, the general chain (chain_split geometry), a wide plan, a resident-planned population
    alpha = mutation in ("no_alpha", "v_scale_for_s")
    for cid in (("lean3n", "wide128n") if alpha else ("lean3n", "gen16n", "wide128n", "res_k1n")):
        assert worst[cid] > TC.TAU_TAP, (mutation, cid, worst[cid])


# ------------------------------------------------------------------------------------------------ the work list
def _check_work_list(case, text):
    cands, refused = TH.parse(text)
    hp, K = case["hp"], len(case["confs"])
    assert [c["k"] for c, _ in cands] == sorted({0, K - 1}), case["id"]
    for c, units in cands:
        sizes = {0: list(hp.s_sizes) + [0] * 8, 1: list(hp.v_sizes) + [0] * 8}
        seen, tiles = {}, []
        for u in units:
            assert 1 <= u["nkb"] <= 8 and u["nrb"] == c["nrb"] and u["width"] == sizes[u["kind"]][u["tap"]] > 0, (case["id"], u)
            # every using cell, ascending, and only those
            using = [i for i, sv in enumerate(c["conf"]) if sv[u["kind"]] == u["tap"]]
            assert [it[0] for it in u["items"]] == using and u["nitems"] == len(using), (case["id"], u, c["conf"])
            for j in range(u["nkb"]):
                key = (u["kind"], u["tap"], u["kb0"] + j)
                assert key not in seen, (case["id"], key)
                seen[key] = True
            for cell, w_off, stride in u["items"]:
                assert w_off % 64 == 0 and stride % 256 == 0 and (stride >= 256 * u["nkb"] or u["nrb"] == 1), (case["id"], u)
                first = w_off + 256 * np.arange(u["nkb"])[:, None] + stride * np.arange(u["nrb"])[None, :]
                assert first.min() >= c["base"] and first.max() + 256 <= c["base"] + c["size"], (case["id"], u, c)
                tiles.append(first.ravel())
        # every 16-column block of every declared slot exactly once
        want = {(kind, tap, kb) for kind in (0, 1) for tap in range(8) for kb in range(-(-sizes[kind][tap] // 16))}
        assert set(seen) == want, (case["id"], sorted(want - set(seen))[:5], sorted(set(seen) - want)[:5])
        if tiles:       # no tile is named twice
            allt = np.concatenate(tiles)
            assert len(np.unique(allt)) == len(allt), case["id"]
    for slot, rc, nunits, msg in refused:
        assert rc != 0 and nunits == 0 and slot in msg and "width 0" in msg, (case["id"], slot, rc, nunits, msg)
    return len(refused)


def _plan_cases():
    from tests.plan_cases import all_cases
    return all_cases()


def test_work_list_over_the_plan_cases():
    cases = _plan_cases()
    texts = TH.dumps(cases)
    wide = split = refused = 0
    for case, text in zip(cases, texts):
        refused += _check_work_list(case, text)
        wide += "wide" in case["id"]
        split += "split" in case["id"]
    assert len(cases) > 500 and wide and split and refused


def test_work_list_under_the_sanitizers():
    """The same stand-alone program built with -fsanitize=address,undefined, run directly over a spread of the plan cases: the same text."""
    cases = _plan_cases()[::7]
    assert TH.dumps(cases, flags=PH.SANITIZE) == TH.dumps(cases)


def test_work_list_refuses_pieces_that_do_not_join():
    """A join that forgot the row-block offset of a piece would name the wrong tiles: the builder refuses such pieces instead."""
    cases = [c for c in _plan_cases() if "wide" in c["id"]][:3]
    assert cases
    exe = TH.program(("p->w_off != p0.w_off + (int64_t)p->rb0 * stride", "p->w_off != p0.w_off"))
    res = subprocess.run([exe], input="".join(PH.case_text(c, 0) for c in cases).encode(), capture_output=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if not k.startswith("MFAS_")})
    assert res.returncode == 0 and b"do not join" in res.stdout


# ------------------------------------------------------------------------------------------------ the ABI
def test_backward_taps_is_declared_exported_bound_and_documented():
    from mfas_amd import _lib
    name = "mfas_population_backward_taps"
    header = open(os.path.join(ROOT, "include", "mfas_hip.h")).read()
    m = re.search(r"int " + name + r"\(([^;]*)\);", header)
    assert m, "not declared in include/mfas_hip.h"
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 9 and "float* const* ds" in m.group(1) and "float* const* dv" in m.group(1)
    assert name in _lib.EXPORTS
    src = open(os.path.join(ROOT, "mfas_amd", "_lib.py")).read()
    assert re.search(r"L\." + name + r"\.argtypes\s*=", src), "no argtypes in mfas_amd/_lib.py"
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert len(getattr(L, name).argtypes) == 9 and getattr(L, name).argtypes[:7] == L.mfas_population_backward.argtypes
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), "no row in INTEGRATION.md"
    assert "ntu_searchable.py:206-247" in header[header.index(name) - 2500:header.index(name)]
