"""mfas_population_backward_taps (k_tap_grad) against the float64 reference of tests/tapgrad_ref64.py: every used tap's gradient of one
train-mode batch of one candidate, elementwise |got - ref64| <= TAU_TAP * 2^-24 * M, over the shape envelope of tests/ref64_cases.py
(31 cases x f32 / bf16 / f16 tables) and the cases of tests/tapgrad_cases.py (a tap selected by two and three cells, lean / general /
chain_split / wide / resident-planned plans, ragged batches, a row offset, slot 7); the identities the call promises (it IS
mfas_population_backward for plane 1 and the parameters, run-to-run and request-independent bits, zeros for an unused tap, refusals that
change nothing); and the module surface behind args.engine_tap_grads.

Run on its own, with a time limit:  python -m pytest tests/test_gpu_tapgrad_ref64.py -m gpu -x -q
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import tapgrad_cases as TC
from tests import tapgrad_ref64 as TG
from tests.gpu_support import dev, gpu_table, make_pop  # noqa: F401
from tests.ref64_cases import DTYPES

pytestmark = pytest.mark.gpu


def _setup(dev, cid, dtype="float32"):
    import torch
    r = TC.reference(cid, dtype)
    tab = gpu_table(r["t"], dtype, dev)
    pop = make_pop(r["hp"], r["conf"], dev, r["seed"], K=r["K"])
    for k in range(r["K"]):
        pop.set_state_dict(k, r["p0"])
    sched = pop.schedule()
    for key, want in r["opts"].get("expect", {}).items():
        assert sched[key] == want, (cid, key, sched)
    return r, tab, pop, torch.from_numpy(r["dlogits"]).to(dev)


def _call(pop, r, tab, dl, taps=None):
    return pop.backward_taps(r["k"], tab, dl, r["row0"], r["n"], step=TC.STEP, taps=taps)


def _check_case(dev, cid, dtype):
    r, tab, pop, dl = _setup(dev, cid, dtype)
    try:
        _, grads = _call(pop, r, tab, dl)
        assert set(grads) == set(r["ref"])
        for name, (ref, M) in r["ref"].items():
            got = grads[name].cpu().numpy()
            assert got.dtype == np.float32 and got.shape == ref.shape, (cid, name, got.shape)
            ratio = R64.assert_close64(got, ref, M, TC.TAU_TAP, f"{cid} {dtype} d {name}", record=f"backward_taps/{dtype}")
            print(f"backward_taps {cid} {dtype} {name}: {ratio:.3g}")
    finally:
        pop.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", [c[0][0] for c in TC.ENVELOPE])
def test_envelope_tap_gradients_vs_ref64(dev, cid, dtype):
    _check_case(dev, cid, dtype)


@pytest.mark.parametrize("cid", TC.TAP_CASE_IDS)
def test_tap_cases_vs_ref64(dev, cid):
    _check_case(dev, cid, "float32")


# ------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("cid", ["lean3a", "gen16", "wide64a", "res_k1", "short"])
def test_identities(dev, cid):
    import torch
    r, tab, pop, dl = _setup(dev, cid)
    k = r["k"]

    def fresh():
        for kk in range(r["K"]):
            pop.set_state_dict(kk, r["p0"])
    try:
        plane1 = pop.backward(k, tab, dl, r["row0"], r["n"], step=TC.STEP)
        params = pop.get_params(k, 0)
        fresh()
        flat0, none = _call(pop, r, tab, dl, taps=[])                  # every pointer NULL: the call is mfas_population_backward
        assert none == {} and torch.equal(flat0, plane1) and torch.equal(pop.get_params(k, 0), params)
        fresh()
        flat1, g1 = _call(pop, r, tab, dl)                              # taps requested: plane 1 and the parameters all the same
        assert torch.equal(flat1, plane1) and torch.equal(pop.get_params(k, 0), params)
        fresh()
        flat2, g2 = _call(pop, r, tab, dl)                              # again: the same bytes
        assert torch.equal(flat2, plane1) and all(torch.equal(g1[n], g2[n]) for n in g1)
        for name in g1:                                                 # one tap alone, and with an unused one: the same bytes
            fresh()
            _, g = _call(pop, r, tab, dl, taps=[name, "s3"])
            assert torch.equal(g[name], g1[name]), (cid, name)
            assert g["s3"].shape == (r["n"], r["hp"].s_sizes[3]) and not g["s3"].any(), (cid, "s3 is selected by no cell: zeros")
    finally:
        pop.close()


def test_rows_beyond_nrows_are_never_written(dev):
    """The raw C call with buffers one row longer than the batch, filled with a sentinel: rows >= nrows keep it, rows < nrows lose it."""
    import torch
    r, tab, pop, dl = _setup(dev, "short")
    try:
        n, hp = r["n"], r["hp"]
        bufs = {f"{m}{j}": torch.full((n + 1, w), -7.5, device=dev) for m, ws in (("s", hp.s_sizes), ("v", hp.v_sizes)) for j, w in enumerate(ws)}
        ptrs = {m: (C.c_void_p * 8)() for m in "sv"}
        for name, b in bufs.items():
            ptrs[name[0]][int(name[1:])] = b.data_ptr()
        tc = tab.to_c()
        rc = pop.lib.mfas_population_backward_taps(pop._h, 0, C.byref(tc), 0, n, TC.STEP, C.c_void_p(dl.data_ptr()), ptrs["s"], ptrs["v"])
        assert rc == 0, pop.lib.mfas_last_error()
        torch.cuda.synchronize()
        for name, b in bufs.items():
            assert (b[n] == -7.5).all(), name
            if name in r["ref"]:
                R64.assert_close64(b[:n].cpu().numpy(), *r["ref"][name], TC.TAU_TAP, f"short raw d {name}")
            else:
                assert not b[:n].any(), name
    finally:
        pop.close()


def test_refusals_change_nothing(dev):
    import torch
    r, tab, pop, dl = _setup(dev, "r16a")        # widths W_C: v3 is a slot of width 0
    try:
        pop.backward(0, tab, dl, 0, r["n"], step=TC.STEP)
        w, m = pop.get_params(0, 0), pop.get_params(0, 1)
        with pytest.raises(RuntimeError, match="v3.*width 0"):
            _call(pop, r, tab, dl, taps=["s0", "v3"])
        with pytest.raises(RuntimeError, match="batch size"):
            pop.backward_taps(0, tab, torch.zeros((r["hp"].B + 1, r["hp"].C), device=dev), 0, r["hp"].B + 1, step=TC.STEP)
        with pytest.raises(RuntimeError):
            pop.backward_taps(0, tab, dl, len(r["t"]["label"]) - 1, r["n"], step=TC.STEP)       # the row range leaves the table
        null = (C.c_void_p * 8)()
        tc = tab.to_c()
        assert pop.lib.mfas_population_backward_taps(pop._h, 0, C.byref(tc), 0, r["n"], TC.STEP, None, null, null) != 0      # no dlogits
        assert torch.equal(pop.get_params(0, 0), w) and torch.equal(pop.get_params(0, 1), m)
    finally:
        pop.close()


# ------------------------------------------------------------------------------------------------ the module surface
def _module(dev, **kw):
    import torch
    import mfas_amd as M
    args = SimpleNamespace(vid_len=(8, 32), num_outputs=60, drpt=0.0, inner_representation_size=16, batchnorm=True, alphas=True,
                           multitask=False, batchsize=16, **kw)
    conf = np.array([[0, 1, 0], [0, 1, 1], [2, 1, 2]])
    torch.manual_seed(5)
    model = M.Searchable_Skeleton_Image_Net(args, conf)
    model.train(True)
    t = O.synth_table(16, 3, snr=0.4)
    return model, conf, t


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_module_fills_the_grad_of_leaf_taps(dev, dtype):
    import torch
    from tests.ref64_cases import dequant
    model, conf, t = _module(dev, engine_tap_grads=True)
    feats = {k: dequant(v, dtype) for k, v in t.items() if k != "label"}
    x = {k: torch.from_numpy(v).to(dev).to(getattr(torch, dtype)).requires_grad_(k in ("s0", "v1", "s3")) for k, v in feats.items()}
    rgb, ske = {k: v for k, v in x.items() if k[0] == "v"}, {k: v for k, v in x.items() if k[0] == "s"}
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    out = model((rgb, ske))
    dl = TC.case_dlogits(SimpleNamespace(C=60), 16, 9)
    out.backward(torch.from_numpy(dl).to(dev))
    hp = O.Hyper(R=16, C=60, B=16, bn=True, drpt=0.0, alphas=True, epochs=1)
    _, _, cache = R64.forward(params, conf, hp, feats, True)
    ref = TG.tap_grads(params, conf, hp, cache, dl, taps=["s0", "v1", "s3"])
    for name, (g, M) in ref.items():
        got = x[name].grad
        assert got is not None and got.dtype == x[name].dtype and got.shape == x[name].shape, name
        # (a bf16 gradient is the float32 one rounded once more: 2^-9 of itself)
        R64.assert_close64(got.float().cpu().numpy(), g, M + (0.0 if dtype == "float32" else np.abs(g) * 2.0 ** 15 / TC.TAU_TAP), TC.TAU_TAP,
                           f"module {dtype} d {name}")
    assert not x["s3"].grad.any()                       # selected by no cell
    assert x["s1"].grad is None and model.central_classifier.weight.grad is not None


def test_module_trains_a_linear_in_front_of_a_tap(dev):
    import torch
    model, conf, t = _module(dev, engine_tap_grads=True)
    x = {k: torch.from_numpy(v).to(dev) for k, v in t.items() if k != "label"}
    lin = torch.nn.Linear(40, x["s0"].shape[1]).to(dev)
    inp = torch.randn(16, 40, device=dev)
    s0 = lin(inp)
    s0.retain_grad()
    rgb, ske = {k: v for k, v in x.items() if k[0] == "v"}, dict({k: v for k, v in x.items() if k[0] == "s"}, s0=s0)
    model((rgb, ske)).square().sum().backward()
    assert s0.grad is not None and s0.grad.any()
    torch.testing.assert_close(lin.weight.grad, s0.grad.T @ inp, rtol=1e-5, atol=1e-6 * float(lin.weight.grad.abs().max()))
    torch.testing.assert_close(lin.bias.grad, s0.grad.sum(0), rtol=1e-5, atol=1e-6 * float(lin.bias.grad.abs().max()))


def test_module_without_the_flag_still_refuses(dev):
    import torch
    model, conf, t = _module(dev)
    x = {k: torch.from_numpy(v).to(dev) for k, v in t.items() if k != "label"}
    rgb, ske = {k: v.clone().requires_grad_(True) for k, v in x.items() if k[0] == "v"}, {k: v for k, v in x.items() if k[0] == "s"}
    with pytest.raises(NotImplementedError, match="the taps require grad"):
        model((rgb, ske))
    model.train(False)
    assert not model((rgb, ske)).requires_grad            # eval mode keeps detaching silently
