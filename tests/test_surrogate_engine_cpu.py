"""The engine's surrogate backend without a GPU: the float64 restatement the kernels are held to (tests/surr64.py) against torch
autograd + torch.optim.Adam in float64, the float32 yardstick the GPU tests reuse, the C ABI's argument checks (every one answers
before the first HIP call), and the Python surface (CLI choice, state_dict exchange, dispatch)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import surr64 as S

CASES = [(H, i, E, L, n) for (H, i, E) in S.SHAPES for L in (1, 2, 4) for n in (1, 17)]


@pytest.mark.parametrize("H,n_in,E,L,n", CASES)
def test_surr64_is_torch_autograd_and_adam_in_float64(H, n_in, E, L, n):
    """surr64's loss, BPTT gradient and Adam step against SimpleRecurrentSurrogate.double() + autograd + torch.optim.Adam: 1e-12 relative
    per tensor (two Adam steps, so the second one starts from non-zero moments)."""
    from mfas_amd.search.surrogate import SimpleRecurrentSurrogate
    c = S.case(H, n_in, E, L, n)
    m = SimpleRecurrentSurrogate(H, n_in, E).double()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["p64"].items()})
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x, y = torch.from_numpy(c["x"]).double(), torch.from_numpy(c["y"]).double().reshape(-1, 1)
    w, mo, v = S.flatten(c["p64"]), None, None
    mo = np.zeros_like(w)
    v = np.zeros_like(w)
    for step in (1, 2):
        opt.zero_grad()
        out = m(x)
        loss = torch.nn.MSELoss()(out, y)
        loss.backward()
        l64, g64, p64 = S.loss_and_grad(S.unflatten(w, H, n_in, E), c["x"], c["y"])
        assert abs(l64 - loss.item()) <= 1e-12 * abs(loss.item())
        assert np.abs(p64 - out.detach().numpy()[:, 0]).max() <= 1e-12
        named = dict(m.named_parameters())
        for k in S.KEYS:
            ref = named[k].grad.numpy()
            assert np.abs(g64[k] - ref).max() <= 1e-12 * np.abs(ref).max(), (k, step)
        opt.step()
        w, mo, v = S.adam_step(w, mo, v, S.flatten(g64), step)
        ref = S.flatten({k: q.detach().numpy() for k, q in named.items()})
        assert np.abs(w - ref).max() <= 1e-12 * np.abs(ref).max(), step
    # the unrolled statement the kernels follow is the same network
    assert torch.allclose(m.forward_unrolled(x), m(x), rtol=0, atol=1e-13)


@pytest.mark.parametrize("H,n_in,E,L,n", CASES)
def test_float32_yardstick_is_small_and_not_zero(H, n_in, E, L, n):
    """The yardstick of the GPU tests — the float32 CPU module's gradient against surr64's, per tensor — guards itself: a comparison
    that compared a thing with itself would give 0, a broken one something large.  (weight_hh's gradient is identically zero at L = 1:
    h0 = 0.)"""
    c = S.case(H, n_in, E, L, n)
    for k in S.KEYS:
        top = np.abs(c["g64"][k]).max()
        if k == "lstm.weight_hh_l0" and L == 1:
            assert top == 0.0 and c["yard"][k] == 0.0
            continue
        assert 0.0 < c["yard"][k] < 1e-4 * top, (k, c["yard"][k], top)
    assert 0.0 < c["pred_yard"] < 1e-5


def _shape(n_in=3, E=100, H=100):
    from mfas_amd import _lib
    return _lib.mfas_surrogate_shape(n_in, E, H, 0)


def test_param_count_and_prototypes():
    import __graft_entry__ as ge
    ge.build()
    from mfas_amd import _lib
    L = _lib.lib()
    assert L.mfas_surrogate_param_count(ctypes.byref(_shape())) == 81301 == len(S.flatten(S.initial_state(100, 3, 100)))
    assert L.mfas_surrogate_param_count(ctypes.byref(_shape(3, 40, 24))) == len(S.flatten(S.initial_state(24, 3, 40)))
    P, I32, I64, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    sp = ctypes.POINTER(_lib.mfas_surrogate_shape)
    assert list(L.mfas_surrogate_param_count.argtypes) == [sp] and L.mfas_surrogate_param_count.restype is I64
    assert list(L.mfas_surrogate_scratch_bytes.argtypes) == [sp, I32, I64] and L.mfas_surrogate_scratch_bytes.restype is I64
    assert list(L.mfas_surrogate_train.argtypes) == [sp, P, P, P, P, P, P, P, P, I32, I32, D, D, D, D, D, P, I64, P, P]
    assert list(L.mfas_surrogate_forward.argtypes) == [sp, P, P, I32, I64, P, P, I64, P]
    for name in ("mfas_surrogate_param_count", "mfas_surrogate_scratch_bytes", "mfas_surrogate_train", "mfas_surrogate_forward"):
        assert name in _lib.EXPORTS
    # the scratch query grows with both arguments and is what a train call checks against
    q = lambda L_, n: L.mfas_surrogate_scratch_bytes(ctypes.byref(_shape()), L_, n)
    assert 0 < q(1, 1) < q(4, 1) < q(4, 17) < q(4, 350)


def test_every_bad_argument_is_refused_before_any_device_call():
    """MFAS_EINVAL with a message naming the value, on a machine with no device: every pointer below is a made-up address that no check
    may follow."""
    import __graft_entry__ as ge
    ge.build()
    from mfas_amd import _lib
    L = _lib.lib()
    fake = 0x10000                                      # non-null, 16-byte aligned, never dereferenced
    step = ctypes.c_int64(0)
    loss = ctypes.c_float(0.0)
    big = 1 << 40

    def train(shape=None, params=fake, m=fake, v=fake, stepp=None, x=(fake,), y=(fake,), Ls=(2,), ns=(17,), nb=1, epochs=1, lr=1e-3,
              b1=0.9, b2=0.999, eps=1e-8, wd=0.0, scratch=fake, sbytes=big, lossp=None, null_lists=False):
        xs, ys = (ctypes.c_void_p * len(x))(*x), (ctypes.c_void_p * len(y))(*y)
        La, na = (ctypes.c_int32 * len(Ls))(*Ls), (ctypes.c_int64 * len(ns))(*ns)
        return L.mfas_surrogate_train(ctypes.byref(shape or _shape()), params, m, v, ctypes.byref(step) if stepp is None else stepp,
                                      None if null_lists else xs, ys, La, na, nb, epochs, lr, b1, b2, eps, wd, scratch, sbytes, None,
                                      ctypes.byref(loss) if lossp is None else lossp)

    def refused(rc, *words):
        assert rc == -1, rc                              # MFAS_EINVAL
        msg = L.mfas_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    need = L.mfas_surrogate_scratch_bytes(ctypes.byref(_shape()), 2, 17)
    refused(train(shape=_shape(n_in=0)), "n_in = 0")
    refused(train(shape=_shape(n_in=9)), "n_in = 9")
    refused(train(shape=_shape(E=15)), "E = 15")
    refused(train(shape=_shape(E=129)), "E = 129")
    refused(train(shape=_shape(H=8)), "H = 8")
    refused(train(shape=_shape(H=130)), "H = 130")
    refused(train(Ls=(0,)), "L = 0")
    refused(train(Ls=(5,)), "L = 5")
    refused(train(ns=(0,)), "n = 0")
    refused(train(nb=0), "n_buckets = 0")
    refused(train(epochs=0), "epochs = 0")
    refused(train(sbytes=need - 1), "scratch_bytes = %d" % (need - 1), str(need))
    refused(train(x=(fake, fake), y=(fake, fake), Ls=(1, 4), ns=(3, 40), nb=2, sbytes=need), "scratch_bytes", "bucket 1")
    for kw in ({"params": None}, {"m": None}, {"v": None}, {"stepp": ctypes.c_void_p(None)}, {"x": (None,)}, {"y": (None,)},
               {"scratch": None}, {"lossp": ctypes.c_void_p(None)}, {"null_lists": True}):
        refused(train(**kw), "null pointer")
    refused(train(b1=1.0), "beta1 = 1 ")
    refused(train(b1=-0.1), "beta1 = -0.1")
    refused(train(b2=1.5), "beta2 = 1.5")
    refused(train(eps=-1e-8), "eps = -1e-08")
    assert step.value == 0
    sh = ctypes.byref(_shape())
    assert L.mfas_surrogate_param_count(ctypes.byref(_shape(E=200))) == -1
    assert L.mfas_surrogate_scratch_bytes(sh, 5, 10) == -1 and L.mfas_surrogate_scratch_bytes(sh, 2, 0) == -1
    refused(L.mfas_surrogate_forward(ctypes.byref(_shape(H=200)), fake, fake, 2, 17, fake, None, 0, None), "H = 200")
    refused(L.mfas_surrogate_forward(sh, None, fake, 2, 17, fake, None, 0, None), "null pointer")
    refused(L.mfas_surrogate_forward(sh, fake, None, 2, 17, fake, None, 0, None), "null pointer")
    refused(L.mfas_surrogate_forward(sh, fake, fake, 2, 17, None, None, 0, None), "null pointer")
    refused(L.mfas_surrogate_forward(sh, fake, fake, 7, 17, fake, None, 0, None), "L = 7")
    refused(L.mfas_surrogate_forward(sh, fake, fake, 2, -3, fake, None, 0, None), "n = -3")


def test_cli_choice_state_dict_exchange_and_dispatch(monkeypatch):
    import main_searchable_ntu
    from mfas_amd.search import surrogate as M
    assert main_searchable_ntu.parse_args(["--surrogate_device", "engine"]).surrogate_device == "engine"
    assert main_searchable_ntu.parse_args([]).surrogate_device == "cpu"
    torch.manual_seed(5)
    eng = M.EngineSurrogate()
    torch.manual_seed(5)
    cpu = M.SimpleRecurrentSurrogate()
    assert isinstance(eng, M.SimpleRecurrentSurrogate)
    for (ka, a), (kb, b) in zip(eng.state_dict().items(), cpu.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka                # the same initialisation draws
    assert tuple(eng.state_dict().keys()) == S.KEYS
    other = M.SimpleRecurrentSurrogate()
    other.load_state_dict(eng.state_dict())
    eng2 = M.EngineSurrogate()
    eng2.load_state_dict(other.state_dict())
    x = torch.from_numpy(S.draw_bucket(3, 5, 1)[0])
    assert torch.equal(eng2(x), cpu(x))                          # on a CPU tensor the forward is the parent's
    with pytest.raises(ValueError):
        M.EngineSurrogateTrainer(eng, torch.optim.Adam(eng.parameters(), amsgrad=True))
    # a plain module takes the branches it took before: the eager loop on the CPU (never the engine trainer)
    made = []
    monkeypatch.setattr(M, "EngineSurrogateTrainer", lambda *a, **k: made.append(a) or (_ for _ in ()).throw(AssertionError("engine")))
    opt = torch.optim.Adam(cpu.parameters(), lr=1e-3)
    xb, yb = S.draw_bucket(2, 6, 2)
    before = cpu.hid2val.bias.detach().clone()
    loss = M.train_simple_surrogate(cpu, torch.nn.MSELoss(), opt, ([torch.from_numpy(xb)], [torch.from_numpy(yb).reshape(-1, 1)]), 2, "cpu")
    assert np.isfinite(loss) and not made and not torch.equal(before, cpu.hid2val.bias.detach())
    assert int(opt.state[cpu.hid2val.bias]["step"]) == 2 and not hasattr(cpu, "_engine_trainer")
