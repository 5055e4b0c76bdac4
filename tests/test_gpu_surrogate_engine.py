"""The engine's surrogate kernels (mfas_amd/csrc/surrogate.hip.h: k_surr_grad, k_surr_adam, k_surr_forward) on the GPU against the float64
restatement tests/surr64.py, with the float32 CPU module's own distance from surr64 as the yardstick (margin 4: another summation
order, the MFMA accumulation order, the device's expf / tanhf), and the Python surface on top of them.

Largest observed ratio |g_engine - g64| / max(yardstick, 2^-20 max|g64|) per tensor over all cases of test_gradient_element_by_element
(MI355X; the bound is 4): embedding.0.weight 1.004, embedding.0.bias 1.005, lstm.weight_ih_l0 1.004, lstm.weight_hh_l0 0.999,
lstm.bias_ih_l0 = lstm.bias_hh_l0 1.003, hid2val.weight 1.005, hid2val.bias 1.001 — all eight at (100, 3, 100), L = 2, n = 1, where the whole
gradient is proportional to the one row's pred - y and both float32 paths carry the same rounding of that prediction (the deviation IS the
yardstick there); over the cases with n >= 15 the largest ratio is 0.39, weight_ih at (100, 3, 100), L = 4, n = 17 (profiles/engine_surrogate.log)."""
import ctypes
import random
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import np_oracle as O
from tests import surr64 as S
from tests.helpers import golden
from tests.surr_cases import CASES, RATIOS
from tests.gpu_dev import dev  # noqa: F401

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20


class Engine:
    """The C ABI with caller-owned torch buffers: parameters, both moments, the step count and the scratch."""

    def __init__(self, H, n_in, E, dev, flat32, extra_scratch=0):
        from mfas_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.shape = _lib.mfas_surrogate_shape(n_in, E, H, 0)
        self.dev = dev
        self.w = torch.from_numpy(np.asarray(flat32, np.float32).copy()).to(dev)
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.step = ctypes.c_int64(0)
        self.extra = extra_scratch
        self.scratch = None

    def train(self, buckets, epochs, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
        xs = [torch.from_numpy(x).to(self.dev) for x, _ in buckets]
        ys = [torch.from_numpy(y).to(self.dev) for _, y in buckets]
        nb = len(xs)
        Ls = (ctypes.c_int32 * nb)(*[x.shape[0] for x in xs])
        ns = (ctypes.c_int64 * nb)(*[x.shape[1] for x in xs])
        need = self.L.mfas_surrogate_scratch_bytes(ctypes.byref(self.shape), max(Ls), max(ns))
        assert need > 0
        if self.scratch is None or self.scratch.numel() < need + self.extra:
            self.scratch = torch.empty(need + self.extra, dtype=torch.uint8, device=self.dev)
        loss = ctypes.c_float(-1.0)
        self._lib.check(self.L.mfas_surrogate_train(
            ctypes.byref(self.shape), self.w.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), ctypes.byref(self.step),
            (ctypes.c_void_p * nb)(*[x.data_ptr() for x in xs]), (ctypes.c_void_p * nb)(*[y.data_ptr() for y in ys]), Ls, ns, nb, epochs,
            lr, betas[0], betas[1], eps, wd, self.scratch.data_ptr(), self.scratch.numel(), torch.cuda.current_stream().cuda_stream,
            ctypes.byref(loss)))
        return loss.value

    def forward(self, x):
        xd = torch.from_numpy(x).to(self.dev)
        pred = torch.empty(x.shape[1], device=self.dev)
        self._lib.check(self.L.mfas_surrogate_forward(ctypes.byref(self.shape), self.w.data_ptr(), xd.data_ptr(), x.shape[0], x.shape[1],
                                                      pred.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream))
        return pred.cpu().numpy()

    def state(self):
        return self.w.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy()


def fresh(H, n_in, E, dev, **kw):
    return Engine(H, n_in, E, dev, S.flatten(S.initial_state(H, n_in, E), np.float32), **kw)


def slices(H, n_in, E):
    out, off = {}, 0
    for k, shp in S.shapes_of(H, n_in, E).items():
        out[k] = slice(off, off + int(np.prod(shp)))
        off += int(np.prod(shp))
    return out


@pytest.mark.parametrize("H,n_in,E,L,n", CASES)
def test_gradient_element_by_element(dev, H, n_in, E, L, n):
    """One step from zeroed moments: exp_avg = (1 - beta1) g and exp_avg_sq = (1 - beta2) g^2 hold the engine's gradient.  Per tensor
    |g_engine - g64| <= 4 max(yardstick, 2^-20 max|g64|); the two LSTM bias slots are bit-identical."""
    c = S.case(H, n_in, E, L, n)
    eng = fresh(H, n_in, E, dev)
    eng.train([(c["x"], c["y"])], 1)
    _, m, v = eng.state()
    g = m.astype(np.float64) / float(np.float32(1.0 - 0.9))
    sl = slices(H, n_in, E)
    assert np.array_equal(m[sl["lstm.bias_ih_l0"]].view(np.uint32), m[sl["lstm.bias_hh_l0"]].view(np.uint32))
    assert np.array_equal(v[sl["lstm.bias_ih_l0"]].view(np.uint32), v[sl["lstm.bias_hh_l0"]].view(np.uint32))
    bad = []
    for k in S.KEYS:
        g64 = c["g64"][k].reshape(-1)
        unit = max(c["yard"][k], FLOOR * np.abs(g64).max())
        dev_k = np.abs(g[sl[k]] - g64).max()
        ratio = dev_k / unit if unit > 0 else (0.0 if dev_k == 0 else np.inf)
        RATIOS[k] = max(RATIOS.get(k, 0.0), ratio)
        print(f"ratio {k} H={H} E={E} L={L} n={n}: {ratio:.3f} (dev {dev_k:.3e}, yardstick {c['yard'][k]:.3e}, max|g64| {np.abs(g64).max():.3e})")
        if not ratio <= 4.0:
            bad.append((k, ratio))
        # the second moment is the square of the same gradient
        np.testing.assert_allclose(v[sl[k]], (1.0 - 0.999) * (g[sl[k]] ** 2), rtol=1e-5, atol=1e-37)
    print("largest ratios so far:", {k: round(r, 3) for k, r in RATIOS.items()})
    assert not bad, bad


@pytest.mark.parametrize("H,n_in,E", S.SHAPES)
def test_update_is_adam_of_its_own_moments(dev, H, n_in, E):
    """With the moments read back, w1 is the float64 Adam formula applied to them within 2 ulp of |w0| + lr: at step 1 and at step 3."""
    c = S.case(H, n_in, E, 4, 17)
    eng = fresh(H, n_in, E, dev)
    lr = 1e-3
    for step in (1, 2, 3):
        w0 = eng.state()[0]
        eng.train([(c["x"], c["y"])], 1, lr=lr)
        w1, m, v = eng.state()
        assert eng.step.value == step
        if step == 2:
            continue
        want = S.adam_update(w0.astype(np.float64), m.astype(np.float64), v.astype(np.float64), step, lr)
        ulp = np.spacing((np.abs(w0) + np.float32(lr)).astype(np.float32)).astype(np.float64)
        worst = (np.abs(w1 - want) / ulp).max()
        print(f"step {step}: worst {worst:.3f} ulp")
        assert worst <= 2.0, (step, worst)
        assert not np.array_equal(w0, w1)


@pytest.mark.parametrize("H,n_in,E,L,n", CASES)
def test_forward_and_the_loss_of_a_step(dev, H, n_in, E, L, n):
    """mfas_surrogate_forward against surr64 within 4 x the float32 CPU module's own deviation (floor 2^-20); the loss a train step
    reports is the mean squared error of the predictions mfas_surrogate_forward gave before it (float64 mean, rounded once)."""
    c = S.case(H, n_in, E, L, n)
    eng = fresh(H, n_in, E, dev)
    pred = eng.forward(c["x"])
    assert pred.shape == (n,) and pred.dtype == np.float32
    devn = np.abs(pred.astype(np.float64) - c["pred64"]).max()
    print(f"forward H={H} L={L} n={n}: dev {devn:.3e}, cpu32 {c['pred_yard']:.3e}")
    assert devn <= 4.0 * max(c["pred_yard"], FLOOR)
    loss = eng.train([(c["x"], c["y"])], 1)
    mse = np.mean((pred.astype(np.float64) - c["y"].astype(np.float64)) ** 2)
    assert abs(np.float64(np.float32(loss)) - mse) <= np.spacing(np.float32(mse)), (loss, mse)


RUN = [(1, 17), (2, 65), (4, 15)]       # three buckets (L, n)


def run_buckets():
    return [S.draw_bucket(L, n, 77 + L) for L, n in RUN]


def test_state_carry_and_determinism(dev):
    """3 buckets x 4 epochs in one call and as four one-epoch calls passing `step` on: bit-identical parameters, moments and last
    loss; the same call twice from the same state is bit-identical (no atomics); a larger scratch changes nothing."""
    H, n_in, E = S.SHAPES[0]
    b = run_buckets()
    one = fresh(H, n_in, E, dev)
    l_one = one.train(b, 4)
    assert one.step.value == 12
    four = fresh(H, n_in, E, dev)
    for e in range(4):
        l_four = four.train(b, 1)
        assert four.step.value == 3 * (e + 1)
    again = fresh(H, n_in, E, dev)
    l_again = again.train(b, 4)
    roomy = fresh(H, n_in, E, dev, extra_scratch=(1 << 20) + 48)
    l_roomy = roomy.train(b, 4)
    for other, lo in ((four, l_four), (again, l_again), (roomy, l_roomy)):
        assert np.float32(lo).view(np.uint32) == np.float32(l_one).view(np.uint32)
        for a, bb in zip(one.state(), other.state()):
            assert np.array_equal(a.view(np.uint32), bb.view(np.uint32))
    assert np.isfinite(l_one) and not np.array_equal(one.state()[0], fresh(H, n_in, E, dev).state()[0])


def test_twelve_steps_stay_with_the_cpu_path(dev):
    """The 12-step run from the same state_dict: per-epoch losses (one-epoch calls: the loss of each epoch's last step) and the final
    predictions on 32 held-out configurations within 4 x the deviation the float32 CPU module shows from surr64 over the same run
    (never below the float32 rounding of the value itself, 2^-24 of it)."""
    from mfas_amd.search import surrogate as M
    H, n_in, E = S.SHAPES[0]
    b = run_buckets()
    held = S.draw_bucket(3, 32, 5)[0]
    # surr64
    p, state, l64, p64 = {k: v.astype(np.float64) for k, v in S.initial_state(H, n_in, E).items()}, None, [], None
    for _ in range(4):
        p, state, losses = S.train(p, b, 1, state)
        l64.append(losses[-1])
    p64 = S.forward(p, held)
    # the float32 CPU module
    cpu = S.module32(H, n_in, E)
    opt = torch.optim.Adam(cpu.parameters(), lr=1e-3)
    data = ([torch.from_numpy(x) for x, _ in b], [torch.from_numpy(y).reshape(-1, 1) for _, y in b])
    l32 = [M.train_simple_surrogate(cpu, torch.nn.MSELoss(), opt, data, 1, "cpu") for _ in range(4)]
    with torch.no_grad():
        p32 = cpu(torch.from_numpy(held)).numpy()[:, 0]
    # the engine
    eng = fresh(H, n_in, E, dev)
    le = [eng.train(b, 1) for _ in range(4)]
    pe = eng.forward(held)
    loss_unit = max(np.abs(np.array(l32) - np.array(l64)).max(), 2.0 ** -24 * max(l64))
    pred_unit = max(np.abs(p32 - p64).max(), 2.0 ** -24 * np.abs(p64).max())
    loss_dev, pred_dev = np.abs(np.array(le, np.float64) - np.array(l64)).max(), np.abs(pe - p64).max()
    print(f"losses: engine dev {loss_dev:.3e}, cpu32 dev {loss_unit:.3e}; predictions: engine dev {pred_dev:.3e}, cpu32 dev {pred_unit:.3e}")
    assert loss_dev <= 4.0 * loss_unit and pred_dev <= 4.0 * pred_unit


def test_module_trainer_and_batched_prediction(dev):
    """EngineSurrogate + train_simple_surrogate + tools.predict_accuracies_with_surrogate on 40 configurations of mixed length: the engine
    trainer is the one used, the nn.Parameters equal the flat buffer afterwards, eval_model agrees with the batched prediction, amsgrad
    is refused."""
    from mfas_amd.search import surrogate as M
    from mfas_amd.search import tools
    rng = np.random.default_rng(9)
    confs = [np.stack([rng.integers(0, 4, L), rng.integers(0, 4, L), rng.integers(0, 2, L)], 1) for L in rng.integers(1, 5, 40)]
    data = M.SurrogateDataloader()
    tools.update_surrogate_dataloader(data, confs, [float(a) for a in rng.uniform(0.2, 0.9, 40)])
    torch.manual_seed(2)
    model = M.EngineSurrogate(100, 3, 100).to(dev)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    args = SimpleNamespace(epochs_surrogate=5)
    loss = tools.train_surrogate(model, data, opt, torch.nn.MSELoss(), args, dev)
    tr = model._engine_trainer
    assert isinstance(tr, M.EngineSurrogateTrainer) and not hasattr(model, "_graphed_trainer")
    assert tr.step.value == 5 * len(data.get_data()[0]) and 0.0 < loss < 1.0 and not opt.state
    flat = torch.cat([model.state_dict()[k].reshape(-1) for k in S.KEYS])
    assert torch.equal(flat, tr.model._flat) and tr.model.flat_parameters() is tr.model._flat
    assert all(not torch.equal(before[k], model.state_dict()[k]) for k in S.KEYS)
    # the same data through the CPU module from the same start: same loss to float32 training round-off
    cpu = M.SimpleRecurrentSurrogate(100, 3, 100)
    cpu.load_state_dict({k: v.cpu() for k, v in before.items()})
    loss_cpu = tools.train_surrogate(cpu, data, torch.optim.Adam(cpu.parameters(), lr=1e-3), torch.nn.MSELoss(), args, "cpu")
    assert abs(loss - loss_cpu) < 1e-3
    preds = tools.predict_accuracies_with_surrogate(confs, model, dev)
    preds_cpu = tools.predict_accuracies_with_surrogate(confs, cpu, "cpu")
    assert np.abs(np.array(preds) - np.array(preds_cpu)).max() < 1e-3
    for i in (0, 7, 39):
        assert abs(float(model.eval_model(confs[i].astype(np.float32), dev)) - float(preds[i])) <= 2e-6
    # a second call keeps its optimizer state; loading a state_dict refreshes the flat copy
    tools.train_surrogate(model, data, opt, torch.nn.MSELoss(), args, dev)
    assert model._engine_trainer is tr and tr.step.value == 10 * len(data.get_data()[0])
    model.load_state_dict(before)
    back = tools.predict_accuracies_with_surrogate(confs[:4], model, dev)
    fresh_cpu = M.SimpleRecurrentSurrogate(100, 3, 100)
    fresh_cpu.load_state_dict({k: v.cpu() for k, v in before.items()})
    assert np.abs(np.array(back) - np.array(tools.predict_accuracies_with_surrogate(confs[:4], fresh_cpu, "cpu"))).max() < 1e-5
    # with grad enabled the forward is PyTorch's (an autograd graph), not the engine's
    out = model(torch.from_numpy(S.draw_bucket(2, 3, 1)[0]).to(dev))
    assert out.requires_grad
    with pytest.raises(ValueError):
        M.EngineSurrogateTrainer(model, torch.optim.Adam(model.parameters(), amsgrad=True))


def test_engine_surrogate_takes_the_pinned_controller_decisions(dev):
    """The reference-pinned controller runs of golden G9 (8 surrogate epochs) with EngineSurrogate: every sampled configuration of
    every call is the CPU path's.  On a mismatch the first differing decision is printed with both surrogates' predictions."""
    import mfas_amd as M
    from mfas_amd.search import EngineSurrogate, ModelSearcher, SimpleRecurrentSurrogate
    from mfas_amd.search import tools
    g = golden("g9_controller_run.npz")
    for tag, iters, levels, K in (("a", 2, 3, 5), ("b", 3, 4, 6)):
        args = SimpleNamespace(search_iterations=iters, max_progression_levels=levels, num_samples=K, initial_temperature=10.0,
                               final_temperature=0.2, temperature_decay=4.0, lr_surrogate=0.001, epochs_surrogate=8, verbose=False)

        def run(make, device):
            calls, preds = [], []

            def fake_train(confs, model_type, dataloaders, a, d, state_dict=None):
                calls.append([np.array(c) for c in confs])
                return [O.fake_accuracy(c) for c in confs]

            real = tools.predict_accuracies_with_surrogate

            def spy(confs, surrogate, d):
                out = real(confs, surrogate, d)
                preds.append((len(calls), [np.array(c) for c in confs], np.array(out)))
                return out

            np.random.seed(3)
            torch.manual_seed(3)
            random.seed(3)
            surrogate = make().to(device)
            tools.predict_accuracies_with_surrogate = spy
            try:
                s_data = ModelSearcher(args)._epnas(None, {"model": surrogate, "criterion": torch.nn.MSELoss()}, None,
                                                    {"train_sampled_fun": fake_train, "get_layer_confs": M.get_possible_layer_configurations},
                                                    device)
            finally:
                tools.predict_accuracies_with_surrogate = real
            return calls, preds, s_data

        calls, preds, s_data = run(lambda: EngineSurrogate(100, 3, 100), dev)
        flat = np.concatenate([np.concatenate([np.asarray(c).reshape(-1), [-1]]) for call in calls for c in call])
        if not np.array_equal(flat, g[tag + "/calls_flat"]):
            ccalls, cpreds, _ = run(lambda: SimpleRecurrentSurrogate(100, 3, 100), "cpu")
            for ci, (a, b) in enumerate(zip(calls, ccalls)):
                diff = [i for i, (u, v) in enumerate(zip(a, b)) if not np.array_equal(u, v)]
                if diff:
                    pe = [p for p in preds if p[0] == ci][-1:]
                    pc = [p for p in cpreds if p[0] == ci][-1:]
                    print(f"run {tag}: call {ci}, decision {diff[0]}: engine {a[diff[0]].tolist()} cpu {b[diff[0]].tolist()}")
                    if pe and pc:
                        worst = int(np.abs(pe[0][2] - pc[0][2]).argmax())
                        print("predictions before it: largest difference at", pe[0][1][worst].tolist(), float(pe[0][2][worst]), float(pc[0][2][worst]))
                    break
        assert np.array_equal(flat, g[tag + "/calls_flat"]), tag
        _, accs, _ = s_data.get_k_best(5)
        np.testing.assert_allclose(np.sort(np.array(accs)), g[tag + "/best_accs"], rtol=1e-12)


def test_search_cli_with_the_engine_surrogate(dev):
    """main_searchable_ntu --surrogate_device engine end to end at the sizes of the --surrogate_device gpu CLI test."""
    import main_searchable_ntu
    data = main_searchable_ntu.main(["--synthetic", "640", "320", "--epochs", "1", "--search_iterations", "1", "--max_fusions", "2",
                                     "--num_samples", "4", "--epochs_surrogate", "3", "--no-verbose", "--surrogate_device", "engine"])
    confs, accs, _ = data.get_k_best(3)
    assert len(confs) == 3 and all(0.0 <= a <= 1.0 for a in accs)
    assert all(np.asarray(c).shape[1] == 3 and 1 <= len(c) <= 2 for c in confs)
