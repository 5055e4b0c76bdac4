"""surr64: a float64 numpy restatement of the search's LSTM surrogate (mfas_amd/search/surrogate.py: forward_unrolled), of the gradient
of its MSE loss by backpropagation through time, and of torch's Adam step — the reference the engine's surrogate kernels are held to
(tests/test_surrogate_engine_cpu.py checks it against torch autograd in float64; tests/test_gpu_surrogate_engine.py uses it on the GPU).

Parameters are a dict of float64 arrays under the module's state_dict names; KEYS is the flat order of the C ABI."""
import functools

import numpy as np

KEYS = ("embedding.0.weight", "embedding.0.bias", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
        "hid2val.weight", "hid2val.bias")
SHAPES = ((100, 3, 100), (24, 3, 40))      # (H, in, E); the second is no multiple of 16 in H nor E


def shapes_of(H, n_in, E):
    return {"embedding.0.weight": (E, n_in), "embedding.0.bias": (E,), "lstm.weight_ih_l0": (4 * H, E), "lstm.weight_hh_l0": (4 * H, H),
            "lstm.bias_ih_l0": (4 * H,), "lstm.bias_hh_l0": (4 * H,), "hid2val.weight": (1, H), "hid2val.bias": (1,)}


def flatten(params, dtype=np.float64):
    return np.concatenate([np.asarray(params[k], dtype).reshape(-1) for k in KEYS])


def unflatten(flat, H, n_in, E):
    out, off = {}, 0
    for k, shp in shapes_of(H, n_in, E).items():
        size = int(np.prod(shp))
        out[k] = np.asarray(flat[off:off + size], np.float64).reshape(shp)
        off += size
    assert off == len(flat)
    return out


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def forward(p, x, keep=None):
    """x (L, n, in) -> predictions (n,).  keep: a list that receives what the backward pass needs, per step."""
    x = np.asarray(x, np.float64)
    L, n, _ = x.shape
    H = p["lstm.weight_hh_l0"].shape[1]
    h = np.zeros((n, H))
    c = np.zeros((n, H))
    for t in range(L):
        e = _sig(x[t] @ p["embedding.0.weight"].T + p["embedding.0.bias"])
        gates = e @ p["lstm.weight_ih_l0"].T + p["lstm.bias_ih_l0"] + h @ p["lstm.weight_hh_l0"].T + p["lstm.bias_hh_l0"]
        i, f, g, o = _sig(gates[:, :H]), _sig(gates[:, H:2 * H]), np.tanh(gates[:, 2 * H:3 * H]), _sig(gates[:, 3 * H:])
        c_new = f * c + i * g
        h_new = o * np.tanh(c_new)
        if keep is not None:
            keep.append((e, i, f, g, o, c, c_new, h))
        h, c = h_new, c_new
    pred = _sig(h @ p["hid2val.weight"][0] + p["hid2val.bias"][0])
    if keep is not None:
        keep.append(h)
    return pred


def loss_and_grad(p, x, y):
    """(mean((pred - y)^2), gradient of it for every parameter, predictions): nn.MSELoss + backward."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    L, n, _ = x.shape
    H = p["lstm.weight_hh_l0"].shape[1]
    keep = []
    pred = forward(p, x, keep)
    err = pred - y
    g = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in p.items()}
    dz = (2.0 * err / n) * pred * (1.0 - pred)
    h_last = keep[-1]
    g["hid2val.weight"][0] = dz @ h_last
    g["hid2val.bias"][0] = dz.sum()
    dh = np.outer(dz, p["hid2val.weight"][0])
    dc = np.zeros((n, H))
    for t in range(L - 1, -1, -1):
        e, i, f, gg, o, c_prev, c, h_prev = keep[t]
        tc = np.tanh(c)
        dc = dc + dh * o * (1.0 - tc * tc)
        dgates = np.concatenate([dc * gg * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - gg * gg), dh * tc * o * (1.0 - o)], 1)
        dc = dc * f
        g["lstm.weight_ih_l0"] += dgates.T @ e
        g["lstm.weight_hh_l0"] += dgates.T @ h_prev
        g["lstm.bias_ih_l0"] += dgates.sum(0)
        g["lstm.bias_hh_l0"] += dgates.sum(0)
        dh = dgates @ p["lstm.weight_hh_l0"]
        dpre = (dgates @ p["lstm.weight_ih_l0"]) * e * (1.0 - e)
        g["embedding.0.weight"] += dpre.T @ x[t]
        g["embedding.0.bias"] += dpre.sum(0)
    return float(np.mean(err * err)), g, pred


def adam_update(w, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The parameter update of torch.optim.Adam from moments that already hold this step's gradient (step counts from 1)."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return w - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)


def adam_step(w, m, v, g, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """One torch.optim.Adam step on flat float64 arrays: (w, m, v) after step number `step` (1 for the first)."""
    g = g + weight_decay * w
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    return adam_update(w, m, v, step, lr, beta1, beta2, eps), m, v


def train(p, buckets, epochs, state=None, **adam):
    """train_simple_surrogate in float64: `epochs` passes over buckets [(x, y)], one Adam step per bucket.  Returns the parameters, the
    optimizer state (m, v, steps) and every step's loss (computed before its update)."""
    H, n_in, E = p["lstm.weight_hh_l0"].shape[1], p["embedding.0.weight"].shape[1], p["embedding.0.weight"].shape[0]
    w = flatten(p)
    m, v, steps = (np.zeros_like(w), np.zeros_like(w), 0) if state is None else state
    losses = []
    for _ in range(epochs):
        for x, y in buckets:
            loss, g, _ = loss_and_grad(unflatten(w, H, n_in, E), x, y)
            steps += 1
            w, m, v = adam_step(w, m, v, flatten(g), steps, **adam)
            losses.append(loss)
    return unflatten(w, H, n_in, E), (m, v, steps), losses


# ---- shared inputs and the float32 yardstick --------------------------------------------------------------------------------
def draw_bucket(L, n, seed):
    """x (L, n, 3) float32 from the configuration grid (s, v in 0..3, nl in 0..1), y (n,) float32 from U(0.2, 0.9)."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, 4, (L, n)), rng.integers(0, 4, (L, n)), rng.integers(0, 2, (L, n))], 2).astype(np.float32)
    return x, rng.uniform(0.2, 0.9, n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def initial_state(H, n_in, E, seed=11):
    """state_dict (float32 numpy) of a freshly initialised SimpleRecurrentSurrogate(H, n_in, E)."""
    import torch
    from mfas_amd.search.surrogate import SimpleRecurrentSurrogate
    gen = torch.random.get_rng_state()
    torch.manual_seed(seed)
    sd = {k: v.numpy().copy() for k, v in SimpleRecurrentSurrogate(H, n_in, E).state_dict().items()}
    torch.random.set_rng_state(gen)
    return sd


def module32(H, n_in, E, sd=None):
    import torch
    from mfas_amd.search.surrogate import SimpleRecurrentSurrogate
    m = SimpleRecurrentSurrogate(H, n_in, E)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in (sd or initial_state(H, n_in, E)).items()})
    return m


@functools.lru_cache(maxsize=None)
def case(H, n_in, E, L, n):
    """One (shape, L, n) case, computed once per process: the inputs, surr64's loss / gradient / predictions, and the YARDSTICK —
    how far the float32 CPU module (nn.LSTM forward, autograd) is from surr64 on the same inputs: per tensor the largest gradient
    deviation, and the largest prediction deviation."""
    import torch
    x, y = draw_bucket(L, n, 1000 * L + n)
    p64 = {k: v.astype(np.float64) for k, v in initial_state(H, n_in, E).items()}
    loss64, g64, pred64 = loss_and_grad(p64, x, y)
    m = module32(H, n_in, E)
    out = m(torch.from_numpy(x))
    torch.nn.MSELoss()(out, torch.from_numpy(y).reshape(-1, 1)).backward()
    g32 = {k: q.grad.numpy().astype(np.float64) for k, q in m.named_parameters()}
    return {"x": x, "y": y, "p64": p64, "loss64": loss64, "g64": g64, "pred64": pred64, "g32": g32,
            "yard": {k: float(np.abs(g32[k] - g64[k]).max()) for k in KEYS},
            "pred_yard": float(np.abs(out.detach().numpy()[:, 0].astype(np.float64) - pred64).max())}
