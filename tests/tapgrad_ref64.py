"""Float64 reference of the TAP gradients of one train-mode batch, d loss / d tap = sum_i scale_i * d_y_i @ W_i[:, tap columns], with an
elementwise magnitude — derived from tests/ref64.py without a second statement of the backward.

ref64.backward does not return d_y, but its weight gradient is d_y^T @ c["x"] with magnitude M_dy^T @ c["Mx"]: run on a copy of the
cache whose x and Mx are the n x n identity it returns d_y^T and M_dy^T of every cell (recover_dy).  Nothing else in that backward
reads x.  The same trick on oracle/np_oracle.py's backward gives the float32 statement the tolerance is calibrated with.

Magnitude of a tap gradient element:  sum_i scale_i * M_dy_i @ |W_i[:, cols]| + |value|   (V under alphas: (1 - sg) + 1 for the scale,
as ref64.forward does: 1 - sigma of a float32 sigma is exact only to 2^-24 absolute).

torch_tap_grads is the independent statement: the chain restated in float64 torch with ref64's dropout masks injected and taps that
require grad, differentiated by torch.autograd.
"""
import numpy as np

from oracle import np_oracle as O
from tests import ref64 as R64

F64 = np.float64


def _identity_cache(cache, n, dtype):
    eye = np.eye(n, dtype=dtype)
    cells = [dict(c, x=eye, Mx=eye) for c in cache["cells"]]
    return dict(cache, cells=cells)


def recover_dy(params, hp, cache, dlogits, M_dlogits=None):
    """[(d_y_i, M_dy_i)] of every cell, (n, R) each, from ref64.backward on the identity-input copy of the cache (M_dlogits: its)."""
    n = np.asarray(dlogits).shape[0]
    G, M = R64.backward(params, hp, _identity_cache(cache, n, F64), dlogits, M_dlogits=M_dlogits)
    return [(G[f"fusion_layers.{i}.0.weight"].T, M[f"fusion_layers.{i}.0.weight"].T) for i in range(len(cache["conf"]))]


def recover_dy32(params, hp, cache32, dlogits):
    """The float32 oracle's d_y_i of every cell, by the same trick on np_oracle.backward (d_y^T @ I is exact)."""
    n = np.asarray(dlogits).shape[0]
    g = O.backward(params, hp, _identity_cache(cache32, n, np.float32), dlogits)
    return [g[f"fusion_layers.{i}.0.weight"].T for i in range(len(cache32["conf"]))]


def tap_columns(conf, hp, i, name):
    """(first column, width) of tap `name` inside cell i's weight, or None when the cell does not select it: [ske | vis | prev]."""
    sj, vj = int(conf[i][0]), int(conf[i][1])
    ws, wv = int(hp.s_sizes[sj]), int(hp.v_sizes[vj])
    if name == f"s{sj}":
        return 0, ws
    if name == f"v{vj}":
        return ws, wv
    return None


def used_taps(conf):
    return sorted({f"s{int(c[0])}" for c in conf}) + sorted({f"v{int(c[1])}" for c in conf})


def tap_grads(params, conf, hp, cache, dlogits, taps=None, mutate=None, M_dlogits=None):
    """{tap: (gradient (n, width), M)} in float64.  taps: names (default: every tap the configuration selects; a tap no cell
    selects gets zeros).  mutate: a deliberate error, for the tests that show the tolerance catches it — "no_alpha" (scale dropped),
    "drop_second" (the second using cell's contribution dropped), "shift_block" (column offset + 16), "v_scale_for_s".  M_dlogits: the
    magnitude of dlogits' own error (ref64.backward's), for a loss gradient formed from computed logits."""
    dys = recover_dy(params, hp, cache, dlogits, M_dlogits)
    n = dys[0][0].shape[0]
    out = {}
    for name in (used_taps(conf) if taps is None else taps):
        width = int((hp.s_sizes if name[0] == "s" else hp.v_sizes)[int(name[1:])])
        g, M = np.zeros((n, width), F64), np.zeros((n, width), F64)
        seen = 0
        for i in range(len(conf)):
            cols = tap_columns(conf, hp, i, name)
            if cols is None:
                continue
            seen += 1
            if mutate == "drop_second" and seen == 2:
                continue
            c0, w = cols
            W = np.asarray(params[f"fusion_layers.{i}.0.weight"], F64)
            if mutate == "shift_block":
                c0 = min(c0 + 16, W.shape[1] - w)
            sc = Msc = 1.0
            if hp.alphas:
                sg = cache["cells"][i]["sg"]
                is_s = name[0] == "s"
                if mutate == "v_scale_for_s":
                    is_s = False
                sc = sg if is_s else 1.0 - sg
                Msc = sg if is_s else (1.0 - sg) + 1.0
                if mutate == "no_alpha":
                    sc = 1.0
            d_y, M_dy = dys[i]
            g += sc * (d_y @ W[:, c0:c0 + w])
            M += Msc * (M_dy @ np.abs(W[:, c0:c0 + w]))
        out[name] = (g, M + np.abs(g))
    return out


def tap_grads32(params, conf, hp, cache32, dlogits, taps=None):
    """The float32 statement (calibration): the same sum in float32 on the float32 oracle's d_y, each cell's product rounded, scaled and
    added in ascending cell order."""
    F32 = np.float32
    dys = recover_dy32(params, hp, cache32, dlogits)
    n = dys[0].shape[0]
    out = {}
    for name in (used_taps(conf) if taps is None else taps):
        width = int((hp.s_sizes if name[0] == "s" else hp.v_sizes)[int(name[1:])])
        g = np.zeros((n, width), F32)
        for i in range(len(conf)):
            cols = tap_columns(conf, hp, i, name)
            if cols is None:
                continue
            c0, w = cols
            W = np.asarray(params[f"fusion_layers.{i}.0.weight"], F32)
            prod = (dys[i].astype(F32) @ W[:, c0:c0 + w]).astype(F32)
            if hp.alphas:
                sg = F32(cache32["cells"][i]["sg"])
                prod = (prod * (sg if name[0] == "s" else F32(1.0) - sg)).astype(F32)
            g = (g + prod).astype(F32)
        out[name] = g
    return out


# ------------------------------------------------------------------------------------------------ the independent statement
def torch_tap_grads(params, conf, hp, feats, dlogits, cache):
    """The train-mode chain restated in float64 torch — Linear, activation, batch-statistics BatchNorm, dropout with ref64's own masks
    (cache["cells"][i]["keep"]) — on taps that are leaves requiring grad; returns {tap: d (sum(logits * dlogits)) / d tap} by
    torch.autograd for every tap the configuration selects."""
    import torch
    t64 = lambda a: torch.from_numpy(np.asarray(a, F64).copy())     # noqa: E731
    leaves = {name: t64(feats[name]).requires_grad_(True) for name in used_taps(conf)}
    out = None
    for i in range(len(conf)):
        s, v = leaves[f"s{int(conf[i][0])}"], leaves[f"v{int(conf[i][1])}"]
        if hp.alphas:
            sg = torch.sigmoid(t64(params[f"alphas.{i}.alpha_x"]))[0]
            s, v = s * sg, v * (1.0 - sg)
        x = torch.cat([s, v] if i == 0 else [s, v, out], 1)
        y = x @ t64(params[f"fusion_layers.{i}.0.weight"]).T + t64(params[f"fusion_layers.{i}.0.bias"])
        nl = int(conf[i][2])
        a = torch.relu(y) if nl == 0 else (torch.sigmoid(y) if nl == 1 else torch.nn.functional.leaky_relu(y, 0.01))
        if hp.bn:
            mu = a.mean(0)
            var = ((a - mu) ** 2).mean(0)
            a = (a - mu) / torch.sqrt(var + hp.bn_eps) * t64(params[f"fusion_layers.{i}.2.weight"]) + t64(params[f"fusion_layers.{i}.2.bias"])
        c = cache["cells"][i]
        if "keep" in c:
            a = torch.where(torch.from_numpy(np.asarray(c["keep"])), a * float(c["scale"]), torch.zeros_like(a))
        out = a
    logits = out @ t64(params["central_classifier.weight"]).T + t64(params["central_classifier.bias"])
    (logits * t64(dlogits)).sum().backward()
    return {name: leaf.grad.numpy() for name, leaf in leaves.items()}, logits.detach().numpy()
