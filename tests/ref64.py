"""Float64 reference of one candidate, with an elementwise error scale for every output.

TEST INFRASTRUCTURE ONLY (nothing under ``mfas_amd/`` imports it).  It restates the arithmetic of ``oracle/np_oracle.py``
(eval / train forward, CE, the multitask 3-term loss, weighted BCE, F1-at-threshold, backward from an arbitrary dL/dlogits,
the BN running-statistic update) in float64 throughout, and runs the same graph a second time on absolute values to give
every output element a magnitude ``M``: what a float32 evaluation of that element can have lost to rounding is a small
multiple of ``2^-24 * M`` whatever order it sums in.  The comparison rule is elementwise,

    |got - ref64| <= tau * 2^-24 * M,

so a small element (a padded row, a ragged tail, a tile with small gradients) is held to its own scale, not to the
tensor's maximum.  Dropout masks come from ``O.dropout_keep``: bit-identical to the engine's and the float32 oracle's.

Magnitudes:
  * linear layer       M_y = M_x @ |W|^T + |b|          (M_x >= |x|: a table value is exact, a previous output carries its M)
  * activation         M_a = slope * M_y + c |a|        (ReLU slope 1, c 0; LeakyReLU 1, 1; Sigmoid 1/4, 4: its own rounding)
  * BN (eval)          M_z = |gamma| * rstd * (M_a + |running_mean|) + |beta| + |z|
  * BN (train)         as eval with the batch mean, plus the batch-mean term mean_b(M_a) and the variance's share
  * dropout            M_z * keep * scale
  * weight gradients   M_dW = M_dy^T @ M_x              (the spec's |dy|^T |a|, with forward errors carried in M_x)
An element at an activation kink (|y| within the bound of 0) may take either branch: its gradient gets an O(1) allowance.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from oracle import np_oracle as O

F64 = np.float64
U = 2.0 ** -24          # float32 unit round-off
KINK_TAU = 64.0         # |y| <= KINK_TAU * U * M_y: the activation branch of that element is not decided by float32 arithmetic


def _f(a):
    return np.asarray(a, F64)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(params, conf, hp: "O.Hyper", feats, train: bool, seed: int = 0, step: int = 0):
    """Returns (logits, M_logits, cache); feats: s0..s3 / v0..v3 (rows, width) as the values the engine reads (dequantised)."""
    L = len(conf)
    cells = []
    out = M_out = None
    for i in range(L):
        s = _f(feats[f"s{int(conf[i][0])}"])
        v = _f(feats[f"v{int(conf[i][1])}"])
        c = {"s_raw": s, "v_raw": v}
        Ms, Mv = np.abs(s), np.abs(v)
        if hp.alphas:
            sg = float(_sig(_f(params[f"alphas.{i}.alpha_x"])[0]))
            c["sg"] = sg
            s, v = s * sg, v * (1.0 - sg)
            # (1 - sigma) of a float32 sigma is exact only to 2^-24 absolute: at sigma(alpha) = 1 the V columns vanish in float32
            Ms, Mv = Ms * sg, Mv * ((1.0 - sg) + 1.0)
        parts, mparts = [s, v], [Ms, Mv]
        if i > 0:
            parts.append(out)
            mparts.append(M_out)
        x, Mx = np.concatenate(parts, 1), np.concatenate(mparts, 1)
        W, b = _f(params[f"fusion_layers.{i}.0.weight"]), _f(params[f"fusion_layers.{i}.0.bias"])
        y = x @ W.T + b
        My = Mx @ np.abs(W).T + np.abs(b)
        nl = int(conf[i][2])
        if nl == 0:
            a, Ma = np.maximum(y, 0.0), My                          # (exact in float32)
        elif nl == 1:
            a = _sig(y)
            Ma = 0.25 * My + 4.0 * np.abs(a)                        # (exp and a division: a few ulp of its own)
        else:
            a = np.where(y > 0, y, 0.01 * y)
            Ma = My + np.abs(a)
        c.update(x=x, Mx=Mx, y=y, My=My, a=a, Ma=Ma, nl=nl, W=W)
        z, Mz = a, Ma
        if hp.bn:
            g, be = _f(params[f"fusion_layers.{i}.2.weight"]), _f(params[f"fusion_layers.{i}.2.bias"])
            if train:
                n = a.shape[0]
                mu = a.mean(0)
                d = a - mu
                var = (d * d).mean(0)
                rstd = 1.0 / np.sqrt(var + hp.bn_eps)
                xhat = d * rstd
                Mmu = Ma.mean(0)
                Mvar = 2.0 * (np.abs(d) * (Ma + Mmu)).mean(0) + var
                # xhat = d * rstd: d's error (M_a + M_mu) and rstd's relative error (half the variance's)
                Mxhat = rstd * (Ma + Mmu) + np.abs(xhat) * (0.5 * Mvar / (var + hp.bn_eps)) + np.abs(xhat)
                c.update(mu=mu, var=var, rstd=rstd, xhat=xhat, Mxhat=Mxhat, Mmu=Mmu, Mvar=Mvar, n=n, g=g)
            else:
                rm, rv = _f(params[f"fusion_layers.{i}.2.running_mean"]), _f(params[f"fusion_layers.{i}.2.running_var"])
                rstd = 1.0 / np.sqrt(rv + hp.bn_eps)
                xhat = (a - rm) * rstd
                Mxhat = rstd * (Ma + np.abs(rm)) + np.abs(xhat)
            z = xhat * g + be
            Mz = Mxhat * np.abs(g) + np.abs(be) + np.abs(z)
        if train and hp.use_dropout:
            keep = O.dropout_keep(seed, step, i, z.shape[0], hp.R, hp.drpt)
            scale = 1.0 / (1.0 - hp.drpt)
            c.update(keep=keep, scale=scale)
            z = np.where(keep, z * scale, 0.0)
            Mz = np.where(keep, Mz * scale, 0.0)
        out, M_out = z, Mz
        cells.append(c)
    Wc, bc = _f(params["central_classifier.weight"]), _f(params["central_classifier.bias"])
    logits = out @ Wc.T + bc
    Ml = M_out @ np.abs(Wc).T + np.abs(bc)
    return logits, Ml, {"cells": cells, "conf": conf, "out": out, "M_out": M_out, "Wc": Wc}


def backward(params, hp: "O.Hyper", cache, dlogits):
    """Gradients of every central parameter for an arbitrary dL/dlogits.  Returns (grads, M_grads) keyed like the state dict."""
    conf = cache["conf"]
    dl = _f(dlogits)
    adl = np.abs(dl)
    G, M = {}, {}
    G["central_classifier.weight"] = dl.T @ cache["out"]
    M["central_classifier.weight"] = adl.T @ cache["M_out"]
    G["central_classifier.bias"] = dl.sum(0)
    M["central_classifier.bias"] = adl.sum(0)
    d_o = dl @ cache["Wc"]
    M_do = adl @ np.abs(cache["Wc"])
    for i in range(len(conf) - 1, -1, -1):
        c = cache["cells"][i]
        d_z, M_dz = d_o, M_do
        if "keep" in c:
            d_z = np.where(c["keep"], d_z * c["scale"], 0.0)
            M_dz = np.where(c["keep"], M_dz * c["scale"], 0.0)
        if hp.bn:
            n, g, xhat, Mxhat = c["n"], c["g"], c["xhat"], c["Mxhat"]
            dgamma = (d_z * xhat).sum(0)
            dbeta = d_z.sum(0)
            G[f"fusion_layers.{i}.2.weight"] = dgamma
            G[f"fusion_layers.{i}.2.bias"] = dbeta
            M_dgamma = (M_dz * np.abs(xhat) + np.abs(d_z) * Mxhat).sum(0)
            M_dbeta = M_dz.sum(0)
            M[f"fusion_layers.{i}.2.weight"] = M_dgamma
            M[f"fusion_layers.{i}.2.bias"] = M_dbeta
            d_a = (g * c["rstd"]) * (d_z - dbeta / n - xhat * (dgamma / n))
            # rstd's relative error (from the forward's variance) scales the whole bracket
            rel_rstd = 0.5 * c["Mvar"] / (c["var"] + hp.bn_eps)
            br = np.abs(d_z) + np.abs(dbeta) / n + np.abs(xhat) * np.abs(dgamma) / n
            M_da = np.abs(g) * c["rstd"] * (M_dz + M_dbeta / n + Mxhat * np.abs(dgamma) / n + np.abs(xhat) * M_dgamma / n
                                             + br * rel_rstd) + np.abs(d_a)
        else:
            d_a, M_da = d_z, M_dz
        nl, y, My = c["nl"], c["y"], c["My"]
        kink = np.abs(y) <= KINK_TAU * U * My
        if nl == 0:
            d_y = np.where(y > 0, d_a, 0.0)
            M_dy = np.where(y > 0, M_da, 0.0)
        elif nl == 1:
            a = c["a"]
            d_y = d_a * (1.0 - a) * a
            M_dy = 0.25 * M_da + np.abs(d_a) * c["Ma"] + np.abs(d_y)
            kink = np.zeros_like(kink)
        else:
            d_y = np.where(y > 0, d_a, 0.01 * d_a)
            M_dy = np.where(y > 0, M_da, 0.01 * M_da)
        # (a kink element may take either branch: allow its whole gradient, |d_a| <= 1 * (2^24 |d_a|) * 2^-24)
        M_dy = M_dy + np.where(kink, np.abs(d_a) / U, 0.0)
        G[f"fusion_layers.{i}.0.weight"] = d_y.T @ c["x"]
        M[f"fusion_layers.{i}.0.weight"] = M_dy.T @ c["Mx"]
        G[f"fusion_layers.{i}.0.bias"] = d_y.sum(0)
        M[f"fusion_layers.{i}.0.bias"] = M_dy.sum(0)
        if hp.alphas or i > 0:
            d_x = d_y @ c["W"]
            M_dx = M_dy @ np.abs(c["W"])
        if hp.alphas:
            ns, nv = c["s_raw"].shape[1], c["v_raw"].shape[1]
            sg = c["sg"]
            dsg = (d_x[:, :ns] * c["s_raw"]).sum() - (d_x[:, ns:ns + nv] * c["v_raw"]).sum()
            Mdsg = (M_dx[:, :ns] * np.abs(c["s_raw"])).sum() + (M_dx[:, ns:ns + nv] * np.abs(c["v_raw"])).sum()
            G[f"alphas.{i}.alpha_x"] = np.array([dsg * sg * (1.0 - sg)])
            M[f"alphas.{i}.alpha_x"] = np.array([(Mdsg + abs(dsg)) * sg * (1.0 - sg) + abs(dsg) * sg])   # (same (1 - sigma))
        if i > 0:
            d_o, M_do = d_x[:, -hp.R:], M_dx[:, -hp.R:]
    return G, M


def running_stats(params, hp: "O.Hyper", cache):
    """BN running statistics after one train-mode forward (unbiased variance, momentum), with their magnitudes."""
    out, M = {}, {}
    mom = hp.bn_momentum
    for i, c in enumerate(cache["cells"]):
        if "mu" not in c:
            continue
        n = c["n"]
        rm, rv = _f(params[f"fusion_layers.{i}.2.running_mean"]), _f(params[f"fusion_layers.{i}.2.running_var"])
        ub = c["var"] * n / (n - 1.0)
        out[f"fusion_layers.{i}.2.running_mean"] = rm + mom * (c["mu"] - rm)
        out[f"fusion_layers.{i}.2.running_var"] = rv + mom * (ub - rv)
        M[f"fusion_layers.{i}.2.running_mean"] = np.abs(rm) + mom * (c["Mmu"] + np.abs(c["mu"]) + np.abs(rm))
        M[f"fusion_layers.{i}.2.running_var"] = np.abs(rv) + mom * (c["Mvar"] * n / (n - 1.0) + ub + np.abs(rv))
    return out, M


# ------------------------------------------------------------------------------------------------ losses and dev metrics
def ce_rows(logits, labels):
    """Per-row cross entropy, float64.  (Its logit sensitivity: |dCE/dlogit|_1 <= 2.)"""
    lg = _f(logits)
    mx = lg.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(1))
    return lse - lg[np.arange(len(lg)), labels]


def ce_loss(logits, labels):
    return float(ce_rows(logits, labels).mean())


def multitask_loss(logits, vlogit, slogit, labels):
    """train_searchable/ntu.py:60-61: CE(central) + CE(visual) + CE(skeleton)."""
    return ce_loss(logits, labels) + ce_loss(vlogit, labels) + ce_loss(slogit, labels)


def bce_rows(logits, z, w):
    """Weighted BCE-with-logits summed over classes per row / C (models/central/mm_imdb.py:655-673), float64."""
    lg, z, w = _f(logits), _f(z), _f(w)
    # -log(sigmoid(x)) = softplus(-x), -log(1 - sigmoid(x)) = softplus(x)
    sp_neg = np.logaddexp(0.0, -lg)
    sp_pos = np.logaddexp(0.0, lg)
    return (w * z * sp_neg + (1.0 - z) * sp_pos).mean(1)


def bce_loss(logits, z, w):
    return float(bce_rows(logits, z, w).mean())


def f1_rows(logits, z, th):
    pr = _sig(_f(logits)) > th
    tr = _f(z) > 0.5
    tp = (pr & tr).sum(1)
    den = pr.sum(1) + tr.sum(1)
    return np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)


def dev_stats(logits, Ml, hp: "O.Hyper", tau: float, labels=None, vlogit=None, slogit=None, z=None, pos_weight=None):
    """What one dev pass over these rows must report, with its allowance:
    (loss_sum, loss_bound, count_lo, count_hi) — count in rows (loss_mode 0) or in 32.32 fixed-point F1 (loss_mode 1).
    A row is ambiguous when its decision is within the logit bound of flipping; it may then go either way."""
    lg = _f(logits)
    bnd = tau * U * np.asarray(Ml, F64)                    # per-element logit bound
    rowb = bnd.max(1)
    n = len(lg)
    if hp.loss_mode == 1:
        w = np.ones(hp.C) if pos_weight is None else _f(pos_weight)
        rows = bce_rows(lg, z, w)
        # |dBCE_row/dlogit_c| <= max(w_c, 1) / C; the float32 loss itself rounds at a few u of its terms
        lb = (np.maximum(w, 1.0)[None, :] * bnd).mean(1) + 64 * U * (rows + 1.0)
        f1 = f1_rows(lg, z, hp.f1_threshold)
        th_logit = math.log(hp.f1_threshold / (1.0 - hp.f1_threshold))
        amb = (np.abs(lg - th_logit) <= bnd + 4 * U * (np.abs(lg) + abs(th_logit))).any(1)
        one = float(1 << 32)
        base = float(np.floor(f1[~amb] * one).sum())
        return float(rows.sum()), float(lb.sum()), base - n, base + one * amb.sum() + n     # (+- 1 per row: the fixed-point floor)
    rows = ce_rows(lg, labels)
    lb = 2.0 * rowb + 64 * U * (rows + 1.0)
    dec = lg
    decb = rowb
    if hp.multitask:
        rows = rows + ce_rows(vlogit, labels) + ce_rows(slogit, labels)
        lb = lb + 64 * U * (rows + 1.0)
        dec = lg + _f(vlogit) + _f(slogit)
        decb = rowb + 4 * U * np.abs(dec).max(1)
    order = np.argsort(-dec, 1, kind="stable")
    top, second = dec[np.arange(n), order[:, 0]], dec[np.arange(n), order[:, 1]] if dec.shape[1] > 1 else np.full(n, -np.inf)
    amb = (top - second) <= 2.0 * decb + 4 * U * np.abs(top)
    correct = order[:, 0] == labels
    lo = int((correct & ~amb).sum())
    return float(rows.sum()), float(lb.sum()), lo, lo + int(amb.sum())


# ------------------------------------------------------------------------------------------------ the comparison rule
def worst_ratio(got, ref, M):
    """max_i |got_i - ref_i| / (2^-24 M_i), with the element that attains it (index tuple)."""
    got, ref, M = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(M, F64)
    assert got.shape == ref.shape == M.shape, (got.shape, ref.shape, M.shape)
    if got.size == 0:
        return 0.0, ()
    err = np.abs(got - ref)
    r = np.where(err == 0, 0.0, err / np.maximum(U * M, 1e-300))
    r = np.where(np.isfinite(got), r, np.inf)
    j = int(np.argmax(r))
    return float(r.flat[j]), np.unravel_index(j, r.shape)


RATIOS: Dict[str, float] = {}       # tag -> worst ratio seen (per process; the GPU test module prints its table)


def assert_close64(got, ref, M, tau: float, tag: str, record: Optional[str] = None):
    """|got - ref| <= tau * 2^-24 * M elementwise; on failure, the worst element (row, column), its values and M."""
    r, idx = worst_ratio(got, ref, M)
    key = record or tag
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    if not r <= tau:
        g, f, m = (float(np.asarray(a, F64)[idx]) for a in (got, ref, M))
        raise AssertionError(f"{tag}: worst |got - ref64| = {r:.3g} * 2^-24 * M > tau = {tau:g} at element {tuple(int(i) for i in idx)}"
                             f" (got {g!r}, ref64 {f!r}, M {m:.4g})")
    return r
