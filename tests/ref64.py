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
  * batch sums (opt.)  batch_sum_term=True: M_mu = mean_b(M_a) + (n - 1) mean_b|a| and M_var += (n - 1) var, the rounding of the two
                       n-term float32 sums themselves at the depth of a serial sum (sound for any order); off by default, see forward()
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


def forward(params, conf, hp: "O.Hyper", feats, train: bool, seed: int = 0, step: int = 0, batch_sum_term: bool = False):
    """Returns (logits, M_logits, cache); feats: s0..s3 / v0..v3 (rows, width) as the values the engine reads (dequantised).
    batch_sum_term (train mode under BatchNorm only): M_mu = mean_b(M_a) counts the errors of the summed values, not the rounding of
    the batch sum itself.  Each of the n - 1 additions of a serial float32 sum rounds a partial sum of at most sum_b|a|, so the mean
    carries up to (n - 1) 2^-24 mean_b|a| more; a column whose values all lie near one number D (a ReLU behind a bias of +D,
    identical rows) has nothing else in M_mu of that size.  With the flag M_mu gains (n - 1) mean_b|a|, and M_var, M_xhat, the
    running mean's M and the backward follow from it.  n - 1 is the depth of a serial sum (how the numpy oracle adds rows), an
    upper bound for every summation order; the engine's own order is shallower.
    The batch variance's own sum has the analogous term: n non-negative terms (a - mu)^2 of mean var, each addition rounding a
    partial sum of at most n var, so M_var gains (n - 1) var.  It is KEPT, as part of the same flag.  The value-domain entries of
    tests/test_inputs_cpu.py calibrate without it (the float32 oracle's running statistics at 0.44 .. 0.83 of the allowed 1.0 on
    every flagged entry); the learning rate of 3e-2 in tests/test_axes_cpu.py does not: with the mean's term alone one of its
    twelve populations stays at 1.33 on a running variance, with both every one is at 0.60 or below (figures in that file)."""
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
                if batch_sum_term:
                    Mmu = Mmu + (n - 1.0) * np.abs(a).mean(0)
                Mvar = 2.0 * (np.abs(d) * (Ma + Mmu)).mean(0) + var
                if batch_sum_term:
                    Mvar = Mvar + (n - 1.0) * var
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


def backward(params, hp: "O.Hyper", cache, dlogits, M_dlogits=None):
    """Gradients of every central parameter for an arbitrary dL/dlogits.  Returns (grads, M_grads) keyed like the state dict.
    M_dlogits: the magnitude of dlogits' own error (a loss gradient formed from computed logits, ce_dlogits / bce_dlogits); it
    joins |dlogits| wherever that multiplies a forward quantity, which is sound because M_out >= |out| in every such product."""
    conf = cache["conf"]
    dl = _f(dlogits)
    adl = np.abs(dl) if M_dlogits is None else np.abs(dl) + _f(M_dlogits)
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


# ------------------------------------------------------------------------------------------------ one train step
# train() is pinned one step at a time: ref64 starts from the float32 state the engine (or the float32 oracle) itself held
# before the step, taken as exact inputs, so nothing Adam's sign-like first steps amplify is ever compared.
UNDERFLOW = 2.0 ** -126     # a float32 result below the smallest normal is rounded at 2^-149 absolute, or flushed to 0


def ce_dlogits(logits, Ml, labels, n, tau_logits):
    """dL/dlogits of the mean cross entropy over n rows, d = (softmax - onehot) / n, and its magnitude M_dl.
    A logit error |delta_i| <= tau_logits 2^-24 Ml_i moves s_j by at most s_j (|delta_j| + sum_i s_i |delta_i|); the argument of
    exp, x_j - max, is itself rounded at 2^-24 |x_j - max| (the same form, two roundings when it is scaled for exp2); exp, the
    row sum, the two divisions and the subtraction of the one-hot each round s_j or d_j once more."""
    lg, Ml = _f(logits), _f(Ml)
    mx = lg.max(1, keepdims=True)
    e = np.exp(lg - mx)
    s = e / e.sum(1, keepdims=True)
    d = s.copy()
    d[np.arange(len(lg)), labels] -= 1.0
    d /= n
    ax = np.abs(lg - mx)
    M = (tau_logits * s * (Ml + (s * Ml).sum(1, keepdims=True)) + 2.0 * s * (ax + (s * ax).sum(1, keepdims=True)) + 4.0 * s) / n \
        + 4.0 * np.abs(d)
    return d, M


def bce_dlogits(logits, Ml, z, w, n, C, tau_logits):
    """dL/dlogits of the weighted BCE-with-logits averaged over n rows and C classes, d = (-w z (1 - s) + (1 - z) s) / (n C),
    s = sigmoid(x), and its magnitude: the logit sensitivity s (1 - s) (w z + 1 - z) / (n C); s rounds a few times relative to
    itself, (1 - s) of a float32 s is exact only to 2^-24 absolute; the sum and the division round d itself."""
    lg, Ml, z, w = _f(logits), _f(Ml), _f(z), _f(w)
    s = _sig(lg)
    k = (w * z + (1.0 - z)) / (n * C)
    d = (-w * z * (1.0 - s) + (1.0 - z) * s) / (n * C)
    M = tau_logits * s * (1.0 - s) * k * Ml + 4.0 * k * (s + z * (1.0 - s)) + 4.0 * np.abs(d)
    return d, M


def adam_step64(w, m, v, g, Mg, scalars, hp: "O.Hyper", tau_v=1.0, m_new=None, v_new=None):
    """One Adam step with L2 weight decay (torch.optim.Adam, oracle/np_oracle.py adam_step) in float64 from the float32 state
    (w, m, v) and the float64 gradient g with magnitude Mg; scalars = (step size lr / (1 - beta1^t), sqrt(1 - beta2^t)).
    Returns ((m', M_m), (v', M_v), (w', M_w)):
      m' = m + (1 - b1) (g' - m), g' = g + wd w,   M_m carried through the same graph on absolute values;
      v' = b2 v + (1 - b2) g'^2.  With delta = tau_v 2^-24 M_g' the error of g', the allowance is (1 - b2)(2 |g'| delta + delta^2)
           plus the recurrence's own roundings (the float32 constants b2 and 1 - b2, then b2 v, (1 - b2) g', . g' and the sum:
           six of at most 2^-24 |v'| each, taken twice — where g' is tiny three of them act alone on all of v', and the rule
           must keep its x4 margin there) and the
           underflow floor; M_v is that allowance / 2^-24 (compare with tau 1);
      w' = w - ss m'/(sqrt(v')/bc2s + eps) evaluated on m_new / v_new when given (the float32 moments the implementation itself
           wrote: a pure elementwise function of them, so no cancellation enters), M_w = |w| + |dw|.
    Every allowance carries the underflow floor 2^-126 (absolute): a weight may be subnormal (wd w then underflows)."""
    w, m, v, g, Mg = _f(w), _f(m), _f(v), _f(g), _f(Mg)
    ss, bc2s = float(scalars[0]), float(scalars[1])
    b1, b2, wd = hp.beta1, hp.beta2, hp.wd
    g1 = g + wd * w
    Mg1 = Mg + wd * np.abs(w) + np.abs(g1)
    m1 = m + (1.0 - b1) * (g1 - m)
    Mm = np.abs(m) + (1.0 - b1) * (Mg1 + np.abs(m)) + np.abs(m1) + UNDERFLOW / U
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    delta = tau_v * U * Mg1
    Mv = ((1.0 - b2) * (2.0 * np.abs(g1) * delta + delta * delta) + UNDERFLOW) / U + 12.0 * np.abs(v1)
    mm = m1 if m_new is None else _f(m_new)
    vv = v1 if v_new is None else _f(v_new)
    dw = ss * mm / (np.sqrt(vv) / bc2s + hp.adam_eps)
    return (m1, Mm), (v1, Mv), (w - dw, np.abs(w) + np.abs(dw) + UNDERFLOW / U)


def train_step64(state, conf, hp: "O.Hyper", batch, seed, step, eta, t, tau_logits, tau_v, observed=None, pos_weight=None,
                 batch_sum_term=False):
    """One train step of one candidate in float64.  state = {"w": state dict (parameters and BN running statistics), "m": ..,
    "v": ..} is the float32 state before the step; batch holds the rows of this step in batch order (taps, label, and vlogit /
    slogit / multilabel where the head uses them): its length is the step's nvalid.  seed / step select the dropout masks (step =
    the global 0-based step), eta is this step's learning rate and t the 1-based Adam step.  observed = {"m": .., "v": ..}: the
    moments the implementation wrote, on which the expected parameters are evaluated.  batch_sum_term: as in forward().
    Returns {"m" / "v" / "w" / "runstat": {key: (expected, M)}, "loss": (sum over the rows, bound), "count": (lo, hi)}."""
    P = state["w"]
    n = len(batch["label"])
    feats = {k: a for k, a in batch.items() if k not in ("label", "multilabel")}
    lg, Ml, cache = forward(P, conf, hp, feats, True, seed=seed, step=step, batch_sum_term=batch_sum_term)
    if hp.loss_mode == 1:
        pw = np.ones(hp.C) if pos_weight is None else _f(pos_weight)
        dl, Mdl = bce_dlogits(lg, Ml, batch["multilabel"], pw, n, hp.C, tau_logits)
    else:
        dl, Mdl = ce_dlogits(lg, Ml, batch["label"], n, tau_logits)
    G, MG = backward(P, hp, cache, dl, M_dlogits=Mdl)
    out = {"m": {}, "v": {}, "w": {}}
    sc = O.adam_scalars(float(eta), int(t), hp)
    for key in O.trainable_keys(conf, hp):
        om = None if observed is None else observed["m"][key]
        ov = None if observed is None else observed["v"][key]
        em, ev, ew = adam_step64(P[key], state["m"][key], state["v"][key], G[key], MG[key], sc, hp, tau_v=tau_v, m_new=om, v_new=ov)
        out["m"][key], out["v"][key], out["w"][key] = em, ev, ew
    rs, Mrs = running_stats(P, hp, cache) if hp.bn else ({}, {})
    out["runstat"] = {k: (rs[k], Mrs[k]) for k in rs}
    loss, lb, lo, hi = dev_stats(lg, Ml, hp, tau_logits, labels=batch["label"], vlogit=feats.get("vlogit"), slogit=feats.get("slogit"),
                                 z=batch.get("multilabel"), pos_weight=pos_weight)
    out["loss"], out["count"] = (loss, lb), (lo, hi)
    return out


def check_train_step(exp, got, loss, count, taus, tag, rec=None, hard=True):
    """One observed step against train_step64's expectation.  got = {"w" / "m" / "v": state dict after the step} (running
    statistics in "w"); taus = {"m", "v", "w", "runstat", "loss"}.  Returns the worst ratio per quantity ("loss": the fraction of
    its bound, "count": 0 inside [lo, hi], else inf; count None: the head keeps no train count); hard: raise on the first quantity over its tau, naming the element.  rec: the
    suffix under which RATIOS records them (train_m/<rec> ...)."""
    worst = {}
    for q, src in (("m", "m"), ("v", "v"), ("w", "w"), ("runstat", "w")):
        r = 0.0
        for key, (ref, M) in exp[q].items():
            if hard:
                r = max(r, assert_close64(got[src][key], ref, M, taus[q], f"{tag} {q} {key}", record=f"train_{q}/{rec}" if rec else None))
            else:
                r = max(r, worst_ratio(got[src][key], ref, M)[0])
        worst[q] = r
    ref_loss, lb = exp["loss"]
    worst["loss"] = abs(float(loss) - ref_loss) / max(lb, 1e-300)
    lo, hi = exp["count"]
    worst["count"] = 0.0 if count is None or lo <= int(count) <= hi else float("inf")
    if rec:
        RATIOS[f"train_loss/{rec}"] = max(RATIOS.get(f"train_loss/{rec}", 0.0), worst["loss"])
    if hard:
        assert worst["loss"] <= taus["loss"], f"{tag} train_loss_sum: got {float(loss)!r}, ref64 {ref_loss!r}, bound {lb:.3g}"
        assert count is None or lo <= int(count) <= hi, f"{tag} train_corrects: got {int(count)}, ref64 allows [{lo}, {hi}]"
    return worst
