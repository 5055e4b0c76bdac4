"""Case module: runs of the float32 oracle (one case, one step, several steps) that the CPU calibrations share.  (tests/helpers.py's
oracle_steps is the plain oracle loop; the one here takes the ref64 cases' arguments.)"""
import numpy as np

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import train_cases as GT


F32 = np.float32


# ------------------------------------------------------------------------------------------------ calibration on the GPU shapes
def oracle_case(case, dtype, seed=None, edit=None, batch_sum_term=False):
    """The float32 oracle and ref64 on exactly the inputs test_gpu_ref64 gives the engine: worst ratio per quantity.
    edit(conf, hp, p0, t, dtype) -> (p0, t): the parameters and the table changed before either side sees them
    (tests/test_inputs_cpu.py); batch_sum_term: ref64.forward's, for the train-mode pass."""
    hp = G.case_hyper(case)
    if seed is None:
        seed = 1000 + G.CASE_IDS.index(case[0]) if case[0] in G.CASE_IDS else 7
    conf, p0 = G.case_params(case, hp, seed)
    t = G.case_table(case, hp, G.N_EVAL, seed, dtype)
    if edit is not None:
        p0, t = edit(conf, hp, p0, t, dtype)
    out = {}
    f = G.feats_of(t)
    lg32, _ = O.forward({k: v.copy() for k, v in p0.items()}, conf, hp, f, False)
    lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
    out["forward"] = R64.worst_ratio(lg32, lg, Ml)[0]
    nb, step = hp.B, 3
    f = G.feats_of(t, 0, nb)
    p32 = {k: v.copy() for k, v in p0.items()}
    lg32, cache32 = O.forward(p32, conf, hp, f, True, seed=seed, step=step)
    lg, Ml, cache = R64.forward(p0, conf, hp, f, True, seed=seed, step=step, batch_sum_term=batch_sum_term)
    out["forward_train"] = R64.worst_ratio(lg32, lg, Ml)[0]
    rng = np.random.default_rng(seed)
    dl = (rng.standard_normal((nb, hp.C)) / nb).astype(F32)
    dl[rng.random((nb, hp.C)) < 0.1] *= F32(1e-3)
    g32 = O.backward(p32, hp, cache32, dl)
    G64, MG = R64.backward(p0, hp, cache, dl)
    out["backward"] = max(R64.worst_ratio(g32[k], G64[k], MG[k])[0] for k in g32)
    if hp.bn:
        O.bn_update_running(p32, hp, cache32)
        rs, Mrs = R64.running_stats(p0, hp, cache)
        out["running_stats"] = max(R64.worst_ratio(p32[k], rs[k], Mrs[k])[0] for k in rs)
    return out


TAUS = {"forward": G.TAU_LOGITS, "forward_train": G.TAU_LOGITS, "backward": G.TAU_GRAD, "running_stats": G.TAU_RUNSTAT}


class _PadMean(np.ndarray):
    """Activations whose batch mean also counts one padded row (mutation 'bn_pad'); results of arithmetic on them are plain."""
    _extra = None

    def mean(self, axis=None, dtype=None, **kw):
        m = np.asarray(self).mean(axis=axis, dtype=dtype, **kw)
        return m if self._extra is None else (m + self._extra).astype(F32)


def oracle_step32(st, conf, hp, batch, seed, step, eta, t, pw=None, mut="", stale=None):
    """One train step of the float32 oracle from state st = {"w", "m", "v"}; returns (state after, loss sum, count or None).
    mut names a deliberate error; stale: the parameters forward and backward read instead of st's (the running statistics and the
    update stay on st's)."""
    P = {k: v.copy() for k, v in st["w"].items()}
    Pf = P if stale is None else {k: v.copy() for k, v in stale.items()}
    n = len(batch["label"])
    feats = {k: v for k, v in batch.items() if k not in ("label", "multilabel")}
    orig_act = O._act
    if mut == "bn_pad":     # a row beyond nvalid (zero inputs: its activation is act(bias)) counted in the batch mean
        cell = [0]

        def act(y, nl):
            a = orig_act(y, nl).view(_PadMean)
            a._extra = orig_act(P[f"fusion_layers.{cell[0]}.0.bias"], nl) / F32(len(y))
            cell[0] += 1
            return a
        O._act = act
    try:
        logits, cache = O.forward(Pf, conf, hp, feats, True, seed=seed, step=step)
    finally:
        O._act = orig_act
    if hp.loss_mode == 1:
        loss, dlog = O.bce_loss(logits, batch["multilabel"], pw)
        if mut == "no_pos_weight":
            dlog = O.bce_loss(logits, batch["multilabel"], np.ones(hp.C, F32))[1]
        count = None
    else:
        loss, dlog, preds = O.ce_loss(logits, batch["label"])
        if hp.multitask:
            preds = O.predict(logits + feats["vlogit"] + feats["slogit"])
            loss = (loss + O.ce_loss(feats["vlogit"], batch["label"])[0]) + O.ce_loss(feats["slogit"], batch["label"])[0]
        count = int((preds == batch["label"]).sum())
    if mut == "div_B":
        dlog = (dlog * F32(n) / F32(hp.B)).astype(F32)
    grads = O.backward(Pf, hp, cache, dlog)
    O.bn_update_running(P, hp, cache)
    ad = O.AdamState(m={k: v.copy() for k, v in st["m"].items()}, v={k: v.copy() for k, v in st["v"].items()}, t=t - 1)
    hq = hp
    if mut == "no_wd":
        import dataclasses
        hq = dataclasses.replace(hp, wd=0.0)
    if mut == "m_no_decay":
        ad.m = {k: np.zeros_like(v) for k, v in ad.m.items()}
    O.adam_step(P, grads, ad, float(eta), hq, O.trainable_keys(conf, hp))
    return {"w": P, "m": ad.m, "v": ad.v}, float(loss) * n, count


def stale_taps(batch, stale):
    """`batch` with its tap columns replaced by the first rows of `stale` (labels and logits inputs stay the batch's own)."""
    n = len(batch["label"])
    return {k: (stale[k][:n] if k[0] in "sv" and k[1:].isdigit() else v) for k, v in batch.items()}


def oracle_steps(conf, hp, p0, t, order, etas, seed, steps, taus, tag, mut="", wrong=None, batch_sum_term=False, post=None):
    """The float32 oracle through steps 1..steps[-1] of one candidate (table t, sample order [EPOCHS][N], dropout seed), every
    step of `steps` checked against ref64 from the oracle's own state before it: worst ratio per quantity.
    post(j, prev, new, again) -> state: what step j leaves, changed before it is checked and carried on (again(state): the same
    step run from another state); tests/test_step_builds_cpu.py drops and repeats a tile's stores with it."""
    N = order.shape[1]
    pw = G.pos_weight(hp) if hp.loss_mode == 1 else None
    keys = O.trainable_keys(conf, hp)
    hist = [{"w": p0, "m": {k: np.zeros_like(p0[k]) for k in keys}, "v": {k: np.zeros_like(p0[k]) for k in keys}}]
    worst = {}
    nb = -(-N // hp.B)
    for j in range(1, steps[-1] + 1):
        batch, ep = GT.batch_of(t, order, hp.B, j)
        bi = (j - 1) % nb
        n = len(batch["label"])
        seen, eta_j, t_j, m, stale = batch, etas[j - 1], j, mut, None
        if mut == "div_B" and n == hp.B:
            m = ""                                  # (only the ragged batch divides by something else than B)
        if mut == "bn_pad" and n == hp.B:
            m = ""
        if mut == "scalars_prev" and j >= 2:
            eta_j, t_j = etas[j - 2], j - 1
        if mut == "stale_forward" and j >= 2:
            stale = hist[j - 2]["w"]
        if mut == "order_epoch0" and ep >= 1:
            seen = GT.batch_of(t, order, hp.B, j - ep * nb)[0]
        if mut == "order_other_candidate":
            seen = GT.batch_of(t, wrong, hp.B, j)[0]
        if mut == "stage_lag2" and bi >= 2:         # the staging buffer of batch bi was not refilled: it still holds batch bi - 2
            seen = stale_taps(batch, GT.batch_of(t, order, hp.B, j - 2)[0])
        if mut == "order_wrap2":                    # the order-table offset wraps after two batches
            idx = order[ep][(bi % 2) * hp.B:(bi % 2) * hp.B + n]
            seen = {k: v[idx] for k, v in t.items()}
        new, loss, count = oracle_step32(hist[-1], conf, hp, seen, seed, j - 1, eta_j, t_j, pw, m, stale)
        if post is not None:
            new = post(j, hist[-1], new, lambda st: oracle_step32(st, conf, hp, seen, seed, j - 1, eta_j, t_j, pw, m, stale)[0])
        if j in steps:
            exp = R64.train_step64(hist[-1], conf, hp, batch, seed, j - 1, etas[j - 1], j, G.TAU_LOGITS, GT.TAU_V, observed=new, pos_weight=pw,
                                     batch_sum_term=batch_sum_term)
            r = R64.check_train_step(exp, new, loss, count, taus, f"{tag} step {j}", hard=False)
            worst = {q: max(worst.get(q, 0.0), r[q]) for q in r}
        hist.append(new)
    return worst


def oracle_train_steps(case, dtype, mut="", seed=None, other_order=False, N=None, steps=(1, 2, 3), edit=None, batch_sum_term=False):
    """Steps of train() as test_gpu_train_ref64 sets them up (N rows: by default one full batch and the ragged one), the float32
    oracle checked step by step on `steps`: worst ratio per quantity.  edit: as in oracle_case."""
    hp = G.case_hyper(case)
    seed = GT.SEED0 + G.CASE_IDS.index(case[0]) if seed is None else seed
    conf, p0 = G.case_params(case, hp, seed)
    N = GT.train_rows(hp.B) if N is None else N
    t = G.case_table(case, hp, N, seed, dtype)
    if edit is not None:
        p0, t = edit(conf, hp, p0, t, dtype)
    order = GT.make_order(N, seed)
    wrong = GT.make_order(N, seed, 2)[1]            # another candidate's order
    return oracle_steps(conf, hp, p0, t, order, GT.step_etas(N, hp.B), seed, tuple(steps), GT.TAUS, case[0], mut, wrong,
                        batch_sum_term=batch_sum_term)


MUT_CE = ("mut", 32, 17, 20, G.W_A, [[3, 3, 0], [1, 2, 1]], True, 0.5, "")
