"""Device plumbing of the ref64 tests: tables and populations on the GPU, the entry-point checks against tests/ref64.py, and the `dev`
fixture that prints the worst observed ratios at teardown.  Re-exports tests/ref64_cases.py, so that one alias serves both."""
import os

import numpy as np
import pytest

from tests.ref64_cases import *  # noqa: F401,F403  (one alias serves a consumer for the cases and the plumbing)
from tests import ref64 as R64


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _torch():
    import torch
    return torch


def gpu_table(t, dtype, dev):
    torch = _torch()
    from mfas_amd.engine import TAPS, FeatureTable
    dt = getattr(torch, dtype)
    taps = {k: torch.from_numpy(np.ascontiguousarray(t[k])).to(dev).to(dt) for k in TAPS if k in t}
    lab = torch.from_numpy(t["label"].astype(np.int32)).to(dev)
    opt = {k: torch.from_numpy(t[k]).to(dev) for k in ("vlogit", "slogit", "multilabel") if k in t}
    return FeatureTable(taps, lab, **opt)


def make_pop(hp, conf, dev, seed, env=None, chunk_cols=0, K=1):
    from mfas_amd import Population
    from tests.helpers import engine_hyper
    env = env or {}
    os.environ.update(env)
    try:
        pop = Population(engine_hyper(hp), [conf] * K, dev, drop_seeds=[seed + k for k in range(K)], chunk_cols=chunk_cols)
    finally:
        for k in env:
            os.environ.pop(k, None)
    if hp.loss_mode == 1:
        pop.set_pos_weight(pos_weight(hp))
    return pop


def state_np(pop, k=0, plane=0):
    return {key: v.numpy() for key, v in pop.get_state_dict(k, plane).items()}


def check_dev(stats, P, conf, hp, t, tag):
    """dev_loss_sum and dev_corrects of one epoch against ref64 on the engine's own parameters after the call."""
    f = feats_of(t)
    lg, Ml, _ = R64.forward(P, conf, hp, f, False)
    loss, lb, lo, hi = R64.dev_stats(lg, Ml, hp, TAU_LOGITS, labels=t["label"], vlogit=f.get("vlogit"), slogit=f.get("slogit"),
                                     z=t.get("multilabel"), pos_weight=pos_weight(hp))
    got_loss, got_cnt = float(stats["dev_loss_sum"].ravel()[0]), int(stats["dev_corrects"].ravel()[0])
    assert abs(got_loss - loss) <= lb, f"{tag} dev_loss_sum: got {got_loss!r}, ref64 {loss!r}, bound {lb:.3g}"
    assert lo <= got_cnt <= hi, f"{tag} dev_corrects: got {got_cnt}, ref64 allows [{lo}, {hi}]"
    key = "dev_loss/" + ("lm1" if hp.loss_mode else "ce")         # (recorded as the fraction of the bound used)
    R64.RATIOS[key] = max(R64.RATIOS.get(key, 0.0), abs(got_loss - loss) / max(lb, 1e-300))


@pytest.fixture(scope="module")
def dev():
    torch = _torch()
    assert torch.cuda.is_available(), "needs a HIP device"
    yield torch.device("cuda:0")
    if R64.RATIOS:      # the observed worst ratios, per entry point and dtype (printed with -s; kept for the PR record)
        print("\nworst |got - ref64| / (2^-24 M):")
        for k in sorted(R64.RATIOS):
            print(f"  {k:40s} {R64.RATIOS[k]:.4g}")


def check_eval_forward(ep, hp, conf, p0, t, tab, tag, rec, env=None, k=0):
    """forward (eval) of candidate k over the ragged row ranges {1, ME - 1, ME + 1, N_EVAL - row0} at row0 = 0 and 5: the logits
    elementwise against ref64, the count (rows, or the 32.32 fixed-point F1 sum) inside [lo, hi]."""
    ME = eval_me(hp)
    for row0 in (0, 5):
        for nrows in sorted({1, ME - 1, ME + 1, N_EVAL - row0}):
            got, corr = ep.forward(k, tab, row0=row0, nrows=nrows, count=True)
            f = feats_of(t, row0, nrows)
            lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
            R64.assert_close64(got.cpu().numpy(), lg, Ml, TAU_LOGITS, f"{tag} forward rows {row0}+{nrows} {env or ''}",
                               record=f"forward/{rec}")
            if hp.loss_mode == 0:
                _, _, lo, hi = R64.dev_stats(lg, Ml, hp, TAU_LOGITS, labels=t["label"][row0:row0 + nrows],
                                             vlogit=f.get("vlogit"), slogit=f.get("slogit"))
                assert lo <= corr <= hi, f"{tag} forward count rows {row0}+{nrows} {env}: {corr} not in [{lo}, {hi}]"
            else:       # the multi-label head counts F1-samples in 32.32 fixed point
                _, _, lo, hi = R64.dev_stats(lg, Ml, hp, TAU_LOGITS, z=t["multilabel"][row0:row0 + nrows], pos_weight=pos_weight(hp))
                assert lo <= corr <= hi, f"{tag} forward F1 sum rows {row0}+{nrows} {env}: {corr} not in [{lo}, {hi}]"


def check_train_passes(pop, dev, hp, conf, p0, t, tab, seed, tag, rec, k=0, drop_seed=None, tau_runstat=None, batch_sum_term=False):
    """forward_train of the first B rows (+ the running statistics it leaves) and backward of an arbitrary dL/dlogits, candidate k
    against ref64 (batch_sum_term: ref64.forward's).  Returns ref64's cache of that forward."""
    torch = _torch()
    nb = hp.B
    step = 3
    f = feats_of(t, 0, nb)
    got = pop.forward_train(k, tab, 0, nb, step=step).cpu().numpy()
    lg, Ml, cache = R64.forward(p0, conf, hp, f, True, seed=seed if drop_seed is None else drop_seed, step=step,
                                batch_sum_term=batch_sum_term)
    R64.assert_close64(got, lg, Ml, TAU_LOGITS, f"{tag} forward_train", record=f"forward_train/{rec}")
    if hp.bn:
        rs, Mrs = R64.running_stats(p0, hp, cache)
        sd = state_np(pop, k)
        for key in rs:
            R64.assert_close64(sd[key], rs[key], Mrs[key], TAU_RUNSTAT if tau_runstat is None else tau_runstat,
                               f"{tag} forward_train {key}", record=f"running_stats/{rec}")
    pop.set_state_dict(k, p0)
    rng = np.random.default_rng(seed)
    dl = (rng.standard_normal((nb, hp.C)) / nb).astype(F32)
    dl[rng.random((nb, hp.C)) < 0.1] *= F32(1e-3)         # a spread of gradient sizes: small tiles are held to their own scale
    from mfas_amd.engine import flat_layout
    flat = pop.backward(k, tab, torch.from_numpy(dl).to(dev), 0, nb, step=step).cpu().numpy()
    G, MG = R64.backward(p0, hp, cache, dl)
    layout, _ = flat_layout(conf, hp)
    for key, shape, off in layout:
        if key in G:
            R64.assert_close64(flat[off:off + int(np.prod(shape))].reshape(shape), G[key], MG[key], TAU_GRAD, f"{tag} backward {key}",
                               record=f"backward/{rec}")
    return cache
