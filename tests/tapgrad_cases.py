"""Case module of the tap-gradient tests (numpy, the oracle, tests/ref64.py and tests/tapgrad_ref64.py only): the cases the shape envelope
of tests/ref64_cases.py does not reach, the tau, and one cached reference per (case, dtype) that the CPU and the GPU tests share.

A case is a ref64_cases tuple (id, R, C, B, widths, cells, bn, drpt, extra) plus options: nrows (rows of the batch; default B), row0
(first table row), K / k (population size and the candidate asked; every candidate has the case's configuration, its own drop seed),
expect (what Population.schedule() must say, so that the case runs the plan it is named for)."""
import functools

import numpy as np

from tests import ref64 as R64
from tests import ref64_cases as G
from tests import tapgrad_ref64 as TG

F32 = np.float32

# |got - ref64| <= TAU_TAP * 2^-24 * M, the project's gradient tau; the float32 oracle-derived values stay under a quarter of it on every
# case below and on the envelope (tests/test_tapgrad_cpu.py, figures in its docstring)
TAU_TAP = G.TAU_GRAD

W_T = dict(s=(24, 17, 200, 9), v=(33, 16, 8, 20))
W_8 = dict(s=(8, 9, 15, 17, 24, 1, 16, 33), v=(16, 8, 9, 40, 1, 17, 15, 31))        # 8 + 8 slots
M3 = [[0, 1, 0], [0, 1, 1], [2, 1, 2]]          # s0 selected by two cells, v1 by three

TAP_CASES = [
    # the lean chain
    (("lean3", 16, 60, 20, W_T, M3, True, 0.5, ""), dict(expect=dict(lean_chain=1))),
    (("lean3a", 16, 60, 20, W_T, M3, True, 0.5, "alphas"), dict(expect=dict(lean_chain=1))),
    # the general chain: B = 16 without alphas is the chain_split geometry
    (("gen16", 128, 60, 16, W_T, M3, True, 0.5, ""), dict(expect=dict(lean_chain=0, wide=0, chain_cus=4))),
    (("gen16a", 128, 60, 16, W_T, M3, True, 0.0, "alphas"), dict(expect=dict(lean_chain=0, wide=0, chain_cus=1))),
    (("gen17a", 128, 17, 17, W_T, M3, False, 0.5, "alphas"), dict(expect=dict(lean_chain=0, wide=0))),
    (("gen17", 128, 17, 17, W_T, M3, True, 0.5, ""), dict(expect=dict(lean_chain=0, wide=0))),
    # wide plans
    (("wide64a", 65, 17, 64, W_T, M3, True, 0.5, "alphas"), dict(expect=dict(wide=1))),
    (("wide64", 65, 17, 64, W_T, M3, False, 0.5, ""), dict(expect=dict(wide=1))),
    (("wide128", 512, 60, 128, W_T, M3, True, 0.5, ""), dict(expect=dict(wide=1))),
    (("wide128a", 512, 7, 128, W_T, M3, True, 0.0, "alphas"), dict(expect=dict(wide=1))),
    # ragged batches, a row offset
    (("short", 16, 60, 20, W_T, M3, True, 0.5, "alphas"), dict(nrows=19)),
    (("short128", 128, 60, 16, W_T, M3, True, 0.5, ""), dict(nrows=15)),
    (("one", 128, 60, 16, W_T, M3, False, 0.5, "alphas"), dict(nrows=1)),
    (("row0", 33, 17, 20, W_T, M3, True, 0.5, "alphas"), dict(row0=7, nrows=20)),
    # candidate 1 of a population of three planned resident
    (("res_k1", 16, 60, 20, W_T, M3, True, 0.5, ""), dict(K=3, k=1, expect=dict(persistent=1))),
    # the same plans without BatchNorm: under BatchNorm ref64's M compounds from cell to cell (a dropped cell stays inside the tau at
    # R = 128), without it the rule sees a tap gradient at the scale of its own products — on every plan kind
    (("lean3n", 16, 60, 20, W_T, M3, False, 0.5, "alphas"), dict(expect=dict(lean_chain=1))),
    (("gen16n", 128, 60, 16, W_T, M3, False, 0.5, ""), dict(expect=dict(lean_chain=0, wide=0, chain_cus=4))),
    (("wide128n", 512, 60, 128, W_T, M3, False, 0.5, "alphas"), dict(expect=dict(wide=1))),
    (("res_k1n", 16, 60, 20, W_T, M3, False, 0.5, ""), dict(K=3, k=1, expect=dict(persistent=1))),
    # slot 7 of both modalities
    (("slot7", 32, 17, 16, W_8, [[7, 7, 0], [7, 3, 1], [0, 7, 2]], True, 0.5, "alphas"), {}),
]
TAP_CASE_IDS = [c[0][0] for c in TAP_CASES]
ENVELOPE = [(c, {}) for c in G.CASES]
ALL_CASES = ENVELOPE + TAP_CASES
ALL_IDS = G.CASE_IDS + TAP_CASE_IDS
STEP = 3


def case_seed(case):
    return 1000 + ALL_IDS.index(case[0])


def case_dlogits(hp, n, seed):
    """check_train_passes' recipe (tests/gpu_support.py): a spread of gradient sizes, small tiles held to their own scale."""
    rng = np.random.default_rng(seed)
    dl = (rng.standard_normal((n, hp.C)) / n).astype(F32)
    dl[rng.random((n, hp.C)) < 0.1] *= F32(1e-3)
    return dl


@functools.lru_cache(maxsize=None)
def _reference(cid, dtype):
    case, opts = ALL_CASES[ALL_IDS.index(cid)]
    hp = G.case_hyper(case)
    seed = case_seed(case)
    conf, p0 = G.case_params(case, hp, seed)
    t = G.case_table(case, hp, G.N_EVAL if hp.B <= G.N_EVAL else hp.B + 8, seed, dtype)
    row0, n = opts.get("row0", 0), opts.get("nrows", hp.B)
    k = opts.get("k", 0)
    f = G.feats_of(t, row0, n)
    lg, Ml, cache = R64.forward(p0, conf, hp, f, True, seed=seed + k, step=STEP)       # (gpu_support.make_pop: drop seed of candidate k)
    dl = case_dlogits(hp, n, seed)
    ref = TG.tap_grads(p0, conf, hp, cache, dl)
    for a in ref.values():
        for x in a:
            x.setflags(write=False)
    return dict(case=case, opts=opts, hp=hp, seed=seed, conf=conf, p0=p0, t=t, row0=row0, n=n, k=k, K=opts.get("K", 1), feats=f, cache=cache,
                dlogits=dl, ref=ref, logits=lg)


def reference(cid, dtype="float32"):
    """Everything a test needs of one case, computed once per process and left unchanged: hyper-parameters, configuration, parameters,
    table, the batch's rows, ref64's cache, dlogits and the expected tap gradients {tap: (value, M)}."""
    return _reference(cid, dtype)
