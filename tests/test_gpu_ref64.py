"""The single-pass entry points, the dev pass and a few train steps against the float64 reference (tests/ref64.py) across the
shape envelope the library accepts (R 1..512, C 1..128, B 2..64, tap widths 0..4100, f32 / bf16 / f16 tables).

Every comparison is elementwise, |got - ref64| <= tau * 2^-24 * M (ref64.assert_close64), with M the element's own magnitude:
a wrong padded row, ragged tail or small-gradient tile cannot hide under the tensor's maximum.  CASES is a covering design,
not a product: every value of every axis appears in at least two cases, paired differently
(tests/test_ref64_cpu.py::test_gpu_cases_cover_every_axis_value_twice checks that, and calibrates the taus on these shapes).

Run on its own, with a time limit:  python -m pytest tests/test_gpu_ref64.py -m gpu -x -q
"""
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64 as R64

pytestmark = pytest.mark.gpu

F32 = np.float32

# tau per quantity (units of 2^-24 * M).  The float32 oracle stays under a quarter of each on every case shape
# (test_ref64_cpu.py::test_float32_oracle_calibration_margin); each mutation in test_ref64_cpu.py exceeds it.
TAU_LOGITS = 6.0
TAU_GRAD = 20.0
TAU_RUNSTAT = 4.0

W_A = dict(s=(1, 8, 9, 15), v=(17, 63, 65, 1000))
W_B = dict(s=(2048, 4100, 1, 0), v=(8, 9, 15, 17))          # s3: an unused (width-0) tap slot
W_C = dict(s=(63, 65, 1000, 2048), v=(4100, 1, 8, 0))       # v3: an unused (width-0) tap slot

# (id, R, C, B, widths, cells, bn, drpt, extra)   extra: alphas / sig1 (sigma(alpha) = 1 in cell 0) / multitask / lm1 (loss_mode 1)
CASES = [
    ("r1a", 1, 1, 2, W_A, [[0, 0, 0], [1, 1, 1]], True, 0.0, ""),
    ("r1b", 1, 17, 3, W_B, [[2, 0, 2]], False, 0.5, ""),
    ("r16a", 16, 2, 33, W_C, [[0, 1, 0], [1, 2, 1], [2, 0, 2]], True, 0.9, ""),
    ("r16b", 16, 60, 20, W_A, [[3, 3, 1], [2, 2, 0], [0, 1, 2], [1, 0, 0]], True, 0.5, "alphas,sig1,multitask"),
    ("r17a", 17, 64, 64, W_B, [[0, 3, 0], [1, 1, 2]], False, 0.5, "lm1"),
    ("r17b", 17, 65, 17, W_C, [[3, 2, 1]], True, 0.0, ""),
    ("r32a", 32, 128, 20, W_A, [[1, 2, 0], [3, 0, 1]], True, 0.5, "alphas"),
    ("r32b", 32, 1, 33, W_B, [[2, 2, 2], [0, 0, 0]], True, 0.9, ""),
    ("r33a", 33, 2, 64, W_C, [[0, 0, 1], [2, 1, 0]], False, 0.5, "multitask"),
    ("r33b", 33, 60, 2, W_A, [[2, 3, 0]], True, 0.5, ""),
    ("r65a", 65, 64, 32, W_B, [[1, 2, 0], [2, 3, 1]], True, 0.0, ""),
    ("r65b", 65, 17, 3, W_C, [[1, 0, 2], [3, 2, 0], [0, 1, 1]], False, 0.9, "alphas,sig1"),
    ("r80a", 80, 65, 16, W_A, [[0, 3, 1], [3, 1, 0]], True, 0.5, "lm1"),
    ("r80b", 80, 1, 16, W_B, [[0, 1, 0]], False, 0.5, ""),
    ("r128a", 128, 128, 16, W_C, [[2, 2, 0], [0, 0, 1]], True, 0.5, ""),
    ("r128b", 128, 60, 17, W_A, [[1, 1, 0], [2, 2, 2], [3, 3, 0], [0, 0, 1]], True, 0.0, "multitask"),
    ("r129a", 129, 2, 20, W_B, [[1, 0, 1], [0, 2, 0]], True, 0.5, ""),
    ("r129b", 129, 64, 32, W_C, [[3, 0, 0]], False, 0.9, "lm1"),
    ("r256a", 256, 17, 16, W_A, [[3, 0, 0], [1, 3, 2]], True, 0.5, ""),
    ("r256b", 256, 60, 20, W_B, [[1, 3, 0]], False, 0.5, "alphas"),
    ("r257a", 257, 1, 2, W_C, [[1, 1, 0], [0, 2, 1]], True, 0.5, ""),
    ("r257b", 257, 65, 16, W_A, [[2, 1, 2]], True, 0.0, ""),
    ("r300", 300, 60, 16, W_A, [[3, 3, 0], [0, 1, 1]], True, 0.5, ""),
    ("r320a", 320, 128, 3, W_B, [[0, 2, 0], [2, 3, 0]], True, 0.9, ""),
    ("r320b", 320, 2, 17, W_C, [[2, 1, 1]], False, 0.5, "multitask"),
    ("r448a", 448, 17, 16, W_A, [[0, 2, 2], [1, 3, 0]], False, 0.5, ""),
    ("r448b", 448, 60, 2, W_B, [[1, 1, 0]], True, 0.5, "lm1"),
    ("r449a", 449, 1, 3, W_C, [[3, 0, 0], [1, 2, 1]], True, 0.5, ""),
    ("r449b", 449, 64, 16, W_A, [[1, 1, 1]], True, 0.0, ""),
    ("r512a", 512, 128, 16, W_B, [[0, 0, 0], [1, 1, 1]], True, 0.5, ""),
    ("r512b", 512, 2, 17, W_C, [[1, 2, 2]], False, 0.5, ""),
]
CASE_IDS = [c[0] for c in CASES]
DTYPES = ("float32", "bfloat16", "float16")
N_EVAL = 83


def case_hyper(case):
    _, R, C, B, w, cells, bn, drpt, extra = case
    return O.Hyper(R=R, C=C, B=B, bn=bn, drpt=drpt, alphas="alphas" in extra, multitask="multitask" in extra,
                   loss_mode=1 if "lm1" in extra else 0, s_sizes=w["s"], v_sizes=w["v"], epochs=1)


def case_params(case, hp, seed):
    conf = np.array(case[5])
    p = O.init_params(conf, hp, seed, perturb_bn=True)
    for k in p:     # every weight uses all 24 significand bits (a product build that drops low weight bits cannot match)
        if k.endswith("0.weight"):
            p[k] = (np.ascontiguousarray(p[k], F32).view(np.uint32) | np.uint32(1)).view(F32)
    if "sig1" in case[8]:
        p["alphas.0.alpha_x"] = np.array([40.0], F32)      # sigma(40) rounds to 1 in float32: the V columns drop out
    return conf, p


def dequant(a, dtype):
    """The values a table of `dtype` holds, as float32 (round to nearest even, like torch's conversion)."""
    a = np.asarray(a, F32)
    if dtype == "bfloat16":
        return O.bf16_round(a)
    if dtype == "float16":
        return a.astype(np.float16).astype(F32)
    return a


def case_table(case, hp, N, seed, dtype):
    """Synthetic taps (quantised to `dtype`), labels, multitask logits and multi-hot targets, as numpy."""
    t = O.synth_table(N, seed, snr=0.4, C=hp.C, s_sizes=hp.s_sizes, v_sizes=hp.v_sizes, with_logits=hp.multitask)
    for k in list(t):
        if k[0] in "sv" and k[1:].isdigit():
            t[k] = dequant(t[k], dtype)
    if hp.loss_mode == 1:
        t["multilabel"] = (O.hash_u01(seed + 77, N * hp.C).reshape(N, hp.C) < F32(0.2)).astype(F32)
    return t


def pos_weight(hp):
    return (F32(1.0) + F32(2.0) * O.hash_u01(991, hp.C)).astype(F32)


def feats_of(t, r0=0, n=None):
    n = len(t["label"]) - r0 if n is None else n
    return {k: v[r0:r0 + n] for k, v in t.items() if k not in ("label", "multilabel")}


def eval_me(hp):
    """Rows per dev-pass tile (mfas_hip.hip: the largest of 64 / 32 / 16 whose LDS tile fits 80 KiB)."""
    Rp, Cp = -(-hp.R // 16) * 16, -(-hp.C // 16) * 16
    for me in (64, 32, 16):
        if (me * max(128 + 8, Cp + 4) + me * (Rp + 8)) * 4 <= 80 * 1024:
            return me
    return 16


def eval_facts(hp):
    """What plan_layout hands the dev pass's choice of build (builds.hip.h: eval_key) for this geometry: batch tiles per workgroup,
    row blocks per wave (1, 2, 4, 8: three take the build for four, five to seven the one for eight), row blocks."""
    nrb = -(-hp.R // 16)
    nrbw = (nrb + 3) // 4
    nrbw = 4 if nrbw == 3 else (8 if 4 < nrbw < 8 else nrbw)
    return dict(mbe=eval_me(hp) // 16, nrbw=nrbw, nrb=nrb)


def eval_name(build):
    """A k_eval build written (MBE, NRBW, split, 16-bit rows, B3) by the name of its instantiation, k_eval<MBE, NRBW, MSP, XB, B3>:
    the bf16 x 3 build keeps its rows 16-bit by itself (XB is the split builds' argument)."""
    mbe, nrbw, split, x16, b3 = build
    return f"k_eval<{mbe},{nrbw},{split},{int(x16 and not b3)},{int(b3)}>"


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


# ------------------------------------------------------------------------------------------------ shared blocks
def eval_envs(hp):
    """The dev-pass builds the switches select at this R: the default one, and where the geometry has them the MFAS_EVAL_NO_* ones."""
    envs = [{}]
    if hp.R <= 32 or 65 <= hp.R <= 128:
        envs += [{"MFAS_EVAL_NO_MSPLIT": "1"}, {"MFAS_EVAL_NO_X16": "1"}, {"MFAS_EVAL_NO_B3": "1"}, {"MFAS_EVAL_NO_WL": "1"}]
    return envs


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


def dev_epoch_rows(B):
    """Rows of the train table of the one-epoch call: two full batches and a ragged one of at least two rows."""
    ntr = 2 * B + max(1, B // 2)
    return ntr + 1 if ntr % B == 1 else ntr


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_entry_points_vs_ref64(dev, case, dtype):
    """forward (eval) over ragged row ranges, forward_train + running statistics, backward of arbitrary dlogits, and one epoch of
    train() with a dev table, against ref64; then (f32, single-label) three train steps against the float32 oracle."""
    cid = case[0]
    hp = case_hyper(case)
    seed = 1000 + CASE_IDS.index(cid)
    conf, p0 = case_params(case, hp, seed)
    t = case_table(case, hp, N_EVAL, seed, dtype)
    tab = gpu_table(t, dtype, dev)
    pop = make_pop(hp, conf, dev, seed)
    pop.set_state_dict(0, p0)
    tag = f"{cid} R{hp.R} C{hp.C} B{hp.B} {dtype}"
    # 1. eval forward: every row range, every dev-pass build the switches select
    for env in eval_envs(hp):
        ep = pop if not env else make_pop(hp, conf, dev, seed, env=env)
        if env:
            ep.set_state_dict(0, p0)
        check_eval_forward(ep, hp, conf, p0, t, tab, tag, dtype, env)
        if env:
            ep.close()
    # 2. forward_train (+ running statistics) and backward of an arbitrary dL/dlogits
    check_train_passes(pop, dev, hp, conf, p0, t, tab, seed, tag, dtype)
    # 3. one epoch of train() with a dev table: the dev statistics on the engine's parameters after the call
    pop.set_state_dict(0, p0)
    ntr = dev_epoch_rows(hp.B)
    ttr = case_table(case, hp, ntr, seed + 1, dtype)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, -(-ntr // hp.B))
    stats, status = pop.train(gpu_table(ttr, dtype, dev), tab, 1, etas)
    assert not status.any(), (tag, status)
    check_dev(stats, state_np(pop), conf, hp, t, f"{tag} train E=1")
    pop.close()
    # 4. f32 tables, single-label head, no BatchNorm: three train steps against the float32 oracle (check_state).  (Under BN the
    #    batch mean removes the fusion bias's gradient: it is round-off sized, and Adam's first steps move such an element by +-lr
    #    whichever sign the round-off has — ref64 pins those gradients above, elementwise.)
    if dtype == "float32" and hp.loss_mode == 0 and not hp.bn:
        from tests.helpers import oracle_steps
        from tests.test_gpu_parity import check_state
        pop = make_pop(hp, conf, dev, seed)
        pop.set_state_dict(0, p0)
        stats, status = pop.train(gpu_table(ttr, dtype, dev), None, 2, O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / hp.B, 2 * -(-ntr // hp.B)),
                                  max_steps=3)
        assert not status.any(), (tag, status)
        params, st, _ = oracle_steps(conf, hp, {k: v.copy() for k, v in p0.items()}, ttr, 3, seed=seed)
        check_state(pop, 0, params, st, 3, tag=f"{tag} train steps")
        pop.close()


# One cell with an identity head (logits = the cell's activations): the feature products reach the output undiluted by the
# classifier's sum, so the bound sees them at the scale of one product.  bf16 tables at R = 72 .. 128 run the exact bf16 x 3 builds.
B3_CASES = [(80, [[0, 1, 0]]), (128, [[3, 1, 1]]), (72, [[2, 3, 2]]), (128, [[3, 3, 0]])]
TAU_ONE_LAYER = 16.0


def one_layer_setup(R, cells, seed, dtype):
    case = ("b3", R, R, 16, W_A, cells, False, 0.5, "")
    hp = case_hyper(case)
    conf, p = case_params(case, hp, seed)
    p["central_classifier.weight"] = np.eye(R, dtype=F32)
    p["central_classifier.bias"] = np.zeros(R, F32)
    return hp, conf, p, case_table(case, hp, N_EVAL, seed, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("R,cells", B3_CASES)
def test_one_layer_eval_products_vs_ref64(dev, R, cells, dtype):
    """The dev pass's feature products at the scale of one product (identity head), weights with all 24 significand bits: the
    default build (bf16 x 3 over bf16 tables) and the f32-product build both against ref64.  A product build that dropped the
    low 8 weight bits sits 35..180 x 2^-24 M away (test_ref64_cpu.py::test_mutation_b3_without_lo_term)."""
    hp, conf, p, t = one_layer_setup(R, cells, 77, dtype)
    tab = gpu_table(t, dtype, dev)
    lg, Ml, _ = R64.forward(p, conf, hp, feats_of(t), False)
    for env in ({}, {"MFAS_EVAL_NO_B3": "1"}):
        pop = make_pop(hp, conf, dev, 3, env=env)
        pop.set_state_dict(0, p)
        R64.assert_close64(pop.forward(0, tab).cpu().numpy(), lg, Ml, TAU_ONE_LAYER, f"one-layer R{R} {dtype} {env}",
                           record=f"forward_one_layer/{dtype}")
        pop.close()


SCHEDULES = {
    # name: (R, C, B, env, chunk_cols, K, check)
    "lean_chain": (16, 60, 20, {}, 0, 2, lambda s: s["lean_chain"] == 1),
    "general_mb1": (65, 60, 16, {"MFAS_CHAIN_SPLIT": "0"}, 0, 2, lambda s: s["lean_chain"] == 0 and s["chain_cus"] == 1),
    "general_mb2": (65, 17, 20, {}, 0, 2, lambda s: s["lean_chain"] == 0 and s["chain_cus"] == 1),
    "general_mb4": (33, 17, 64, {}, 0, 2, lambda s: s["lean_chain"] == 0 and s["chain_cus"] == 1),
    "same_group": (128, 60, 16, {"MFAS_SAME_GROUP": "2", "MFAS_CHAIN_SPLIT": "0"}, 128, 3,
                   lambda s: s["groups"] == -1 and s["chain_cus"] == 1),
    "chain_split": (128, 60, 16, {"MFAS_SAME_GROUP": "2"}, 128, 3, lambda s: s["groups"] == -1 and s["chain_cus"] == 4),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_train_schedules_dev_stats_vs_ref64(dev, name):
    """Each train schedule (lean chain, general chain at 1 / 2 / 4 m-blocks, the same-group launch, chain_split), asserted with
    pop.schedule(): one epoch with a dev table, every candidate's dev statistics against ref64 on its parameters after the call."""
    R, C, B, env, cc, K, check = SCHEDULES[name]
    hp = O.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, s_sizes=W_A["s"], v_sizes=W_A["v"], epochs=1)
    confs = [np.array(c) for c in ([[3, 3, 0], [1, 2, 1]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1], [1, 1, 0]])[:K]]
    from mfas_amd import Population
    from tests.helpers import engine_hyper
    os.environ.update(env)
    try:
        pop = Population(engine_hyper(hp), confs, dev, drop_seeds=list(range(5, 5 + K)), chunk_cols=cc)
    finally:
        for k in env:
            os.environ.pop(k, None)
    sched = pop.schedule()
    assert check(sched), (name, sched)
    for k, c in enumerate(confs):
        pop.set_state_dict(k, O.init_params(c, hp, 40 + k, perturb_bn=True))
    case = (name, R, C, B, W_A, None, True, 0.5, "")
    ntr = 5 * B + 3
    ttr, tdv = case_table(case, hp, ntr, 61, "bfloat16"), case_table(case, hp, N_EVAL, 62, "bfloat16")
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, ntr / B, -(-ntr // B))
    stats, status = pop.train(gpu_table(ttr, "bfloat16", dev), gpu_table(tdv, "bfloat16", dev), 1, etas)
    assert not status.any(), (name, status)
    for k, c in enumerate(confs):
        check_dev(stats[k:k + 1], state_np(pop, k), c, hp, tdv, f"{name} cand {k}")
    pop.close()


@pytest.mark.gpu
def test_width0_tap_slot(dev):
    """A width-0 tap is an unused slot: a configuration that selects it is refused at create; one that does not trains and
    evaluates with the empty tap present in the table (no pointer is needed for it)."""
    hp = O.Hyper(R=16, C=17, B=16, bn=True, drpt=0.5, s_sizes=W_B["s"], v_sizes=W_B["v"], epochs=1)
    with pytest.raises(RuntimeError, match="unused tap slot"):
        make_pop(hp, np.array([[3, 0, 0]]), dev, 1)
    case = ("w0", 16, 17, 16, W_B, [[2, 1, 0]], True, 0.5, "")
    conf, p0 = case_params(case, hp, 5)
    t = case_table(case, hp, N_EVAL, 5, "float32")
    assert t["s3"].shape == (N_EVAL, 0)
    tab = gpu_table(t, "float32", dev)
    pop = make_pop(hp, conf, dev, 5)
    pop.set_state_dict(0, p0)
    lg, Ml, _ = R64.forward(p0, conf, hp, feats_of(t), False)
    R64.assert_close64(pop.forward(0, tab).cpu().numpy(), lg, Ml, TAU_LOGITS, "width-0 slot forward")
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N_EVAL / 16, 6)
    stats, status = pop.train(tab, tab, 1, etas)
    assert not status.any()
    check_dev(stats, state_np(pop), conf, hp, t, "width-0 slot train")
    pop.close()
