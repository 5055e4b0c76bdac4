"""Case module (numpy, the oracle and tests/ref64.py only): the shape envelope's case table, the taus, and the builders of
hyper-parameters, parameters and tables that the ref64 tests and their CPU calibrations share."""
import numpy as np

from oracle import np_oracle as O


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


# ------------------------------------------------------------------------------------------------ shared blocks
def eval_envs(hp):
    """The dev-pass builds the switches select at this R: the default one, and where the geometry has them the MFAS_EVAL_NO_* ones."""
    envs = [{}]
    if hp.R <= 32 or 65 <= hp.R <= 128:
        envs += [{"MFAS_EVAL_NO_MSPLIT": "1"}, {"MFAS_EVAL_NO_X16": "1"}, {"MFAS_EVAL_NO_B3": "1"}, {"MFAS_EVAL_NO_WL": "1"}]
    return envs


def dev_epoch_rows(B):
    """Rows of the train table of the one-epoch call: two full batches and a ragged one of at least two rows."""
    ntr = 2 * B + max(1, B // 2)
    return ntr + 1 if ntr % B == 1 else ntr


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
