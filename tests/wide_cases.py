"""Case module: the wide-batch / wide-width case table with its taus, seeds and input builders."""
from tests import ref64_cases as G
from tests import train_cases as GT
from tests.ref64_cases import W_A, W_B, W_C


# (id, R, C, B, widths, cells of candidate 0, bn, drpt, extra, table dtype)
WIDE_CASES = [
    ("w65", 65, 17, 64, W_A, [[0, 3, 0], [2, 1, 1]], True, 0.5, "", "float32"),
    ("w80", 80, 60, 33, W_B, [[1, 2, 0], [0, 1, 2]], False, 0.5, "lm1", "bfloat16"),
    # (R = 128 at B = 64 was accepted — eight row blocks need no k-split slabs; R = 177 is the smallest width from there on whose
    #  OUT unit, 64 * (3 * 192 + 36) * 4 = 156,672 B, no longer fits: the refused neighbour of the headline width)
    ("w177", 177, 60, 64, W_C, [[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 0, 0]], True, 0.5, "multitask", "float16"),
    ("w256", 256, 60, 64, W_A, [[3, 0, 0], [1, 3, 2]], False, 0.5, "alphas,sig1", "float32"),
    ("w512a", 512, 2, 20, W_B, [[2, 0, 0]], True, 0.0, "", "bfloat16"),
    ("w512b", 512, 128, 64, W_C, [[1, 2, 0], [3, 1, 1]], True, 0.5, "", "float16"),
    ("wc", 33, 256, 64, W_A, [[2, 3, 0], [0, 1, 1]], False, 0.5, "lm1", "float32"),
    ("wb65", 16, 60, 65, W_B, [[0, 1, 0], [1, 3, 1], [2, 2, 2]], True, 0.5, "", "bfloat16"),
    ("wb100", 17, 65, 100, W_C, [[3, 2, 1], [0, 0, 0]], True, 0.9, "", "float16"),
    ("wb128", 129, 64, 128, W_A, [[1, 1, 0]], True, 0.5, "multitask", "bfloat16"),
]
WIDE_IDS = [c[0] for c in WIDE_CASES]
PER_CANDIDATE = ("w177", "wb100")        # the cases that also run with per-candidate sample orders
# candidates 1 and 2: other cell counts (tap slots 0..2 only: every width set has them)
POOL = {1: [[0, 1, 2]], 2: [[2, 1, 1], [1, 2, 0]], 3: [[1, 0, 0], [2, 2, 1], [0, 1, 0]], 4: [[0, 0, 1], [1, 1, 0], [2, 2, 2], [0, 2, 0]]}
K = 3
SEED0 = 5000
# Per-case taus where the float32 oracle itself exceeds a quarter of the project's tau on the case's shape
# (tests/test_wide_cpu.py::test_wide_float32_oracle_calibration_margin): four times the oracle's measured maximum, rounded up.
# {case: {quantity: (tau, measured)}}; quantities: forward / forward_train / backward / running_stats, train steps m / v / w / runstat / loss
CASE_TAUS = {
    "w512a": {"train_runstat": (6, 1.313)},
    "wb128": {"running_stats": (5, 1.239), "train_runstat": (5, 1.005)},
}


def case_taus(cid):
    """(taus of the single passes, taus of the train steps) for a case."""
    single = {"forward": G.TAU_LOGITS, "forward_train": G.TAU_LOGITS, "backward": G.TAU_GRAD, "running_stats": G.TAU_RUNSTAT}
    train = dict(GT.TAUS)
    for q, (tau, _) in CASE_TAUS.get(cid, {}).items():
        if q.startswith("train_"):
            train[q[len("train_"):]] = float(tau)
        else:
            single[q] = float(tau)
    return single, train


def base_case(case, cells=None):
    """The 9-tuple test_gpu_ref64's helpers take."""
    return case[:5] + (case[5] if cells is None else cells,) + case[6:9]


def case_confs(case):
    others = [n for n in (1, 2, 3, 4) if n != len(case[5])][:K - 1]
    return [case[5]] + [POOL[n] for n in others]


def ceil16(x):
    return -(-x // 16) * 16


def pick_chunk(cols_p, target):
    return max([c for c in range(16, min(cols_p, target) + 1, 16) if cols_p % c == 0] or [16])


def legacy_refusal(case, confs):
    """Why mfas_population_create refused this geometry before the wide path: 'B>64', 'C_padded' or 'lds' (the LDS need of the
    step, the streaming sweep units and the general chain, over 150 KiB), else None.  A restatement of the validator's two rules and
    of plan_layout's lds_step for the launch-per-phase schedule with the general chain (none of the cases has a lean chain)."""
    _, R, C, B, w, _, bn, drpt, extra, _ = case
    Rp, Cp = ceil16(R), ceil16(C)
    MB = -(-B // 16)
    MB = 4 if MB == 3 else MB
    Bp, nrb = 16 * MB, Rp // 16
    if B > 64:
        return "B>64"
    if Cp > 8 * min(16, 512 // Bp):
        return "C_padded"
    assert not (nrb == 1 and Cp <= 64 and MB <= 2), "lean chain: not restated here"
    cols = [(ceil16(w["s"][c[0]]), ceil16(w["v"][c[1]])) for conf in confs for c in conf]
    tot_cols = sum(a + b for a, b in cols)
    lds_max = 64
    while Bp * (8 * lds_max + 20) * 4 <= 72 * 1024 and lds_max < 1024:
        lds_max *= 2
    target = 64
    while target * nrb < 64 * 16 and target < lds_max:
        target *= 2
    while target > 64 and tot_cols / target < 320.0:
        target //= 2
    if nrb >= 8:
        target = min(target, 64 if len(confs) >= 28 else 256)
    ls = 0
    for a, b in cols:                                   # feature units (k-split reduction slabs below eight row blocks)
        for cp in (a, b):
            cc = pick_chunk(cp, target)
            ls = max(ls, Bp * (cc + 16) + Bp * (cc + 4) + Bp * (Rp + 16) + (8 * nrb * MB * 256 if nrb < 8 else 0))
    if any(len(conf) > 1 for conf in confs):            # OUT units: the whole Rp x Rp block
        ls = max(ls, Bp * (Rp + 16) + Bp * (Rp + 4) + Bp * (Rp + 16))
    ls = max(ls, Bp * (Rp + 16) + Bp * (Rp + 4) + Bp * (Cp + 16))     # HEAD
    ls *= 4
    base = (2 * Bp * (Rp + 4) + Bp * (Cp + 4) + 4 * Rp + 3 * Bp + 16) * 4
    yf = (2 if "alphas" in extra else 1) * 4 * nrb * MB * 256 * 4
    lds_step = max(ls, base + (yf if base + yf <= max(ls, 64 * 1024) else 0))
    return "lds" if lds_step > 150 * 1024 else None


def case_inputs(case, order_mode="shared"):
    """What a wide case trains, as numpy (no device): hyper-parameters, the K candidates with their initial parameters and seeds."""
    from tests.helpers import engine_hyper
    hp = G.case_hyper(base_case(case))
    seed = SEED0 + WIDE_IDS.index(case[0])
    confs, p0s = [], []
    for k, cells in enumerate(case_confs(case)):
        conf, p0 = G.case_params(base_case(case, cells), hp, seed + 10 * k)
        confs.append(conf)
        p0s.append(p0)
    ehp = engine_hyper(hp)
    ehp.order_per_candidate = order_mode == "per_candidate"
    seeds = [seed + 3 * k for k in range(K)]
    return hp, ehp, seed, confs, p0s, seeds


def train_inputs(case, hp, ehp, seed, full=1):
    """The train table of `full` full batches and a ragged one, the sample order and the learning rates of a wide case."""
    N = GT.train_rows(hp.B, full)
    assert 2 <= N - full * hp.B <= hp.B - 1
    t = G.case_table(base_case(case), hp, N, seed, case[9])
    return N, t, GT.make_order(N, seed, K if ehp.order_per_candidate else None), GT.step_etas(N, hp.B)


def edit_inputs(edit, hp, confs, p0s, t, dtype):
    """Every candidate's parameters and the shared table passed through edit(conf, hp, p0, t, dtype) -> (p0, t) (the table as
    candidate 0's call returns it); edit None: unchanged."""
    if edit is None:
        return p0s, t
    out = [edit(confs[k], hp, p0s[k], t, dtype) for k in range(len(confs))]
    return [p for p, _ in out], out[0][1]
