"""Case module: the resident step-loop builds, forms, late-step cases, taus and input builders."""
from tests import ref64_cases as G
from tests import train_cases as GT
from tests import wide_cases as GW


FULL = 5                            # full batches of the train table: nb = 6
STEPS = (1, 2, 3, 5, 6, 7)
LATE = (5, 6, 7)
# parameters, taps and orders of row i are drawn from SEED0 + i: a base on which test_resident_cpu.py's calibration holds for every
# row (TAU_RUNSTAT's margin is narrow, see SEED0 in train_cases.py)
SEED0 = 7000

# tap widths: 9 / 17 / 65 are no multiple of 16; 600, 1000 and 3000 pad to 608 = 16 * 38, 1008 = 16 * 63 and 3008 = 16 * 188, which cut into
# odd chunks (at 256 columns: 19 units of 32, 7 of 144, 47 of 64); 1008 is the WIDE unit at a chunk of 1024
W_R = dict(s=(9, 600, 2048, 1000), v=(17, 65, 1000, 3000))
# populations: mixed depths 1..4, all three nonlinearities
POP_A = [[[0, 1, 0], [2, 0, 1]], [[3, 2, 2]], [[1, 1, 1], [0, 2, 0], [2, 1, 2], [3, 0, 1]]]
POP_B = [[[1, 2, 2], [3, 1, 0], [0, 0, 1]], [[2, 2, 0]]]
POP_W = [[[3, 2, 0], [0, 0, 1]], [[2, 1, 2]], [[1, 3, 1], [3, 0, 0], [0, 2, 2], [2, 2, 1]]]
# more than 256 - K units at 256 columns, at most twice that: two units per workgroup (each 3000-wide tap is 47 units)
POP_N = [[[2, 3, 0], [1, 3, 1]], [[3, 3, 2]], [[0, 3, 1], [2, 2, 0], [3, 3, 2]], [[1, 3, 0]]]
POP_M = [[[1, 3, 2]], [[0, 3, 0], [3, 3, 1], [2, 0, 2], [1, 3, 0]], [[2, 3, 1], [0, 1, 0]], [[3, 3, 0], [1, 2, 2], [1, 3, 1]], [[0, 0, 2]]]

# (id, R, C, B, widths, confs, hyper flags, table dtype, tap_bits, chunk_cols, K)
# flags: bn / drpt0 / alphas / multitask / lm1 (loss_mode 1 with pos_weight); drpt is 0.5 unless drpt0
RESIDENT_BUILDS = [
    ("mb1-plain0-f32-nu1", 16, 60, 16, W_R, POP_A, "alphas,bn", "float32", 0, 0, 3),
    ("mb1-plain0-f32-nu2", 11, 23, 7, W_R, POP_N, "multitask,bn", "float32", 32, 0, 4),
    ("mb1-plain0-x16-nu1", 16, 64, 7, W_R, POP_B, "lm1", "bfloat16", 16, 512, 2),
    ("mb1-plain0-x16-nu2", 8, 5, 16, W_R, POP_M, "alphas", "float16", 0, 0, 5),
    ("mb1-plain0-x16-wide", 16, 17, 16, W_R, POP_W, "multitask,bn,drpt0", "bfloat16", 16, 1024, 3),
    ("mb1-plain1-f32-nu1", 16, 60, 7, W_R, POP_B, "", "float32", 32, 128, 2),
    ("mb1-plain1-f32-nu2", 16, 23, 16, W_R, POP_M, "", "float32", 0, 0, 5),
    ("mb1-plain1-x16-nu1", 11, 64, 16, W_R, POP_A, "", "float16", 16, 0, 3),
    ("mb1-plain1-x16-nu2", 16, 5, 7, W_R, POP_N, "", "bfloat16", 16, 0, 4),
    ("mb1-plain1-x16-wide", 8, 17, 7, W_R, POP_W, "", "float16", 16, 1024, 3),
    ("mb1-plain2-f32-nu1", 8, 60, 16, W_R, POP_A, "bn,drpt0", "float32", 0, 512, 3),
    ("mb1-plain2-f32-nu2", 16, 23, 7, W_R, POP_N, "bn", "float32", 32, 0, 4),
    ("mb1-plain2-x16-nu1", 16, 64, 7, W_R, POP_B, "bn", "bfloat16", 0, 0, 2),
    ("mb1-plain2-x16-nu2", 11, 5, 16, W_R, POP_M, "bn,drpt0", "float16", 16, 0, 5),
    ("mb1-plain2-x16-wide", 16, 17, 16, W_R, POP_W, "bn", "bfloat16", 16, 1024, 3),
    ("mb2-plain0-f32-nu1", 16, 60, 20, W_R, POP_B, "multitask,bn,drpt0", "float32", 32, 0, 2),
    ("mb2-plain0-f32-nu2", 16, 23, 32, W_R, POP_M, "lm1", "float32", 0, 0, 5),
    ("mb2-plain0-x16-nu1", 11, 64, 32, W_R, POP_A, "alphas,bn,drpt0", "float16", 16, 0, 3),
    ("mb2-plain0-x16-nu2", 16, 5, 20, W_R, POP_N, "multitask,bn", "bfloat16", 16, 0, 4),
    ("mb2-plain0-x16-wide", 16, 17, 20, W_R, POP_W, "lm1,bn", "float16", 16, 1024, 3),
    ("mb2-plain1-f32-nu1", 16, 60, 20, W_R, POP_A, "", "float32", 0, 512, 3),
    ("mb2-plain1-f32-nu2", 8, 23, 32, W_R, POP_N, "", "float32", 32, 0, 4),
    ("mb2-plain1-x16-nu1", 16, 64, 32, W_R, POP_B, "", "bfloat16", 0, 128, 2),
    ("mb2-plain1-x16-nu2", 16, 60, 20, W_R, POP_M, "", "float16", 16, 0, 5),
    ("mb2-plain1-x16-wide", 11, 17, 32, W_R, POP_W, "", "bfloat16", 16, 1024, 3),
    ("mb2-plain2-f32-nu1", 11, 60, 32, W_R, POP_B, "bn", "float32", 32, 0, 2),
    ("mb2-plain2-f32-nu2", 16, 23, 20, W_R, POP_M, "bn,drpt0", "float32", 0, 0, 5),
    ("mb2-plain2-x16-nu1", 16, 64, 20, W_R, POP_A, "bn", "float16", 16, 512, 3),
    ("mb2-plain2-x16-nu2", 8, 5, 32, W_R, POP_N, "bn", "bfloat16", 0, 0, 4),
    ("mb2-plain2-x16-wide", 16, 17, 20, W_R, POP_W, "bn,drpt0", "float16", 16, 1024, 3),
]
BUILD_IDS = [r[0] for r in RESIDENT_BUILDS]
FORMS = ("f32-nu1", "f32-nu2", "x16-nu1", "x16-nu2", "x16-wide")
ALL_BUILDS = [f"mb{mb}-plain{plain}-{form}" for mb in (1, 2) for plain in (0, 1, 2) for form in FORMS]
# the rows that also train one epoch with the 83-row dev table (the dev pass reads what the resident launch stored): one per PLAIN
DEV_ROWS = ("mb2-plain0-x16-nu2", "mb2-plain1-x16-nu1", "mb1-plain2-f32-nu2")
# Per-case taus where the float32 oracle itself exceeds a quarter of the project's tau on the case's inputs
# (tests/test_resident_cpu.py): four times the oracle's measured maximum, rounded up.  {id: {quantity: (tau, measured)}}
CASE_TAUS = {}


def case_taus(rid):
    taus = dict(GT.TAUS)
    taus.update({q: float(tau) for q, (tau, _) in CASE_TAUS.get(rid, {}).items()})
    return taus


def base_case(row, cells=None):
    """The 9-tuple test_gpu_ref64's helpers take: (id, R, C, B, widths, cells, bn, drpt, extra)."""
    rid, R, C, B, w, confs, flags = row[:7]
    fl = set(filter(None, flags.split(",")))
    extra = ",".join(sorted(fl & {"alphas", "multitask", "lm1"}))
    return (rid, R, C, B, w, confs[0] if cells is None else cells, "bn" in fl, 0.0 if "drpt0" in fl else 0.5, extra)


def row_order_mode(rid):
    return ("shared", "per_candidate")[BUILD_IDS.index(rid) % 2]


def president_name(rid):
    """The launch record's name of a RESIDENT_BUILDS row: k_president<MB, tiles per wave, 16-bit staging, units per workgroup, PLAIN> —
    four tiles per wave (PERSIST_NTR), eight for the wide unit (PERSIST_NTR16)."""
    mb, plain, form = rid.split("-", 2)
    ntr, x16, nu = {"f32-nu1": (4, 0, 1), "f32-nu2": (4, 0, 2), "x16-nu1": (4, 1, 1), "x16-nu2": (4, 1, 2), "x16-wide": (8, 1, 1)}[form]
    return f"k_president<{mb[2:]},{ntr},{x16},{nu},{plain[5:]}>"


def assert_president_record(pop, rids, tag):
    """The library's record of the population's last train call: one of the builds `rids` name, launched, and nothing else."""
    rec = pop.launch_record()
    assert len(rec) == 1 and set(rec) <= {president_name(r) for r in rids} and all(n > 0 for n in rec.values()), (tag, rec)


def build_inputs(row):
    """What a RESIDENT_BUILDS row trains, as numpy (no device)."""
    from tests.helpers import engine_hyper
    rid, R, C, B, w, cells, flags, dtype, tap_bits, cc, K = row
    seed = SEED0 + BUILD_IDS.index(rid)
    hp = G.case_hyper(base_case(row))
    confs, p0s = [], []
    for k, c in enumerate(cells):
        conf, p0 = G.case_params(base_case(row, c), hp, seed + 10 * k)
        confs.append(conf)
        p0s.append(p0)
    ehp = engine_hyper(hp)
    ehp.tap_bits = tap_bits
    ehp.order_per_candidate = row_order_mode(rid) == "per_candidate"
    N = GT.train_rows(B, FULL)
    t = G.case_table(base_case(row), hp, N, seed, dtype)
    order = GT.make_order(N, seed, K if ehp.order_per_candidate else None)
    return dict(hp=hp, ehp=ehp, confs=confs, seeds=[seed + 3 * k for k in range(K)], p0s=p0s, N=N, t=t, dtype=dtype, order=order,
                etas=GT.step_etas(N, B), seed=seed)


LATE_WIDE = ("wb65", "w177")
LATE_PARAMS = [(name, mode) for name in GT.TRAIN_SCHEDULES for mode in ("shared", "per_candidate")] + \
              [(cid, "per_candidate" if cid in GW.PER_CANDIDATE else "shared") for cid in LATE_WIDE]
