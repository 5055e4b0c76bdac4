"""Case module: the populations, tap cases and scalar sets of the axes tests, with their seeds and input builders."""
import dataclasses
from unittest import mock

from tests import ref64 as R64
from tests import ref64_cases as G
from tests import train_cases as GT


AXES_SEED0 = 9000


# ------------------------------------------------------------------------------------------------ the designs
# unused (width 0) slots between used ones, one width >= 1000 per modality, widths that are no multiple of 16
W_8 = dict(s=(1, 0, 9, 15, 17, 63, 65, 1000), v=(8, 2048, 0, 0, 33, 0, 4100, 129))
W_AV = dict(s=(3, 6, 12, 24, 48), v=(3, 6, 12))                 # AV-MNIST (avmnist_searchable.py)
W_26 = dict(s=(17, 65), v=(9, 0, 64, 129, 1000, 15))            # 2 + 6, MM-IMDB-like; v1 unused
WIDTHS = {"w8": W_8, "wav": W_AV, "w26": W_26}

# (id, R, C, B, widths, cells, bn, drpt, extra): the 9-tuple of test_gpu_ref64's helpers
TAP_CASES = [
    ("t8a", 16, 60, 20, W_8, [[7, 7, 0], [0, 0, 1]], True, 0.5, ""),                        # the lean chain; slot 7 of both in cell 0
    ("t8b", 33, 17, 33, W_8, [[2, 1, 2], [7, 6, 0], [4, 4, 1]], False, 0.5, "multitask"),
    ("t8c", 128, 60, 16, W_8, [[5, 4, 0], [6, 7, 1]], True, 0.0, ""),
    ("t8d", 65, 2, 17, W_8, [[3, 6, 1], [3, 0, 0], [5, 1, 2], [6, 6, 0]], False, 0.9, "alphas"),   # s3 and v6 in two cells
    ("t8w", 16, 17, 65, W_8, [[6, 7, 2], [7, 4, 0]], True, 0.5, ""),                        # B = 65: the wide path
    ("tav_a", 16, 10, 16, W_AV, [[4, 2, 0], [1, 1, 1]], True, 0.5, ""),
    ("tav_b", 32, 10, 20, W_AV, [[3, 0, 2], [4, 2, 0], [2, 1, 1]], False, 0.5, "alphas"),
    ("t26a", 17, 23, 16, W_26, [[1, 5, 0], [0, 3, 1]], False, 0.5, "lm1"),
    ("t26b", 80, 60, 3, W_26, [[0, 2, 1], [1, 5, 0], [1, 4, 2]], False, 0.5, ""),
    ("t26c", 256, 5, 20, W_26, [[1, 3, 0], [0, 5, 1]], True, 0.5, ""),
]
TAP_IDS = [c[0] for c in TAP_CASES]


def case_seed(cid):
    return AXES_SEED0 + TAP_IDS.index(cid)


# Candidates of a population per width set: K >= 3 takes them in turn.  In "w8" candidates 0 and 2 share tap s7, candidate 1 selects
# only slots 0..3 and candidate 2 only slots 4..7, with s7 and v7 in its first two cells (BatchNorm populations cut it to those).
TAP_CONFS = {
    "w8": ([[7, 7, 0], [2, 4, 1]], [[0, 0, 2]], [[7, 6, 0], [5, 7, 1], [4, 4, 0]], [[3, 1, 1]]),
    "wav": ([[4, 2, 0], [1, 1, 1]], [[0, 0, 2]], [[2, 1, 0], [3, 0, 1], [4, 2, 0]], [[1, 2, 1]]),
    "w26": ([[1, 5, 0], [0, 3, 1]], [[0, 0, 2]], [[1, 4, 0], [0, 5, 1], [1, 2, 0]], [[0, 2, 1]]),
}
# BatchNorm populations keep to two cells (a deeper BatchNorm stack leaves most rows of a train batch ambiguous in ref64 itself,
# DESIGN.md section 8): candidate 2 loses its third cell there.  The tap populations of TAP_NO_BN train without BatchNorm and keep it.
# For same_group and chain_split that is a necessity: at R = 128, C = 60 over the 8-slot widths two BatchNorm cells already leave
# 3 .. 8 of the ragged batch's 8 rows ambiguous, on each of the ten table seeds 161 .. 170 tried.  For general_mb1, general_mb4 and
# tap_major it is a choice — a three-cell candidate over a tap axis was preferred to BatchNorm there — so slots >= 4 run under
# BatchNorm on four of the nine schedules (lean_chain, general_mb2, persistent, two_group_ab) and on the wide population; the scalar
# sets keep BatchNorm on every schedule.
TAP_NO_BN = ("general_mb1", "general_mb4", "same_group", "chain_split", "tap_major")
SCALAR_CONFS = tuple(c[:2] for c in GT.SCHED_CONFS)


def no_bn_hyper(hp):
    return dataclasses.replace(hp, bn=False)


# plain cells: depths 2, 4, 1 within the first three candidates, 3 from the fourth on; all three nonlinearities
PLAIN_CONFS = ([[3, 3, 0], [1, 2, 1]], [[1, 0, 1], [0, 2, 2], [2, 3, 0], [3, 1, 2]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1], [1, 1, 0]])

# a TRAIN_SCHEDULES-like entry for the wide path (B > 64): (R, C, B, env, chunk_cols, K, tap_bits, check)
EXTRA_ENTRIES = {"wide_b65": (16, 60, 65, {}, 0, 3, 0, lambda s: s["wide"] == 1 and s["persistent"] == 0)}
TAP_WIDTHS_OF = {"lean_chain": "w8", "general_mb1": "w26", "general_mb2": "wav", "general_mb4": "w8", "same_group": "w8",
                 "chain_split": "w8", "persistent": "w8", "two_group_ab": "w8", "tap_major": "w8", "wide_b65": "w8"}


SCALAR_SETS = {
    # the edges: no weight decay, no first moment, running statistics = the batch's, a large adam_eps, eta_max >= 1e-2
    "sa": dict(wd=0.0, beta1=0.0, beta2=0.99, adam_eps=1e-3, bn_eps=1e-3, bn_momentum=1.0, f1_threshold=0.5, eta_max=1e-2, eta_min=1e-4),
    "sb": dict(wd=1e-2, beta1=0.5, beta2=0.9, adam_eps=1e-6, bn_eps=1e-2, bn_momentum=0.5, f1_threshold=0.7, eta_max=5e-3, eta_min=1e-5),
    # every learning rate exactly 0: w comes back bit-identical while m and v move
    "sc": dict(wd=1e-3, beta1=0.8, beta2=0.95, adam_eps=1e-5, bn_eps=1e-4, bn_momentum=0.01, f1_threshold=0.6, eta_max=0.0, eta_min=0.0),
    # a learning rate of 3e-2: three steps move the fusion biases so far that the float32 batch sums round by more than M_mu and
    # M_var count; its population steps are judged with ref64's batch_sum_term (BATCH_SUM_SETS), nothing else is
    "sd": dict(wd=5e-3, beta1=0.7, beta2=0.98, adam_eps=1e-4, bn_eps=5e-3, bn_momentum=0.3, f1_threshold=0.4, eta_max=3e-2, eta_min=3e-5),
}
BATCH_SUM_SETS = ("sd",)
# the multi-label head under BatchNorm at two dev-pass geometries with MFAS_EVAL_NO_* builds (R <= 32 and 65 <= R <= 128)
SCALAR_EVAL_CASES = [
    ("se16", 16, 23, 16, G.W_A, [[0, 3, 0], [1, 1, 2]], True, 0.5, "lm1"),
    ("se80", 80, 60, 16, G.W_A, [[3, 1, 1], [2, 2, 0]], True, 0.5, "lm1"),
]


def plain_hyper(hp):
    return dataclasses.replace(hp, allow_plain_cell=True, bn=False, drpt=0.0)


def scalar_hyper(sid):
    return lambda hp: dataclasses.replace(hp, **SCALAR_SETS[sid])


def spec_flag(spec):
    """ref64's batch_sum_term for the train steps of a population of POPS: on for the scalar sets of BATCH_SUM_SETS alone."""
    return spec[3] == "scalar" and spec[4] in BATCH_SUM_SETS


def scalar_case_hyper(case, sid):
    return dataclasses.replace(G.case_hyper(case), **SCALAR_SETS[sid])


# Populations: (id, schedule name, order mode, axis, key) — key: the width set (tap), None (plain) or the scalar set
ALL_NAMES = list(GT.TRAIN_SCHEDULES) + ["wide_b65"]
TAP_POPS = [(f"tap-{n}-{m}", n, m, "tap", TAP_WIDTHS_OF[n]) for n in GT.TRAIN_SCHEDULES for m in ("shared", "per_candidate")] + \
           [("tap-wide_b65-shared", "wide_b65", "shared", "tap", "w8")]
PLAIN_POPS = [(f"plain-{n}", n, "per_candidate" if n in ("two_group_ab", "persistent", "general_mb2") else "shared", "plain", None)
              for n in ALL_NAMES if n != "tap_major"]
SCALAR_POPS = [(f"{sid}-{n}-{m}", n, m, "scalar", sid) for sid in SCALAR_SETS
               for n, m in [(n, "shared") for n in ALL_NAMES] + [("two_group_ab", "per_candidate"), ("persistent", "per_candidate")]]
POPS = TAP_POPS + PLAIN_POPS + SCALAR_POPS
POP_IDS = [p[0] for p in POPS]


def pop_entry(name):
    return EXTRA_ENTRIES.get(name) or GT.TRAIN_SCHEDULES[name]


def pop_inputs(spec, full=1):
    """What a population of POPS trains, as numpy: test_gpu_train_ref64.schedule_inputs with the axis' arguments."""
    pid, name, mode, axis, key = spec
    kw = dict(entry=pop_entry(name))
    if axis == "tap":
        deep = name in TAP_NO_BN
        kw.update(widths=WIDTHS[key], sched_confs=TAP_CONFS[key] if deep else tuple(c[:2] for c in TAP_CONFS[key]),
                  hyper=no_bn_hyper if deep else None)
    elif axis == "plain":
        kw.update(hyper=plain_hyper, sched_confs=PLAIN_CONFS)
    else:
        kw.update(hyper=scalar_hyper(key), sched_confs=SCALAR_CONFS)
    return GT.schedule_inputs(name, mode, full, **kw)


POP_DL_SEED = 100       # candidate k's arbitrary dL/dlogits of the entry-point block is drawn from POP_DL_SEED + k


def pop_eval_table(inp):
    """The 83-row table a population's entry points and dev pass read (seed 62, like the sibling files' dev tables)."""
    hp = inp["hp"]
    return G.case_table(("pop", hp.R, hp.C, hp.B, None, None, hp.bn, hp.drpt, ""), hp, G.N_EVAL, 62, inp["dtype"])


# ------------------------------------------------------------------------------------------------ calibration
class count_spy:
    """Records ref64.train_step64's count interval of every step it is asked for: the ambiguity condition needs ref64 alone."""

    def __enter__(self):
        self.seen = []
        real = R64.train_step64

        def spy(state, conf, hp, batch, *a, **kw):
            exp = real(state, conf, hp, batch, *a, **kw)
            self.seen.append((exp["count"], len(batch["label"]), hp))
            return exp
        self.patch = mock.patch.object(R64, "train_step64", spy)
        self.patch.__enter__()
        return self

    def __exit__(self, *a):
        self.patch.__exit__(*a)

    def check(self, tag):
        for (lo, hi), n, hp in self.seen:
            if hp.loss_mode == 0:
                assert 4 * (hi - lo) <= n, (tag, "ambiguous rows in a train step", lo, hi, n)
