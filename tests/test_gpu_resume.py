"""Resume: a schedule run in segments (mfas_population_train_from), through export / import, a checkpoint file, a move into a
population of another size, and successive halving on top of it — every check is EXACT (bit patterns), no tolerance anywhere.

Why exact is the right bar (include/mfas_hip.h, "Resume"): step t of epoch e is e * nb + t for the Adam step scalars, the dropout
stream, the sample order and the statistics slot alike, every epoch starts with a forward-only prologue, and a candidate's state
between two epochs is exactly planes 0 / 1 / 2 (+ the kept best and the host bookkeeping of train_searchable/ntu.py:17-18,82-86).

Shapes: N_train = 3 B + 5 (4 batches per epoch, the last of 5 rows), N_dev = 64, E = 3, BatchNorm + dropout 0.5, taps 16..100 columns
wide (100 and 24 are no multiples of 16), configurations of 1..4 cells with all three non-linearities.  One case per train schedule,
each asserted through Population.schedule()."""
import os

import numpy as np
import pytest
import torch

import mfas_amd as M
from mfas_amd import ntu_searchable as NS
from mfas_amd.engine import load_checkpoint, save_checkpoint
from oracle import np_oracle as O
from tests.gpu_dev import dev  # noqa: F401

pytestmark = pytest.mark.gpu

S_W, V_W = (16, 48, 100, 32), (64, 96, 24, 80)
C, E, N_DEV = 10, 3, 64
CONFS = [np.array(c) for c in ([[3, 1, 1], [1, 3, 0], [1, 1, 2], [3, 3, 0]], [[0, 2, 2]], [[2, 0, 0], [0, 1, 1]],
                               [[1, 2, 2], [2, 3, 1], [0, 0, 0]], [[2, 2, 1]], [[3, 0, 2], [2, 1, 0]],
                               [[0, 3, 0], [1, 0, 2], [3, 2, 1], [2, 2, 2]], [[1, 1, 0]], [[3, 3, 2], [0, 0, 1]],
                               [[2, 1, 1], [1, 2, 0], [0, 3, 2]], [[0, 1, 0]], [[1, 3, 1], [3, 1, 2]])]

CASES = {
    # name: (R, B, K, env, chunk_cols, per-candidate orders, loss_mode, schedule check)
    "resident": (16, 20, 6, {}, 0, True, 0, lambda s: s["persistent"] == 1),
    "resident_shared_order": (16, 20, 6, {}, 0, False, 0, lambda s: s["persistent"] == 1),
    "same_group": (32, 16, 3, {}, 0, True, 0, lambda s: s["persistent"] == 0 and s["groups"] == -1 and s["chain_cus"] == 1),
    "same_group_multilabel": (32, 16, 3, {}, 0, True, 1, lambda s: s["persistent"] == 0 and s["groups"] == -1),
    "two_group": (32, 16, 12, {"MFAS_GROUPS": "2"}, 0, True, 0, lambda s: s["persistent"] == 0 and s["groups"] == 2),
    "chain_split": (128, 16, 2, {}, 0, True, 0, lambda s: s["groups"] == -1 and s["chain_cus"] == 4),
    "wide": (80, 33, 2, {}, 0, True, 0, lambda s: s["wide"] == 1 and s["persistent"] == 0),
}


def make_table(n, seed, dev, loss_mode):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    label = torch.randint(0, C, (n,), generator=g, device=dev)
    taps = {}
    for name, sizes in (("s", S_W), ("v", V_W)):
        for j, w in enumerate(sizes):
            mu = torch.randn(C, w, generator=torch.Generator(device=dev).manual_seed(1000 + 10 * (name == "v") + j), device=dev)
            taps[f"{name}{j}"] = torch.relu(0.5 * mu[label] + torch.randn(n, w, generator=g, device=dev)).to(torch.bfloat16)
    ml = None
    if loss_mode == 1:
        ml = torch.nn.functional.one_hot(label, C).float()
        ml = torch.clamp(ml + (torch.rand(n, C, generator=g, device=dev) < 0.15).float(), max=1.0)
    return M.FeatureTable(taps, label.to(torch.int32), multilabel=ml)


class Case:
    """One schedule's workload: tables, eta table and sample orders of the whole E-epoch schedule, and identically initialised handles."""

    def __init__(self, name, dev):
        self.name, self.dev = name, dev
        self.R, self.B, self.K, self.env, self.cc, self.per_cand, self.loss_mode, self.check = CASES[name]
        self.hp = M.Hyper(R=self.R, C=C, B=self.B, bn=True, drpt=0.5, s_sizes=S_W, v_sizes=V_W, tap_bits=16, loss_mode=self.loss_mode,
                          order_per_candidate=self.per_cand)
        self.confs = CONFS[:self.K]
        self.n = 3 * self.B + 5
        self.nb = 4
        self.etas = O.eta_sequence(1e-3, 1e-6, 1, 2, self.n / self.B, E * self.nb)
        self.order = (NS.make_order_per_candidate(self.n, E, True, 77, dev, range(self.K)) if self.per_cand
                      else NS.make_order(self.n, E, True, 77, dev))
        self.seeds = list(range(300, 300 + self.K))
        # The snapshot_best runs need a candidate whose epoch 0 stays its best epoch (a snapshot taken two calls before the end has to
        # survive them).  Whether a data set has one is a property of the data, not of the code under test: take the first of a few
        # table seeds whose uninterrupted, plain train() run shows it.
        for data_seed in range(21, 101, 10):
            self.tr, self.dv = make_table(self.n, data_seed, dev, self.loss_mode), make_table(N_DEV, data_seed + 1, dev, self.loss_mode)
            self._ref = {}
            m = self.metric(self.reference(False)[0])
            if (m[:, 0:1] >= m).all(axis=1).any():
                break

    def fresh(self, init=True):
        os.environ.update(self.env)
        try:
            pop = M.Population(self.hp, self.confs, self.dev, drop_seeds=self.seeds, chunk_cols=self.cc)
        finally:
            for k in self.env:
                os.environ.pop(k, None)
        sched = pop.schedule()
        assert self.check(sched), (self.name, sched)
        if init:
            pop.init([11 + k for k in range(self.K)])
        return pop

    def train(self, pop, snapshot, first=0, last=None):
        return pop.train(self.tr, self.dv, E, self.etas, order=self.order, snapshot_best=snapshot, first_epoch=first, last_epoch=last)

    def reference(self, snapshot, threshold=None):
        """The uninterrupted one-call run (mfas_population_train), computed once per (snapshot, threshold) and never modified."""
        key = (snapshot, threshold)
        if key not in self._ref:
            pop = self.fresh()
            if threshold is not None:
                pop.set_best_threshold(threshold)
            stats, status = pop.train(self.tr, self.dv, E, self.etas, order=self.order, snapshot_best=snapshot)
            self._ref[key] = (stats.copy(), status.copy(), state_of(pop))
            pop.close()
        return self._ref[key]

    def metric(self, stats):
        scale = 1.0 / 4294967296.0 if self.loss_mode == 1 else 1.0
        return stats["dev_corrects"].astype(np.float64) * scale / float(N_DEV)

    def threshold(self):
        """snapshot_best's starting threshold for this case: just below the smallest epoch-0 dev metric, so that epoch 0 replaces the
        initial parameters for every candidate; the case must then hold a candidate whose epoch 0 stays the best (strict '>')."""
        m = self.metric(self.reference(False)[0])
        assert (m[:, 0:1] >= m).all(axis=1).any(), f"{self.name}: no table seed gave a candidate that keeps epoch 0 as its best epoch: {m}"
        return float(m[:, 0].min()) - 1.0 / 1024.0


_CASES = {}


def case_of(name, dev):
    if name not in _CASES:
        _CASES[name] = Case(name, dev)
    return _CASES[name]


def state_of(pop):
    """Planes 0 (parameters + BatchNorm running statistics), 1 and 2 of every candidate, as bytes."""
    return [[pop.get_params(k, pl).cpu().numpy().tobytes() for pl in range(3)] for k in range(pop.K)]


def assert_same(got, want, what):
    stats, status, state = got
    rstats, rstatus, rstate = want
    for col in stats.dtype.names:
        assert stats[col].tobytes() == rstats[col].tobytes(), (what, col, stats[col], rstats[col])
    assert status.tobytes() == rstatus.tobytes(), (what, status, rstatus)
    for k, (a, b) in enumerate(zip(state, rstate)):
        for pl in range(3):
            assert a[pl] == b[pl], (what, "candidate", k, "plane", pl)


def run_segments(case, pop, snapshot, first=0):
    """Epochs [first, E) one call each; returns the assembled statistics (every call's columns outside its segment must be zero)."""
    total, status = None, None
    for ep in range(first, E):
        stats, status = case.train(pop, snapshot, ep, ep + 1)
        outside = np.delete(stats, ep, axis=1)
        assert outside.tobytes() == np.zeros_like(outside).tobytes(), (case.name, ep, "statistics outside the segment")
        assert [pop.get_progress(k)["epochs_done"] for k in range(pop.K)] == [ep + 1] * pop.K
        if total is None:
            total = np.zeros_like(stats)
        total[:, ep] = stats[:, ep]
    return total, status


# ------------------------------------------------------------------------------------------------ 1. segments equal one call
@pytest.mark.parametrize("snapshot", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_segments_equal_one_call(dev, name, snapshot):
    """train(E = 3) against train_from over [0, 1), [1, 2), [2, 3) on an identically initialised handle: planes 0 / 1 / 2, the
    BatchNorm statistics (plane 0), every statistics column and status, bit for bit; and train(E) against train_from(0, E).  With
    snapshot_best the starting threshold makes epoch 0 — a snapshot taken two calls before the end — the kept best of a candidate."""
    case = case_of(name, dev)
    thr = case.threshold() if snapshot else None
    want = case.reference(snapshot, thr)
    if snapshot:
        first_best = (case.metric(want[0])[:, 0:1] >= case.metric(want[0])).all(axis=1)
        assert first_best.any()
    pop = case.fresh()
    if snapshot:
        pop.set_best_threshold(thr)
    stats, status = run_segments(case, pop, snapshot)
    assert_same((stats, status, state_of(pop)), want, f"{name}: three segments")
    pop.close()
    pop = case.fresh()
    if snapshot:
        pop.set_best_threshold(thr)
    stats, status = case.train(pop, snapshot, 0, E)
    assert_same((stats, status, state_of(pop)), want, f"{name}: train_from(0, E)")
    pop.close()


# ------------------------------------------------------------------------------------------------ 2. export / import, checkpoint file
@pytest.mark.parametrize("via", ["export", "file"])
@pytest.mark.parametrize("name", list(CASES))
def test_export_import_continues_bit_identically(dev, name, via, tmp_path):
    """After epoch 0 (first_epoch = 1 from then on): export every candidate, destroy the population, import into a fresh one with the
    same configurations and seeds, run epochs [1, 3): the uninterrupted run's bits.  The same through a checkpoint file."""
    case = case_of(name, dev)
    snapshot = True
    thr = case.threshold()
    want = case.reference(snapshot, thr)
    pop = case.fresh()
    pop.set_best_threshold(thr)
    stats0, _ = case.train(pop, snapshot, 0, 1)
    if via == "export":
        states = [pop.export_candidate(k) for k in range(pop.K)]
        assert all(st["epochs_done"] == 1 and st["nb"] == case.nb and st["best"] is not None for st in states)
    else:
        save_checkpoint(str(tmp_path / "pop.ckpt"), pop)
    pop.close()
    pop = case.fresh(init=False)
    pop.set_best_threshold(thr)
    if via == "export":
        for k, st in enumerate(states):
            pop.import_candidate(k, st)
    else:
        load_checkpoint(str(tmp_path / "pop.ckpt"), pop)
    stats, status = run_segments(case, pop, snapshot, first=1)
    stats[:, 0] = stats0[:, 0]
    assert_same((stats, status, state_of(pop)), want, f"{name}: {via}")
    pop.close()


def test_checkpoint_refuses_a_mismatch(dev, tmp_path):
    case = case_of("same_group", dev)
    pop = case.fresh()
    case.train(pop, False, 0, 1)
    path = str(tmp_path / "pop.ckpt")
    save_checkpoint(path, pop)
    pop.close()
    other = M.Population(case.hp, case.confs[:2] + [CONFS[3]], dev, drop_seeds=case.seeds)
    with pytest.raises(ValueError, match="configurations"):
        load_checkpoint(path, other)
    other.close()
    hp2 = M.Hyper(**{**case.hp.__dict__, "drpt": 0.25})
    other = M.Population(hp2, case.confs, dev, drop_seeds=case.seeds)
    with pytest.raises(ValueError, match="drpt"):
        load_checkpoint(path, other)
    other.close()


# ------------------------------------------------------------------------------------------------ 3. move across population sizes
def test_move_into_a_smaller_population(dev):
    """R = 32, chunk_cols = 64: a K = 6 population trains epoch 0, candidates 1 and 4 move into a K = 2 population (created with their
    seeds), which runs epochs [1, 3) — the bits of a K = 2 population of those two candidates trained uninterrupted with the same
    seeds, orders and chunk_cols.  The control comes first: at this geometry and chunk_cols the one-call train() gives candidates 1
    and 4 the same bits in the K = 6 and in the K = 2 population (the unit decomposition, hence the summation order, is per
    candidate)."""
    R, B, n, nb, picks = 32, 16, 53, 4, [1, 4]
    hp = M.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5, s_sizes=S_W, v_sizes=V_W, tap_bits=16, order_per_candidate=True)
    tr, dv = make_table(n, 31, dev, 0), make_table(N_DEV, 32, dev, 0)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, n / B, E * nb)
    order6 = NS.make_order_per_candidate(n, E, True, 78, dev, range(6))
    order2 = order6[picks].contiguous()
    seeds6, init6 = list(range(500, 506)), list(range(40, 46))

    def population(idx):
        pop = M.Population(hp, [CONFS[i] for i in idx], dev, drop_seeds=[seeds6[i] for i in idx], chunk_cols=64)
        pop.init([init6[i] for i in idx])
        return pop

    big, small = population(range(6)), population(picks)
    assert big.schedule()["persistent"] == 0 and small.schedule()["persistent"] == 0
    sb, _ = big.train(tr, dv, E, etas, order=order6, snapshot_best=True)
    ss, status_s = small.train(tr, dv, E, etas, order=order2, snapshot_best=True)
    want_state = state_of(small)
    for j, i in enumerate(picks):       # the control, on the one-call train()
        assert sb[i].tobytes() == ss[j].tobytes(), ("control: statistics", i)
        assert state_of(big)[i] == want_state[j], ("control: state", i)
    big.close()
    small.close()

    big = population(range(6))
    s0, _ = big.train(tr, dv, E, etas, order=order6, snapshot_best=True, first_epoch=0, last_epoch=1)
    small = M.Population(hp, [CONFS[i] for i in picks], dev, drop_seeds=[seeds6[i] for i in picks], chunk_cols=64)
    for j, i in enumerate(picks):
        small.move_from(big, i, j)
    big.close()                          # (the move is ordered before the source's destruction: destroy synchronises its stream)
    assert [small.get_progress(j)["epochs_done"] for j in range(2)] == [1, 1]
    s12, status = small.train(tr, dv, E, etas, order=order2, snapshot_best=True, first_epoch=1, last_epoch=E)
    s12[:, 0] = s0[picks, 0]
    assert_same((s12, status, state_of(small)), (ss, status_s, want_state), "moved candidates")
    small.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_population_unchanged(dev):
    case = case_of("same_group", dev)
    pop = case.fresh()

    def refused(call, match):
        before = state_of(pop), [pop.get_progress(k) for k in range(pop.K)]
        with pytest.raises(RuntimeError, match=match) as ei:
            call()
        assert "mfas_hip error -1" in str(ei.value)      # MFAS_EINVAL
        assert (state_of(pop), [pop.get_progress(k) for k in range(pop.K)]) == before

    refused(lambda: case.train(pop, False, 2, 3), r"first_epoch = 2 .* 0 epoch\(s\) complete")              # a fresh population
    case.train(pop, False, 0, 1)
    refused(lambda: case.train(pop, False, 2, 3), r"first_epoch = 2 .* 1 epoch\(s\) complete")              # not what the record says
    short = make_table(2 * case.B + 5, 21, dev, 0)                                                            # 3 batches per epoch, not 4
    refused(lambda: pop.train(short, case.dv, E, case.etas, order=case.order, first_epoch=1, last_epoch=2), r"3 batches per epoch.* 4 batches per epoch")
    refused(lambda: case.train(pop, True, 1, 2), "snapshot_best = 1 .* started with snapshot_best = 0")     # flipped mid-schedule
    flat = pop.get_params(0, 0)
    refused(lambda: pop.set_state(0, 0, flat), "plane 0")
    refused(lambda: pop.set_state(0, 4, flat), "plane 4")
    other = M.Population(case.hp, [case.confs[1], case.confs[0]], dev)
    refused(lambda: pop.move_from(other, 0, 0), "different configurations")
    other.close()
    # ... and the schedule still goes on where it stood: the uninterrupted run's bits
    stats, status = run_segments(case, pop, False, first=1)
    want = case.reference(False)
    stats[:, 0] = want[0][:, 0]
    assert_same((stats, status, state_of(pop)), want, "after the refusals")
    pop.close()


def test_train_after_a_partial_schedule_starts_fresh(dev):
    """mfas_population_train owes nothing to an unfinished schedule: after train_from(0, 1) it gives what a population that was
    handed the same parameters through set_params (a fresh Adam) gives, and it resets the record."""
    case = case_of("same_group", dev)
    a = case.fresh()
    case.train(a, False, 0, 1)
    w = [a.get_params(k, 0) for k in range(a.K)]
    got = a.train(case.tr, case.dv, E, case.etas, order=case.order) + (state_of(a),)
    assert [a.get_progress(k)["epochs_done"] for k in range(a.K)] == [0] * a.K
    with pytest.raises(RuntimeError, match="first_epoch = 1"):
        case.train(a, False, 1, 2)
    a.close()
    b = case.fresh(init=False)
    for k in range(b.K):
        b.set_params(k, w[k])
    want = b.train(case.tr, case.dv, E, case.etas, order=case.order) + (state_of(b),)
    b.close()
    assert_same(got, want, "train() after a partial schedule")


# ------------------------------------------------------------------------------------------------ 5. halving end to end
def test_halving_end_to_end(dev):
    """train_sampled_models with engine_halving = (2, (1, 2)) on K = 8, R = 16, E = 3 against the same call without it (torch seeded
    alike, engine_chunk_cols fixed): 8 metrics; the 2 finalists' equal the full run's; an eliminated candidate's equals the full run's
    best over the epochs it ran, from that run's statistics (captured through Population.train)."""
    from types import SimpleNamespace
    args = SimpleNamespace(vid_len=(8, 32), num_outputs=C, drpt=0.5, inner_representation_size=16, batchnorm=True, alphas=False,
                           multitask=False, weightsharing=False, batchsize=20, eta_max=1e-3, eta_min=1e-6, Ti=1, Tm=2,
                           use_dataparallel=False, verbose=False, epochs=E, s_sizes=S_W, v_sizes=V_W, engine_chunk_cols=64)
    confs = CONFS[:8]
    tr, dv = make_table(65, 41, dev, 0), make_table(N_DEV, 42, dev, 0)
    loaders = {"train": M.FeatureLoader(tr, 20, shuffle=True), "dev": M.FeatureLoader(dv, 20, shuffle=False)}
    seen = []
    real_train = M.Population.train

    def spy(self, *a, **kw):
        out = real_train(self, *a, **kw)
        seen.append((self.K, kw.get("first_epoch", 0), kw.get("last_epoch"), out[0].copy()))
        return out

    M.Population.train = spy
    try:
        torch.manual_seed(9)
        full = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, loaders, args, dev)
        full_stats = seen[-1][3]
        assert len(seen) == 1 and seen[0][0] == 8
        del seen[:]
        args.engine_halving = (2, (1, 2))
        torch.manual_seed(9)
        halved = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, loaders, args, dev)
    finally:
        M.Population.train = real_train
    assert [(k, f, l) for k, f, l, _ in seen] == [(8, 0, 1), (4, 1, 2), (2, 2, 3)], [(k, f, l) for k, f, l, _ in seen]
    assert len(halved) == 8 and len(full) == 8
    acc = full_stats["dev_corrects"].astype(np.float64) / float(N_DEV)
    best_upto = lambda i, n: float(max(0.0, acc[i, :n].max()))
    rung1 = M.population.halving_survivors([best_upto(i, 1) for i in range(8)], [0] * 8, 2)
    rung2 = [rung1[p] for p in M.population.halving_survivors([best_upto(i, 2) for i in rung1], [0] * 4, 2)]
    assert len(rung1) == 4 and len(rung2) == 2
    for i in range(8):
        ran = 3 if i in rung2 else 2 if i in rung1 else 1
        assert halved[i] == best_upto(i, ran), (i, ran, halved[i], best_upto(i, ran), acc[i])
        if ran == 3:
            assert halved[i] == full[i], (i, halved[i], full[i])
