"""Deferred stores on the GPU (launches.hip.h, mark_deferred; sweep.hip.h, tile_run's modes): in the two-group launch-per-phase
schedule a feature segment's W / m / v are stored every second step — a virtual pass updates the tile in registers and drops it, the
group's next sweep loads the same version, replays that step and applies its own.  The replay is the same instructions on the same
bits, so everything must equal, BYTE FOR BYTE, the same population trained under MFAS_GROUPS=1 (one group: nothing is ever deferred):
the W, m and v planes of every candidate, the per-epoch statistics with the dev counts, the status words and the best epoch's kept
parameters.  One more test holds the nontemporal headline build, k_step<1,1,4,0,1>, to the float64 reference at step 4 of a four-step
call (both groups have replayed by then), at the taus of tests/test_gpu_step_builds_ref64.py.

Shapes: K = 8 (two groups of 4), two-cell configurations on 64- and 128-column taps, B = 16; R = 128 (eight row blocks: one per
wave) and R = 32 (two row blocks: the k-split units with their cross-wave reduction); N = 2 * 16 + 5 and 3 * 16 + 5 (T = 3: group A pairs
steps (0, 1) and leaves 2 plain, group B has one pair after its plain step 0; T = 4: A has two pairs, B a pair and a plain last step),
the last batch ragged.  That a plan really defers shows in the gather's own line (MFAS_GATHER_VERBOSE: three row sets)."""
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import ref64_cases as G
from tests import step_build_gpu as GB
from tests import train_cases as GT
from tests import step_build_cases as SB
from tests.gpu_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

S_SIZES, V_SIZES = (64, 128, 64, 128), (128, 64, 128, 64)
K, B, CHUNK = 8, 16, 64
# step 4 of a four-step call, and (test_gpu_train_ref64's check wants its last step inside the second epoch) step 7 of a seven-step call:
# six batches per epoch, so that call ends an epoch on a double pass (A) and a plain one (B) and starts the next from the stored planes
STEPS_REF64 = (4, 7)
SWITCHES = ("MFAS_GROUPS", "MFAS_NT", "MFAS_NO_GATHER", "MFAS_GATHER_VERBOSE")


def confs_of(seed):
    rng = np.random.default_rng(seed)
    return [np.stack([rng.integers(0, 4, 2), rng.integers(0, 4, 2), rng.integers(0, 2, 2)], 1) for _ in range(K)]


def run(dev, capfd, R, N, E, env, groups, per_candidate=True, max_steps=-1, segments=None, expect_defer=None):
    """One population trained under `env` and MFAS_GROUPS=groups -> everything that must not depend on the schedule, as bytes."""
    import torch
    from mfas_amd import FeatureTable, Hyper, Population
    assert not any(s in os.environ for s in SWITCHES)
    hp = Hyper(R=R, C=60, B=B, bn=True, drpt=0.5, order_per_candidate=per_candidate, s_sizes=S_SIZES, v_sizes=V_SIZES)
    tr = FeatureTable.from_numpy(O.synth_table(N, 3, snr=0.6, s_sizes=S_SIZES, v_sizes=V_SIZES), dev, torch.bfloat16)
    dv = FeatureTable.from_numpy(O.synth_table(50, 4, snr=0.6, s_sizes=S_SIZES, v_sizes=V_SIZES), dev, torch.bfloat16)
    nb = -(-N // B)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N / B, E * nb)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    perm = lambda: torch.stack([torch.randperm(N, generator=g, device=dev) for _ in range(E)])  # noqa: E731
    order = (torch.stack([perm() for _ in range(K)]) if per_candidate else perm()).to(torch.int32)
    env = dict(env, MFAS_GROUPS=str(groups), MFAS_GATHER_VERBOSE="1")
    os.environ.update(env)
    try:
        capfd.readouterr()
        pop = Population(hp, confs_of(R + N), dev, drop_seeds=list(range(70, 70 + K)), chunk_cols=CHUNK)
        try:
            sched = pop.schedule()
            assert not sched["persistent"] and not sched["wide"] and sched["groups"] == (2 if groups == 2 else sched["groups"])
            pop.init(list(range(1, K + 1)))
            out = []
            if segments is None:
                stats, status = pop.train(tr, dv if max_steps < 0 else None, E, etas, order=order, max_steps=max_steps, snapshot_best=max_steps < 0)
                out += [stats.tobytes(), status.tobytes()]
            else:
                for first, last in segments:
                    stats, status = pop.train(tr, dv, E, etas, order=order, snapshot_best=True, first_epoch=first, last_epoch=last)
                    out += [stats.tobytes(), status.tobytes()]
                    out += [pop.get_params(k, pl).cpu().numpy().tobytes() for k in range(K) for pl in range(3)]
            assert not status.any()
            out += [pop.get_params(k, pl).cpu().numpy().tobytes() for k in range(K) for pl in range(3)]
        finally:
            pop.close()
    finally:
        for key in env:
            os.environ.pop(key, None)
    err = capfd.readouterr().err
    if expect_defer is not None:
        assert ("3 row sets" in err) == expect_defer and ("[gather] on" in err) == expect_defer, err
    return out


# (R, full batches in front of the ragged one, epochs, max_steps, segments)
CASES = {
    "r128-T3": (128, 2, 2, -1, None),
    "r128-T4": (128, 3, 2, -1, None),
    "r32-T3": (32, 2, 2, -1, None),
    "r32-T4": (32, 3, 2, -1, None),
    "r128-2-of-T5": (128, 4, 2, 2, None),
    "r128-resume": (128, 3, 3, -1, [(0, 1), (1, 3)]),
    "r32-resume": (32, 2, 3, -1, [(0, 1), (1, 2), (2, 3)]),
}


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_deferred_stores_bit_identical(dev, capfd, case, nt):
    """Per-candidate sample orders (gathered rows, three sets): two epochs with the dev pass and the best-epoch copy, a call cut by
    max_steps inside its first epoch, and schedules trained in segments (train_from with first = 1)."""
    R, full, E, max_steps, segments = CASES[case]
    N = full * B + 5
    env = {"MFAS_NT": str(nt)}
    got = run(dev, capfd, R, N, E, env, 2, max_steps=max_steps, segments=segments, expect_defer=True)
    want = run(dev, capfd, R, N, E, env, 1, max_steps=max_steps, segments=segments, expect_defer=False)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (case, nt, "item %d of %d (statistics, status, then candidate-major W / m / v)" % (i, len(got)))


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("R,per_candidate", [(128, True), (32, True), (128, False)])
def test_deferred_stores_without_gathered_rows(dev, capfd, R, per_candidate, nt):
    """The same plan staging its rows from the table: MFAS_NO_GATHER=1 through every candidate's own order, and one order shared by
    the population (which never gathers).  T = 4, two epochs with the dev pass."""
    N = 3 * B + 5
    env = {"MFAS_NT": str(nt)}
    if per_candidate:
        run(dev, capfd, R, N, 2, env, 2, expect_defer=True)           # (the plan is the same with and without the gather: it defers)
        env["MFAS_NO_GATHER"] = "1"
    got = run(dev, capfd, R, N, 2, env, 2, per_candidate=per_candidate, expect_defer=False)
    want = run(dev, capfd, R, N, 2, env, 1, per_candidate=per_candidate, expect_defer=False)
    assert got == want


def test_headline_build_deferred_vs_ref64(dev, capfd):
    """k_step<1,1,4,0,1> — the nontemporal headline build — in a deferring plan against ref64: step 4 of a four-step call (group A:
    two pairs; group B: plain, a pair, plain) from the state a three-step call leaves, and step 7 of a seven-step call, taus of tests/test_gpu_step_builds_ref64.py.
    The population is that file's `step-split` row (R = 113, eight row blocks, per-candidate orders) without chain_split, chunk 64."""
    base = next(r for r in SB.SWEEP_FORMS if r["id"] == "step-split")
    row = dict(base, env=dict(base["env"], MFAS_CHAIN_SPLIT="0"), cc=CHUNK, facts=dict(base["facts"], chain_split=0),
               forms={"k_step<1,N,4,0,1>", "k_chain<1,0>"})
    inp = SB.row_inputs(base)
    assert inp["ehp"].order_per_candidate
    os.environ["MFAS_GATHER_VERBOSE"] = "1"
    try:
        capfd.readouterr()
        S, ST, pop, _ = GB.train_states(dev, row, inp, 1, STEPS_REF64)
        pop.close()
    finally:
        del os.environ["MFAS_GATHER_VERBOSE"]
    assert "3 row sets" in capfd.readouterr().err
    GB.check_ref64(row, inp, S, ST, STEPS_REF64, SB.case_taus("step-split"), "NT=1 deferred", "builds/k_step")
