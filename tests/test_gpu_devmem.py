"""A population's device memory across calls (mfas_amd/csrc/devmem.hip.h: every buffer a DevBuf, the grow-only ones through reserve).

(a) One population grows every grow-only buffer — statistics and step scalars (train with 1, then 3 epochs), the evaluate arena
    (M = 1, then M = 4 with a report and no caller's scores), the move scratch of a second population (a one-cell, then a two-cell
    candidate) — and must then hold, byte for byte, what fresh populations hold that made only the second call of each pair.
(b) In a process of its own on the test-hooks variant, which counts DevBuf's live allocations: a resident population whose second
    epoch falls back to launch-per-phase (the not-resident hook launches nothing), with a kept-best plane, then evaluate and a move,
    holds after the fallback exactly as many allocations as a population created launch-per-phase that made the same calls — and
    after both are destroyed the process holds none.

The smallest shapes that still reach every buffer: R = 16, C = 5, B = 8, N = 24 (three batches), K = 2 (one and two cells), f32
tables holding the two narrowest taps of each modality.  Everything is exact; nothing here provokes a fault."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mfas_amd as M
from tests import devmem_gpu as DG
from tests.gpu_dev import dev  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, CONFS = DG.K, DG.CONFS


def planes(pop, ks=range(K)):
    return [[pop.get_params(k, pl).cpu().numpy() for pl in range(3)] for k in ks]


def same_planes(a, b):
    return all(np.array_equal(x, y) for ka, kb in zip(a, b) for x, y in zip(ka, kb))


def same_bytes(a, b):
    """arrays (or scalars) with the same bytes; dicts of them, key by key"""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same_bytes(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_buffers_that_grew_hold_what_fresh_ones_hold(dev):
    hp, tr, dv, etas = DG.workload(dev)

    def fresh():
        return M.Population(hp, CONFS, dev, drop_seeds=[5, 6])

    seedpop = fresh()
    seedpop.init([1, 2])
    start = [seedpop.get_params(k, 0) for k in range(K)]        # every run starts from these parameters
    seedpop.close()

    def trained(epochs_list):
        pop = fresh()
        for epochs in epochs_list:
            for k in range(K):
                pop.set_params(k, start[k])
            stats, status = pop.train(tr, dv, epochs, etas)
            assert not status.any()
        return pop, stats

    grown, stats = trained([1, 3])           # statistics and (a resident population's) step scalars grow
    ref, ref_stats = trained([3])
    assert grown.schedule() == ref.schedule() and grown.schedule()["persistent"]      # (resident: the step scalars live on the device)
    assert stats.tobytes() == ref_stats.tobytes() and (stats["train_loss_sum"] != 0).all()
    assert same_planes(planes(grown), planes(ref))

    grown.evaluate(dv, members=[0])          # the arena grows: M = 1, then four members, the report and its own score rows
    got, want = (p.evaluate(dv, members=[0, 1, 0, 1], report=True) for p in (grown, ref))
    assert got["member_stats"].tobytes() == want["member_stats"].tobytes() and got["ensemble"] == want["ensemble"]
    assert same_bytes(got["report"], want["report"])      # the tallies and everything report_metrics derives from them
    assert got["report"]["confusion"].any() and got["report"]["rank_hist"].any()

    dst, dst_ref = fresh(), fresh()          # the move scratch grows: the one-cell candidate, then the two-cell one
    dst.move_from(grown, 0, 0)
    dst.move_from(grown, 1, 1)
    dst_ref.move_from(ref, 1, 1)
    assert same_planes(planes(dst, [1]), planes(dst_ref, [1])) and same_planes(planes(dst), planes(ref))
    assert dst.get_progress(1) == dst_ref.get_progress(1)
    for p in (grown, ref, dst, dst_ref):
        p.close()


def test_no_allocation_outlives_its_population():
    import __graft_entry__ as ge
    lib = ge.build_variant("hooks", ["-DMFAS_TEST_HOOKS"])
    prog = "import sys; sys.path.insert(0, sys.argv[1]); from tests import devmem_gpu as DG; DG.live_allocations_program(sys.argv[1])"
    res = subprocess.run([sys.executable, "-c", prog, ROOT], env=dict(os.environ, MFAS_LIB=lib), capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert res.returncode == 0 and "LIVE_OK" in res.stdout and " end=0" in res.stdout, (res.stdout[-2000:], res.stderr[-3000:])
