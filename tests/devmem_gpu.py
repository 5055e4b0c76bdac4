"""Device plumbing of tests/test_gpu_devmem.py: the smallest workload that still reaches every device buffer of a population —
R = 16, C = 5, B = 8, N = 24 (three batches), K = 2 (one and two cells), f32 tables holding the two narrowest taps of each modality —
and the program that counts DevBuf's live allocations (a process of its own on the test-hooks variant, MFAS_LIB)."""
import numpy as np

R, C, B, N, K = 16, 5, 8, 24, 2
CONFS = [np.array([[0, 1, 0]]), np.array([[1, 0, 1], [0, 1, 2]])]
EPOCHS = 3


def workload(dev):
    """-> (hyper-parameters, train table, dev table, eta table of an EPOCHS-epoch schedule)"""
    import torch
    import mfas_amd as M
    from mfas_amd.engine import S_SIZES, V_SIZES
    from oracle import np_oracle as O
    hp = M.Hyper(R=R, C=C, B=B, bn=True, drpt=0.5)
    tr, dv = (M.FeatureTable.synthetic(N, seed, dev, torch.float32, snr=0.5, C=C, s_sizes=S_SIZES[:2], v_sizes=V_SIZES[:2]) for seed in (1, 2))
    return hp, tr, dv, O.eta_sequence(1e-3, 1e-6, 1, 2, N / B, EPOCHS * (N // B))


def live_allocations_program(root):
    """Runs in a process that loaded the test-hooks variant.  A resident population whose epoch 1 falls back to launch-per-phase (the
    not-resident hook launches nothing), with a kept-best plane; the same calls on a population created launch-per-phase; evaluate on
    the kept best; a move into a third population; all destroyed.  Prints LIVE_OK and the counts."""
    import ctypes
    import os
    import torch
    import mfas_amd as M
    from mfas_amd import _lib
    L = _lib.lib()
    assert _lib.tuning()["hooks"] == "1"
    L.mfas_test_live_allocations.restype = ctypes.c_int64
    live = L.mfas_test_live_allocations
    dev = torch.device("cuda:0")
    hp, tr, dv, etas = workload(dev)
    assert live() == 0

    def made(env, resident):
        """a population created under env that trains epochs [0, 2) of EPOCHS with a kept-best plane -> (it, the allocations it holds)"""
        before = live()
        os.environ.update(env)
        try:
            pop = M.Population(hp, CONFS, dev, drop_seeds=[5, 6])
        finally:
            for k in env:
                del os.environ[k]
        assert bool(pop.schedule()["persistent"]) == resident, pop.schedule()
        pop.init([1, 2])
        _, status = pop.train(tr, dv, EPOCHS, etas, snapshot_best=True, first_epoch=0, last_epoch=2)
        assert not status.any() and not pop.schedule()["persistent"]
        return pop, live() - before

    pop, held = made({"MFAS_PERSIST_TEST_NOT_RESIDENT": "1"}, True)       # epoch 0 resident, epoch 1 after persist_fallback
    ref, ref_held = made({"MFAS_PERSIST": "0"}, False)
    assert held == ref_held and held > 0, (held, ref_held)
    pop.evaluate(dv, members=[0, 1], plane=3, report=True)
    dst = M.Population(hp, CONFS, dev, drop_seeds=[7, 8])
    dst.move_from(pop, 1, 1)
    assert dst.get_progress(1)["epochs_done"] == 2 and torch.equal(dst.get_params(1, 3), pop.get_params(1, 3))
    assert live() > held + ref_held
    for p in (pop, ref, dst):
        p.close()
    assert live() == 0, live()
    print("LIVE_OK after_fallback=%d per_phase=%d end=%d" % (held, ref_held, live()))
