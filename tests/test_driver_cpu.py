"""The host driver's single statements (mfas_amd/driver.py, and pack_confs in engine.py), without a GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mfas_amd import driver as D
from mfas_amd import ntu_searchable as NS
from mfas_amd.engine import Hyper, cell_in_features, pack_confs
from mfas_amd.scheduler import LRCosineAnnealingScheduler

MIXED = [[[3, 1, 1], [1, 3, 0], [1, 1, 2], [3, 3, 0]], [[0, 2, 2]], [[2, 0, 0], [0, 1, 1]], [[1, 2, 2], [2, 3, 1], [0, 0, 0]]]


@pytest.mark.parametrize("cells", [0, 5])
def test_pack_confs_refuses_other_than_1_to_4_cells(cells):
    with pytest.raises(ValueError, match=r"^a configuration has 1\.\.4 fusion cells$"):
        pack_confs([np.zeros((1, 3), int), np.zeros((cells, 3), int)])


def test_pack_confs_arrays():
    """What Population.__init__ used to build in place: cf[k, :len] = conf, nc[k] = len, unused rows zero."""
    confs, cf, nc = pack_confs([np.array(c).reshape(-1) for c in MIXED])      # (flat input is reshaped to [cells, 3])
    assert cf.shape == (4, 4, 3) and cf.dtype == np.int32 and nc.dtype == np.int32
    assert nc.tolist() == [4, 1, 2, 3]
    for k, c in enumerate(MIXED):
        assert confs[k].dtype == np.int64 and confs[k].tolist() == c
        assert cf[k, :len(c)].tolist() == c
        assert not cf[k, len(c):].any()


def test_etas_for_cosine_is_the_schedulers_table():
    sched = LRCosineAnnealingScheduler(1e-3, 1e-6, 1, 2, 65 / 20)
    want = LRCosineAnnealingScheduler(1e-3, 1e-6, 1, 2, 65 / 20).eta_table(3 * 4)
    got = D.etas_for(sched, None, 3, 4)
    assert np.array_equal(np.asarray(got), np.asarray(want))


def test_etas_for_other_schedulers_step_once_per_epoch():
    lr0 = 1e-3
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5)
    with pytest.warns(UserWarning):      # (torch's: scheduler.step() before optimizer.step())
        got = D.etas_for(sched, opt, 3, 4)
    assert got == [lr0 * 0.125] * 12
    assert sched.last_epoch == 3 and opt.param_groups[0]["lr"] == lr0 * 0.125


def test_torch_init_bounds_are_linear_init_bounds_of_the_cell_fan_ins():
    hp = Hyper(R=32, s_sizes=(16, 48, 100, 32), v_sizes=(64, 96, 24, 80))
    for conf in MIXED:
        conf = np.asarray(conf)
        got = D.torch_init_bounds(conf, hp)
        want = np.zeros(10, np.float32)
        for i in range(len(conf)):
            want[2 * i], want[2 * i + 1] = D.linear_init_bounds(cell_in_features(conf, i, hp))
        want[8], want[9] = D.linear_init_bounds(hp.R)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    # torch's own expressions (nn.Linear.reset_parameters: kaiming_uniform_(a = sqrt 5); 1 / sqrt(fan_in))
    gain = torch.nn.init.calculate_gain("leaky_relu", math.sqrt(5))
    assert D.linear_init_bounds(80) == (math.sqrt(3.0) * (gain / math.sqrt(80)), 1 / math.sqrt(80))


def test_train_one_closes_the_population_when_train_raises(monkeypatch):
    calls = []

    class FakePopulation:
        def __init__(self, hp, confs, device, drop_seeds=None):
            calls.append(("create", len(confs), list(drop_seeds)))

        def set_params(self, k, flat):
            calls.append("set_params")

        def train(self, *a, **kw):
            assert kw["snapshot_best"] is True
            raise RuntimeError("train failed")

        def close(self):
            calls.append("close")

    monkeypatch.setattr(D, "Population", FakePopulation)
    model = SimpleNamespace(conf=np.array([[0, 0, 0]]), flat_params=lambda: torch.zeros(3))
    loader = SimpleNamespace(table=[0] * 65, shuffle=False)
    with pytest.raises(RuntimeError, match="train failed"):
        D.train_one(model, Hyper(B=20), loader, loader, 2, [1e-3] * 8, "cpu", drop_seed=(1 << 32) + 5, order_seed=6)
    assert calls == [("create", 1, [5]), "set_params", "close"]


def test_reexported_driver_state_is_shared():
    assert NS.PROFILE is D.PROFILE and NS.RUNG_CHANGES is D.RUNG_CHANGES and NS._DEVICE_STREAMS_OK is D._DEVICE_STREAMS_OK
    assert NS.train_sampled_models is D.train_sampled_models
