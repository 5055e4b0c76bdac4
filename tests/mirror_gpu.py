"""Device plumbing of the mirror tests: the argument namespace and the loaders."""
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")


def mkargs(**kw):
    a = dict(vid_len=(8, 32), num_outputs=60, drpt=0.5, inner_representation_size=16, batchnorm=False,
             alphas=False, multitask=False, weightsharing=False, batchsize=16, eta_max=1e-3, eta_min=1e-6,
             Ti=1, Tm=2, use_dataparallel=False, verbose=False, epochs=3)
    a.update(kw)
    return SimpleNamespace(**a)


def loaders(ttr, tdv, dev, B, shuffle=True, dtype=torch.float32):
    import mfas_amd as M
    return {"train": M.FeatureLoader(M.FeatureTable.from_numpy(ttr, dev, dtype), B, shuffle=shuffle),
            "dev": M.FeatureLoader(M.FeatureTable.from_numpy(tdv, dev, dtype), B, shuffle=False),
            "test": M.FeatureLoader(M.FeatureTable.from_numpy(tdv, dev, dtype), B, shuffle=False)}
