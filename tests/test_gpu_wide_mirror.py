"""The Python mirror and the CLI at batch sizes and widths that take (or border on) the wide path: the found-architecture script at
its default representation size with batch 64, and train_sampled_models at R = 128 / 177, B = 64 against the float32 oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import np_oracle as O
from tests.helpers import CONFS
from tests.gpu_dev import dev  # noqa: F401
from tests.mirror_gpu import loaders, mkargs

pytestmark = pytest.mark.gpu


def test_found_ntu_cli_default_width_at_batch_64():
    """main_found_ntu.py at --inner_representation_size 256 (its default) and --batchsize 64 — refused before — runs to an accuracy."""
    import main_found_ntu
    acc = main_found_ntu.main(["--synthetic", "200", "83", "83", "--inner_representation_size", "256", "--batchsize", "64",
                               "--epochs", "2", "--no-verbose"])
    assert 0.0 <= float(acc) <= 1.0


@pytest.mark.parametrize("R", [128, 177])
def test_train_sampled_models_batch_64_matches_oracle(dev, R):
    """Four sampled configurations at B = 64, deterministic mode (BatchNorm, no dropout, no shuffling, the modules' own initial
    parameters): the float32 oracle's best dev count within one sample per candidate (the G12 convention for a path that differs
    from the oracle only in summation order).  R = 128 is the headline width (batch-resident kernels); R = 177 is its nearest
    neighbour that does not fit them and takes the wide path."""
    import mfas_amd as M
    args = mkargs(batchnorm=True, drpt=0.0, epochs=2, inner_representation_size=R, batchsize=64)
    n_tr, n_dev = 200, 83
    ttr, tdv = O.synth_table(n_tr, 51, snr=0.5), O.synth_table(n_dev, 52, snr=0.5)
    ld = loaders(ttr, tdv, dev, 64, shuffle=False)
    confs = [np.array(CONFS[c]) for c in ("l1", "l2", "l3", "c4")]
    torch.manual_seed(11)
    pre = [M.Searchable_Skeleton_Image_Net(args, c) for c in confs]
    sd0 = [{k: v.detach().numpy().copy() for k, v in m.state_dict().items() if "num_batches" not in k} for m in pre]
    got = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev, premodels=pre)
    ohp = O.Hyper(R=R, B=64, bn=True, drpt=0.0, epochs=2)
    for k, conf in enumerate(confs):
        want = O.train_candidate(conf, ohp, sd0[k], ttr, tdv)
        assert abs(got[k] - want) <= 1.0 / n_dev + 1e-9, (R, k, got[k], want)
