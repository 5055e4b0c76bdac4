"""The host drivers — train_sampled_models (NTU, AV-MNIST, MM-IMDB), train_ntu_track_acc, train_mmimdb_track_f1 — decide seeds, sample
orders, initial parameters, eta tables, what a returned model holds and what is printed; the library does the arithmetic.  A restatement
of that host layer changes no value, so everything a driver call returns, leaves in a model or prints must equal, BYTE FOR BYTE, what the
drivers gave before: tests/golden/driver_digests.json holds, per case, SHA-256 digests of those, written by this module run as a script
(`python -m tests.test_gpu_driver_digests --record`) at the commit before the restatement.

Only names spelled alike before and after are used (mfas_amd.train_sampled_models, .train_ntu_track_acc, .mmimdb_searchable.*,
.avmnist_searchable.*, .Searchable_Skeleton_Image_Net, .FeatureTable / .FeatureLoader).  Tables come from numpy seeds; the drivers draw
their seeds from torch's global stream, so torch.manual_seed goes immediately before every driver call, and the JSON names the torch
version it was recorded with: under another one the generators may differ and the test FAILS asking for a new record at the parent.

Beside what each case lists, every case digests the statistics and status words of all Population.train calls the drivers made
(run_case): float64 loss sums see what accuracies out of 41 samples cannot.  The planted signal (1.5 sigma) and eta_max = 1e-2 make two
epochs learn something, so the accuracies differ between candidates and cases.

Shapes (all cases): R = 16, B = 20, N_train = 65 (3 batches and a ragged one of 5), N_dev = 41, E = 2, engine_chunk_cols = 64; NTU taps of
16..96 columns, every width a multiple of 16; AV-MNIST with channels = 3 (taps of 3..48 columns); MM-IMDB's fixed 64 / 128 / 512."""
import contextlib
import hashlib
import io
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.gpu_dev import dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_digests.json")
S_W, V_W = (16, 48, 96, 32), (64, 96, 32, 80)
C, R, B, E, N_TR, N_DEV = 10, 16, 20, 2, 65, 41
CONFS = [np.array(c) for c in ([[0, 2, 2]], [[2, 0, 0], [0, 1, 1]], [[1, 2, 2], [2, 3, 1], [0, 0, 0]],
                               [[3, 1, 1], [1, 3, 0], [1, 1, 2], [3, 3, 0]], [[0, 3, 0], [1, 0, 2], [3, 2, 1], [2, 2, 2]])]      # depths 1, 2, 3, 4, 4
SHARING = [np.array(c) for c in ([[0, 0, 0]], [[0, 0, 0], [1, 1, 1]], [[0, 0, 0], [1, 1, 1], [2, 2, 0]])]      # later candidates load earlier cells
AV_CONFS = [np.array(c) for c in ([[4, 2, 1]], [[3, 1, 0], [4, 2, 1]], [[0, 0, 0], [2, 1, 1], [1, 2, 0]])]
MM_CONFS = [np.array(c) for c in ([[0, 0, 0]], [[1, 2, 1], [0, 3, 0]], [[1, 1, 0], [1, 3, 1], [0, 0, 0]])]
POS_WEIGHT = [1.0 + 0.25 * c for c in range(23)]


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


SEEN = []      # the figures of the case that ran last, for --record's printout


def f64(values):
    out = np.asarray([float(v) for v in values], np.float64)
    SEEN.append(out.tolist())
    return out


def np_table(n, seed, s_sizes, v_sizes, nclass, multilabel=False):
    rng = np.random.default_rng(seed)
    label = rng.integers(0, nclass, n)
    t = {"label": label.astype(np.int32)}
    for name, sizes in (("s", s_sizes), ("v", v_sizes)):
        for j, w in enumerate(sizes):
            mu = np.random.default_rng(1000 + 10 * (name == "v") + j).standard_normal((nclass, w))
            t[f"{name}{j}"] = np.maximum(1.5 * mu[label] + rng.standard_normal((n, w)), 0.0).astype(np.float32)
    if multilabel:
        ml = np.zeros((n, nclass), np.float32)
        ml[np.arange(n), label] = 1.0
        t["multilabel"] = np.maximum(ml, (rng.random((n, nclass)) < 0.15).astype(np.float32))
    return t


# (tests/mirror_gpu.py's loaders takes tables; this one draws its own of the given widths, with multi-hot targets on request)
def loaders(dev, s_sizes, v_sizes, nclass, multilabel=False):
    import torch
    import mfas_amd as M
    out = {}
    for split, n, seed in (("train", N_TR, 41), ("dev", N_DEV, 42)):
        t = np_table(n, seed, s_sizes, v_sizes, nclass, multilabel)
        table = M.FeatureTable.from_numpy(t, dev)
        if multilabel:
            table.multilabel = torch.from_numpy(t["multilabel"]).to(dev).contiguous()
        out[split] = M.FeatureLoader(table, B, shuffle=(split == "train"))
    return out


def ntu_args(**kw):
    base = dict(vid_len=(8, 32), num_outputs=C, drpt=0.5, inner_representation_size=R, batchnorm=False, alphas=False, multitask=False,
                weightsharing=False, batchsize=B, eta_max=1e-2, eta_min=1e-6, Ti=1, Tm=2, use_dataparallel=False, verbose=False,
                epochs=E, s_sizes=S_W, v_sizes=V_W, engine_chunk_cols=64)
    base.update(kw)
    return SimpleNamespace(**base)


def model_digests(models):
    out = {}
    for n, m in enumerate(models):
        import torch
        out[f"model{n}.flat"] = sha(m.flat_params().numpy())
        out[f"model{n}.bn_counters"] = sha(np.asarray([int(b.num_batches_tracked) for b in m.modules()
                                                       if isinstance(b, torch.nn.BatchNorm1d)], np.int64))
        out[f"model{n}.training"] = sha(np.asarray([int(x.training) for x in m.modules()], np.int8))
    return out


def captured(fn):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn()
    return out, buf.getvalue()


def _ts(dev, seed, confs, args, **kw):
    import torch
    import mfas_amd as M
    ld = loaders(dev, S_W, V_W, C)
    torch.manual_seed(seed)
    return M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev, **kw)


def case_ts_default(dev):
    return {"accuracies": sha(f64(_ts(dev, 11, CONFS, ntu_args())))}


def case_ts_bn_return(dev):
    accs, models = _ts(dev, 12, CONFS, ntu_args(batchnorm=True), return_model=[0, 2])
    return {"accuracies": sha(f64(accs)), **model_digests(models)}


def case_ts_shared(dev):
    return {"accuracies": sha(f64(_ts(dev, 13, CONFS, ntu_args(engine_order="shared"))))}


def case_ts_device_init(dev):
    return {"accuracies": sha(f64(_ts(dev, 14, CONFS, ntu_args(engine_init="device"))))}


def case_ts_premodels(dev):
    import torch
    import mfas_amd as M
    args = ntu_args()
    pre = []
    for i, c in enumerate(CONFS):
        torch.manual_seed(100 + i)
        pre.append(M.Searchable_Skeleton_Image_Net(args, c))
    return {"accuracies": sha(f64(_ts(dev, 15, CONFS, args, premodels=pre)))}


def case_ts_halving(dev):
    return {"accuracies": sha(f64(_ts(dev, 16, CONFS[:4], ntu_args(engine_halving=(2, (1,))))))}


def case_ts_sharing(dev):
    shared = {}
    accs, models = _ts(dev, 17, SHARING, ntu_args(weightsharing=True), return_model=[0, 1, 2], state_dict=shared)
    out = {"accuracies": sha(f64(accs)), **model_digests(models), "state_dict.keys": sha("\n".join(sorted(shared)).encode())}
    for name in sorted(shared):
        for key in sorted(shared[name]):
            out[f"state_dict.{name}.{key}"] = sha(shared[name][key].detach().cpu().numpy())
    return out


def case_ts_verbose(dev):
    accs, text = captured(lambda: _ts(dev, 18, CONFS[:2], ntu_args(verbose=True)))
    return {"accuracies": sha(f64(accs)), "stdout": sha(text.encode())}


def case_ts_avmnist(dev):
    import torch
    from mfas_amd import avmnist_searchable as AV
    ld = loaders(dev, *AV.av_sizes(3), C)
    out = {}
    for drpt in (0.5, 0.0):      # [Linear, nl, Dropout] cells, then plain [Linear, nl] ones
        args = ntu_args(channels=3, drpt=drpt)
        del args.s_sizes, args.v_sizes
        torch.manual_seed(19)
        out[f"accuracies.drpt{drpt}"] = sha(f64(AV.train_sampled_models(AV_CONFS, AV.Searchable_Audio_Image_Net, ld, args, dev)))
    return out


def mm_args(**kw):
    args = ntu_args(num_outputs=23, pos_weight=list(POS_WEIGHT), **kw)
    del args.s_sizes, args.v_sizes
    return args


def case_ts_mmimdb(dev):
    import torch
    from mfas_amd import mmimdb_searchable as MM
    ld = loaders(dev, MM.MM_TEXT_SIZES, MM.MM_IMAGE_SIZES, 23, multilabel=True)
    torch.manual_seed(20)
    return {"f1": sha(f64(MM.train_sampled_models(MM_CONFS, MM.Searchable_Text_Image_Net, ld, mm_args(), dev)))}


def _track_acc(dev, seed, make_scheduler):
    import torch
    import mfas_amd as M
    args = ntu_args(batchnorm=True)
    ld = loaders(dev, S_W, V_W, C)
    torch.manual_seed(seed)
    model = M.Searchable_Skeleton_Image_Net(args, CONFS[2])
    opt = torch.optim.Adam(model.central_params(), lr=1e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-3)
    sched = make_scheduler(opt)
    torch.manual_seed(seed + 1000)
    best, text = captured(lambda: M.train_ntu_track_acc(model, torch.nn.CrossEntropyLoss(), opt, sched, ld, {"train": N_TR, "dev": N_DEV},
                                                        device=dev, num_epochs=E, verbose=True))
    assert best.dtype == torch.float64 and best.dim() == 0
    return {"returned": sha(best.numpy()), **model_digests([model]), "stdout": sha(text.encode()),
            "lr_after": sha(f64([opt.param_groups[0]["lr"]]))}


def case_track_acc_cos(dev):
    import mfas_amd as M
    return _track_acc(dev, 21, lambda opt: M.LRCosineAnnealingScheduler(1e-3, 1e-6, 1, 2, N_TR / B))


def case_track_acc_step(dev):
    import torch
    return _track_acc(dev, 22, lambda opt: torch.optim.lr_scheduler.StepLR(opt, 1, 0.5))


def case_track_f1(dev):
    import torch
    import mfas_amd as M
    from mfas_amd import mmimdb_searchable as MM
    args = mm_args(batchnorm=True)
    ld = loaders(dev, MM.MM_TEXT_SIZES, MM.MM_IMAGE_SIZES, 23, multilabel=True)
    torch.manual_seed(23)
    model = MM.Searchable_Text_Image_Net(args, MM_CONFS[1])
    opt = torch.optim.Adam(model.central_params(), lr=1e-3, weight_decay=1e-3)
    sched = M.LRCosineAnnealingScheduler(1e-3, 1e-6, 1, 2, N_TR / B)
    torch.manual_seed(1023)
    best, text = captured(lambda: MM.train_mmimdb_track_f1(model, MM.WeightedCrossEntropyWithLogits(POS_WEIGHT), opt, sched, ld,
                                                           {"train": N_TR, "dev": N_DEV}, device=dev, num_epochs=E, verbose=True, init_f1=0.1))
    return {"returned": sha(f64([best])), **model_digests([model]), "stdout": sha(text.encode())}


CASES = {"ts-default": case_ts_default, "ts-bn-return": case_ts_bn_return, "ts-shared": case_ts_shared,
         "ts-device-init": case_ts_device_init, "ts-premodels": case_ts_premodels, "ts-halving": case_ts_halving,
         "ts-sharing": case_ts_sharing, "ts-verbose": case_ts_verbose, "ts-avmnist": case_ts_avmnist, "ts-mmimdb": case_ts_mmimdb,
         "track-acc-cos": case_track_acc_cos, "track-acc-step": case_track_acc_step, "track-f1": case_track_f1}


def run_case(name, dev):
    """The case's digests, and one over the statistics and status words of every Population.train call the drivers made, in call order:
    the loss sums are float64 sums over every sample of every epoch, so they move with any seed, order, eta or initial value (the
    accuracies, counts out of 41, are coarse)."""
    import mfas_amd as M
    real_train, seen = M.Population.train, []

    def spy(self, *a, **kw):
        out = real_train(self, *a, **kw)
        seen.extend([np.ascontiguousarray(out[0]).tobytes(), np.ascontiguousarray(out[1]).tobytes()])
        return out

    M.Population.train = spy
    try:
        got = CASES[name](dev)
    finally:
        M.Population.train = real_train
    assert seen, name
    return {**got, "population.train": sha(*seen)}


@pytest.fixture(scope="module")
def golden():
    import torch
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["torch_version"] == torch.__version__, (
        f"tests/golden/driver_digests.json was recorded with torch {g['torch_version']}, this is {torch.__version__}: the drivers' seeds and "
        "initial parameters come from torch's generators, so record again at the commit before the drivers were restated "
        "(python -m tests.test_gpu_driver_digests --record)")
    return g["cases"]


@pytest.mark.parametrize("name", list(CASES))
def test_driver_bit_identical(dev, golden, name):
    got = run_case(name, dev)
    want = golden[name]
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    differ = [key for key in sorted(got) if got[key] != want[key]]
    assert not differ, (name, "differs from the recorded drivers in", differ)


def record(path=GOLDEN):
    import torch
    dev = torch.device("cuda:0")
    cases = {}
    for name in CASES:
        del SEEN[:]
        cases[name] = run_case(name, dev)
        print(f"{name:16s} {len(cases[name])} digests; figures {SEEN}", flush=True)
    with open(path, "w") as f:
        json.dump({"torch_version": torch.__version__, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {path}")
    return 0


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, \
        "usage: python -m tests.test_gpu_driver_digests --record [FILE]   (at the commit before the restatement)"
    sys.exit(record(*sys.argv[2:]))
