"""GPU tests of the Python mirror of the reference interface (mfas_amd.train_sampled_models & friends) and of the
stochastic (dropout + shuffle) parity gate against the reference's own seed statistics (G10)."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import np_oracle as O
from tests.helpers import CONFS, golden
from tests.mirror_gpu import loaders, mkargs
from tests.gpu_dev import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def test_train_sampled_models_signature_and_determinism(dev):
    import mfas_amd as M
    args = mkargs(batchnorm=True, drpt=0.0, epochs=3)
    ttr, tdv = O.synth_table(256, 31, snr=0.5), O.synth_table(128, 32, snr=0.5)
    ld = loaders(ttr, tdv, dev, 16, shuffle=False)
    confs = [np.array(CONFS[c]) for c in ("l1", "l2", "l3", "c4")]
    torch.manual_seed(7)
    a = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev, state_dict=dict())
    torch.manual_seed(7)
    b = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev)
    assert a == b and len(a) == 4 and all(isinstance(x, float) and 0.0 <= x <= 1.0 for x in a)
    assert np.array(a).shape == (4,) and max(a[0], a[1]) >= a[0]           # what tools.py / surrogate.py do with them
    # device-side init path (bench) trains too
    args2 = mkargs(batchnorm=True, drpt=0.0, epochs=3, engine_init="device")
    torch.manual_seed(7)
    c = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args2, dev)
    assert len(c) == 4 and min(c) > 2.0 / 60      # clearly above chance after 3 short epochs
    with pytest.raises(TypeError):
        M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev, preaccuracies=[0.1] * 4)
    with pytest.raises(TypeError):
        M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, {"train": [1], "dev": [2]}, args, dev)


def test_init_from_module_matches_oracle_run(dev):
    """The module's torch-initialised parameters are what the engine trains: same params into the oracle ->
    same dev counts."""
    import mfas_amd as M
    args = mkargs(batchnorm=True, drpt=0.0, epochs=2)
    ttr, tdv = O.synth_table(128, 41, snr=0.5), O.synth_table(96, 42, snr=0.5)
    ld = loaders(ttr, tdv, dev, 16, shuffle=False)
    conf = np.array(CONFS["l2"])
    torch.manual_seed(3)
    model = M.Searchable_Skeleton_Image_Net(args, conf)
    sd0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if "num_batches" not in k}
    opt = torch.optim.Adam(model.central_params(), lr=args.eta_max, weight_decay=1e-4)
    sched = M.LRCosineAnnealingScheduler(args.eta_max, args.eta_min, args.Ti, args.Tm, 128 / 16)
    acc = M.train_ntu_track_acc(model, torch.nn.CrossEntropyLoss(), opt, sched, ld, {"train": 128, "dev": 96},
                                device=dev, num_epochs=2)
    ohp = O.Hyper(R=16, B=16, bn=True, drpt=0.0, epochs=2)
    hist = []
    want = O.train_candidate(conf, ohp, {k: v.copy() for k, v in sd0.items()}, ttr, tdv, history=hist)
    assert abs(float(acc) - want) <= 1.0 / 96 + 1e-9
    assert acc.dtype == torch.float64 and not model.training
    # best-epoch weights were restored into the module: test accuracy == best dev accuracy (same table)
    tacc = M.test_ntu_track_acc(model, ld, {"test": 96}, device=dev)
    assert abs(float(tacc) - float(acc)) < 1e-12
    # eval-mode Module.forward runs on the engine and agrees with the oracle on the restored weights
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if "num_batches" not in k}
    feats = {k: torch.from_numpy(tdv[k][:32]).to(dev) for k in tdv if k != "label"}
    out = model(({k: v for k, v in feats.items() if k[0] == "v"}, {k: v for k, v in feats.items() if k[0] == "s"}))
    ref, _ = O.forward(sd, conf, ohp, {k: tdv[k][:32] for k in tdv if k != "label"}, False)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=2e-4, atol=2e-5)


def test_return_model_and_weightsharing(dev):
    import mfas_amd as M
    args = mkargs(batchnorm=True, drpt=0.0, epochs=2)
    ttr, tdv = O.synth_table(128, 41, snr=0.5), O.synth_table(96, 42, snr=0.5)
    ld = loaders(ttr, tdv, dev, 16)
    confs = [np.array(CONFS["l1"]), np.array(CONFS["l2"]), np.array(CONFS["l3"])]
    torch.manual_seed(1)
    accs, models = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev, return_model=[0, 2])
    assert len(accs) == 2 and len(models) == 2
    for a, m in zip(accs, models):
        assert abs(float(M.test_ntu_track_acc(m, ld, {"test": 96}, device=dev)) - a) < 1e-12
        assert int(m.fusion_layers[0][2].num_batches_tracked) == 2 * 8
    # weight sharing: serial, cells published under "{idx}.L_{in}_{out}.A_{act}"
    args_ws = mkargs(batchnorm=True, drpt=0.0, epochs=1, weightsharing=True)
    shared = dict()
    torch.manual_seed(1)
    accs = M.train_sampled_models([confs[0], confs[0]], M.Searchable_Skeleton_Image_Net, ld, args_ws, dev,
                                  state_dict=shared)
    assert "0.L_640_16.A_relu" in shared and len(accs) == 2
    assert accs[1] >= accs[0] - 0.05     # the second copy starts from the first one's trained cell


def test_stochastic_parity_vs_reference_seed_statistics(dev):
    """Parity gate, stochastic mode: dropout + shuffle streams cannot match torch's, so the MEAN best
    dev accuracy over many engine seeds must sit inside the reference's own seed distribution (G10: mean +- 3 s.e.
    of the reference sample, plus 0.1 % top-1)."""
    import mfas_amd as M
    g = golden("g10_stochastic.npz")
    for tag in ("B", "A"):
        N, Nd, snr, R, B, E, bn, drpt = g[tag + "/meta"]
        ref = g[tag + "/accs"]                       # (seeds, confs)
        ttr, tdv = O.synth_table(int(N), 1, snr=float(snr)), O.synth_table(int(Nd), 2, snr=float(snr))
        ld = loaders(ttr, tdv, dev, int(B), shuffle=True)
        args = mkargs(inner_representation_size=int(R), batchnorm=bool(bn), drpt=float(drpt), epochs=int(E),
                      batchsize=int(B), engine_init="device")
        nconf = ref.shape[1]
        reps = 96
        confs = [g[f"{tag}/conf{i}"] for i in range(nconf)] * reps
        torch.manual_seed(11)
        accs = np.array(M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev)).reshape(reps, nconf)
        for i in range(nconf):
            se_ref = ref[:, i].std(ddof=1) / np.sqrt(ref.shape[0])
            se_eng = accs[:, i].std(ddof=1) / np.sqrt(reps)
            tol = 3.0 * np.hypot(se_ref, se_eng) + 0.001
            assert abs(accs[:, i].mean() - ref[:, i].mean()) <= tol, (tag, i, accs[:, i].mean(), ref[:, i].mean(), tol)
            # the spread must be of the reference's order too (neither collapsed nor blown up)
            assert 0.4 * ref[:, i].std(ddof=1) <= accs[:, i].std(ddof=1) <= 2.5 * ref[:, i].std(ddof=1), (tag, i)


def test_cli_entry_points_and_table_io(dev, tmp_path):
    """main_searchable_ntu / main_found_ntu counterparts run end to end on small synthetic tables; the on-disk
    feature-table format round-trips bit-exactly."""
    import mfas_amd as M
    import main_found_ntu
    import main_searchable_ntu
    t = M.FeatureTable.synthetic(96, 5, dev, torch.bfloat16, snr=0.5, with_logits=True)
    t.save(str(tmp_path), "train")
    u = M.FeatureTable.load(str(tmp_path), "train", dev)
    assert u.dtype == torch.bfloat16 and torch.equal(u.label, t.label)
    for k in t.taps:
        assert torch.equal(u.taps[k].view(torch.int16), t.taps[k].view(torch.int16))
    assert torch.equal(u.vlogit, t.vlogit)
    data = main_searchable_ntu.main(["--synthetic", "640", "320", "--epochs", "1", "--search_iterations", "1",
                                     "--max_fusions", "2", "--num_samples", "4", "--epochs_surrogate", "3",
                                     "--batchnorm", "--no-verbose", "--engine_init", "device"])
    confs, accs, _ = data.get_k_best(3)
    assert len(confs) == 3 and all(0.0 <= a <= 1.0 for a in accs)
    # the same search with the surrogate's train steps replayed as HIP graphs on the device
    data = main_searchable_ntu.main(["--synthetic", "640", "320", "--epochs", "1", "--search_iterations", "1",
                                     "--max_fusions", "2", "--num_samples", "4", "--epochs_surrogate", "3",
                                     "--no-verbose", "--surrogate_device", "gpu"])
    confs, accs, _ = data.get_k_best(3)
    assert len(confs) == 3 and all(0.0 <= a <= 1.0 for a in accs)
    acc = main_found_ntu.main(["--synthetic", "640", "320", "320", "--conf", "4", "--inner_representation_size", "32",
                               "--batchnorm", "--epochs", "2", "--batchsize", "16", "--no-verbose"])
    assert 0.0 <= float(acc) <= 1.0


DIST_WORKER = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from types import SimpleNamespace
import mfas_amd as M
world = int(os.environ.get("WORLD_SIZE", "1"))
backend = os.environ.get("MFAS_TEST_BACKEND", "gloo")
rank = int(os.environ.get("RANK", "0"))
dev = torch.device("cuda", rank if backend == "nccl" else 0)      # nccl (= RCCL): one GPU per rank; gloo: both ranks on cuda:0
torch.cuda.set_device(dev)
if world > 1:
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
args = SimpleNamespace(vid_len=(8, 32), num_outputs=60, drpt=0.5, inner_representation_size=16, batchnorm=True,
                       alphas=False, multitask=False, weightsharing=False, batchsize=16, eta_max=1e-3, eta_min=1e-6,
                       Ti=1, Tm=2, use_dataparallel=False, verbose=False, epochs=2, engine_init="device",
                       engine_all_ranks=bool(int(os.environ.get("MFAS_TEST_ALL_RANKS", "1"))))
tr = M.FeatureTable.synthetic(512, 1, dev, torch.bfloat16, snr=0.5)
dv = M.FeatureTable.synthetic(256, 2, dev, torch.bfloat16, snr=0.5)
ld = {{"train": M.FeatureLoader(tr, 16, shuffle=True), "dev": M.FeatureLoader(dv, 16, shuffle=False)}}
rng = np.random.default_rng(0)
confs = [np.stack([rng.integers(0, 4, L), rng.integers(0, 4, L), rng.integers(0, 2, L)], 1) for L in (1, 2, 3, 4, 4, 2, 1)]
torch.manual_seed(5)
import mfas_amd.driver as _ns
_ns._TEST_FAIL_RANK = int(os.environ.get("MFAS_TEST_FAIL_RANK", "-1"))      # the failure is injected by the TEST (module attribute), never by the product reading the environment
accs = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev)
from mfas_amd import population as P
hp = M.Hyper.from_args(args)
hp.multitask, hp.tap_bits = False, 16        # (what train_sampled_models derives for these tables: the same calibrated model)
owner, _, model = P.shard_call(confs, hp, world, dev, args.engine_all_ranks)
if model is not None:
    print("MODEL", json.dumps(model.describe()), flush=True)
print("RESULT", json.dumps(accs), flush=True)
print("SHARE", json.dumps([owner.count(r) for r in range(world)]), "BACKEND", dist.get_backend() if world > 1 else "none", flush=True)
if world > 1:
    dist.destroy_process_group()
"""


def test_population_sharding_two_ranks_matches_single(dev, tmp_path):
    """N>1 path end to end on the GPU box: 2 processes (gloo rendezvous on 127.0.0.1; both use cuda:0) shard the
    population, train their shares in the HIP engine, all-gather the accuracies — and get bit-for-bit what one
    process gets (seeds are broadcast, so results do not depend on the world size)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "w.py"
    script.write_text(DIST_WORKER.format(root=root))

    single = _run_dist(script, 1)[0][0]
    two, shares = _run_dist(script, 2)
    assert two[0] == two[1] == single and len(single) == 7
    assert shares[0][0] == [4, 3] or sorted(shares[0][0]) == [3, 4]          # really sharded (engine_all_ranks)
    # the sharder's own policy: 7 search-sized candidates cost one rank the same step time as 4 + 3 on two (a latency-bound
    # step is flat up to 8 resident candidates, mfas_amd/population.py) -> the call uses ONE rank, the other only joins the gather
    lazy, shares = _run_dist(script, 2, MFAS_TEST_ALL_RANKS="0")
    assert lazy[0] == lazy[1] == single and shares[0][0] == [7, 0]
    # a rank whose share fails (hook: rank 1's first attempt raises) is re-queued on the other one — same accuracies, nobody hangs
    requeued, _ = _run_dist(script, 2, MFAS_TEST_FAIL_RANK="1")
    assert requeued[0] == requeued[1] == single


def _run_dist(script, world, **extra):
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29577", WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    outs, shares = [], []
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out.decode()[-2000:]
        lines = out.decode().splitlines()
        line = [l for l in lines if l.startswith("RESULT")][-1]
        outs.append(json.loads(line[len("RESULT "):]))
        sh = [l for l in lines if l.startswith("SHARE")][-1].split(" BACKEND ")
        shares.append((json.loads(sh[0][len("SHARE "):]), sh[1].strip()))
    return outs, shares


def test_population_sharding_two_ranks_rccl(dev, tmp_path):
    """The same over RCCL (torch.distributed backend "nccl"), one GPU per rank: runs wherever the box has >= 2 GPUs (the driver's
    8-GPU node); skipped on the 1-GPU boxes the builder gets."""
    import os
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL: one process per GPU)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "w.py"
    script.write_text(DIST_WORKER.format(root=root))
    single = _run_dist(script, 1)[0][0]
    two, shares = _run_dist(script, 2, MFAS_TEST_BACKEND="nccl")
    assert two[0] == two[1] == single
    assert shares[0][1] == "nccl" and sorted(shares[0][0]) == [3, 4]


def test_global_pooling_kernel(dev):
    """GlobalPooling2D on the GPU: NTU tap shapes, all dtypes, odd inner sizes; plus its bandwidth."""
    import time
    from mfas_amd.pooling import build_feature_table, global_pool
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for shape in [(3, 128, 4, 4), (2, 512, 8, 32, 32), (5, 7, 13), (4, 256, 2, 2), (2, 1024), (3, 9, 1001)]:
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            x = torch.randn(shape, generator=g, device=dev).to(dt)
            got = global_pool(x, torch.float32)
            want = x.float().reshape(shape[0], shape[1], -1).mean(2) if len(shape) > 2 else x.float()
            torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-6)
    x = torch.randn(4, 64, 8, 16, 16, generator=g, device=dev)
    assert global_pool(x, torch.bfloat16).dtype == torch.bfloat16
    torch.testing.assert_close(global_pool(x, torch.bfloat16).float(), x.reshape(4, 64, -1).mean(2), rtol=1e-2, atol=1e-3)
    raw = {"s0": torch.randn(6, 128, 4, 4, device=dev), "v0": torch.randn(6, 512, 2, 8, 8, device=dev)}
    t = build_feature_table(raw, torch.zeros(6, dtype=torch.int32, device=dev))
    assert t.taps["v0"].shape == (6, 512) and t.dtype == torch.bfloat16
    big = torch.randn(16, 512, 8, 32, 32, device=dev)          # v0-shaped: 16 samples x 16.8 MB
    global_pool(big)
    torch.cuda.synchronize()
    gbs = 0.0
    for _ in range(5):      # best of five rounds: a correctness suite must not fail because the box was busy for a moment
        t0 = time.perf_counter()
        for _ in range(10):
            global_pool(big)
        torch.cuda.synchronize()
        gbs = max(gbs, big.numel() * 4 * 10 / (time.perf_counter() - t0) / 1e9)
    print(f"global_pool: {gbs:.0f} GB/s on a 268 MB f32 tap")
    assert gbs > 500        # (sanity bound: the kernel streams at ~6 TB/s, a per-element loop would not reach 50 GB/s)


def test_generic_pooled_tap_loader_is_accepted(dev):
    """dataloaders may be any iterable of reference-shaped batches {'rgb','ske','label'} carrying pooled
    taps (here a torch DataLoader over a dict Dataset): drained once into a HIP table, same result as a FeatureLoader."""
    import mfas_amd as M
    from types import SimpleNamespace

    t = O.synth_table(96, 41, snr=1.0)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 96

        def __getitem__(self, i):
            return {"rgb": {k: torch.from_numpy(t[k][i]) for k in ("v0", "v1", "v2", "v3")},
                    "ske": {k: torch.from_numpy(t[k][i]) for k in ("s0", "s1", "s2", "s3")},
                    "label": int(t["label"][i])}

    args = SimpleNamespace(vid_len=(8, 32), num_outputs=60, drpt=0.0, inner_representation_size=16, batchnorm=True,
                           alphas=False, multitask=False, weightsharing=False, batchsize=16, eta_max=1e-3, eta_min=1e-6,
                           Ti=1, Tm=2, use_dataparallel=False, verbose=False, epochs=2, engine_init="device")
    confs = [np.array(CONFS["c4"]), np.array(CONFS["l2"])]
    generic = {"train": torch.utils.data.DataLoader(DS(), batch_size=16, shuffle=False),
               "dev": torch.utils.data.DataLoader(DS(), batch_size=16, shuffle=False)}
    tab = M.FeatureTable.from_numpy(t, dev)
    fast = {"train": M.FeatureLoader(tab, 16, shuffle=False), "dev": M.FeatureLoader(tab, 16, shuffle=False)}
    M.train_sampled_models(confs[:1], M.Searchable_Skeleton_Image_Net, generic, args, dev)   # drains the loaders (a DataLoader draws from the torch RNG)
    torch.manual_seed(3)
    a = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, generic, args, dev)
    torch.manual_seed(3)
    b = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, fast, args, dev)
    assert a == b and all(0.0 <= x <= 1.0 for x in a)
    assert getattr(generic["train"], "_mfas_feature_loader", None) is not None      # drained once, then cached
    with pytest.raises(TypeError):      # raw video cannot be served: no backbones in this engine
        M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net,
                               {"train": [{"rgb": torch.zeros(2, 3, 8, 32, 32), "ske": torch.zeros(2, 3, 8, 25, 2), "label": torch.zeros(2)}],
                                "dev": fast["dev"]}, args, dev)


@pytest.mark.parametrize("R,B,bn,drpt", [(16, 20, False, 0.5), (16, 16, True, 0.3), (128, 16, True, 0.5), (64, 11, True, 0.0)])
def test_train_mode_forward_vs_oracle(dev, R, B, bn, drpt):
    """mfas_population_forward_train == Searchable_Skeleton_Image_Net.forward under model.train(True)
    (ntu_searchable.py:206-247): batch-statistics BN with running-stat update, dropout (the oracle shares the engine's
    counter-based stream), logits of one batch; the module surface returns the same and bumps num_batches_tracked."""
    import mfas_amd as M
    from tests.helpers import engine_hyper, rel_err
    ohp = O.Hyper(R=R, B=B, bn=bn, drpt=drpt)
    conf = np.array(CONFS["c4"])
    t = O.synth_table(B, 91, snr=0.4)
    tab = M.FeatureTable.from_numpy(t, dev, torch.float32)
    params = O.init_params(conf, ohp, 17, perturb_bn=True)
    pop = M.Population(engine_hyper(ohp), [conf], dev, drop_seeds=[77])
    pop.set_state_dict(0, params)
    got = pop.forward_train(0, tab, 0, B, step=5).cpu().numpy()
    feats = {k: v for k, v in t.items() if k != "label"}
    want, cache = O.forward({k: v.copy() for k, v in params.items()}, conf, ohp, feats, True, seed=77, step=5)
    assert rel_err(got, want) < 3e-4, rel_err(got, want)
    if bn:      # the running statistics moved exactly like a train step's
        p2 = {k: v.copy() for k, v in params.items()}
        O.bn_update_running(p2, ohp, cache)
        sd = pop.get_state_dict(0)
        for i in range(4):
            for nm in ("running_mean", "running_var"):
                np.testing.assert_allclose(sd[f"fusion_layers.{i}.2.{nm}"].numpy(), p2[f"fusion_layers.{i}.2.{nm}"], rtol=2e-4, atol=1e-6)
    # eval-mode forward of the same rows differs (dropout / batch statistics) unless there is neither
    ev = pop.forward(0, tab).cpu().numpy()
    assert (rel_err(ev, want) > 1e-3) or (not bn and drpt == 0.0)
    pop.close()
    # module surface: train() -> train-mode forward on the engine, eval() -> eval-mode forward
    args = mkargs(inner_representation_size=R, batchnorm=bn, drpt=drpt, batchsize=B)
    model = M.Searchable_Skeleton_Image_Net(args, conf)
    model.train(True)
    x = {k: torch.from_numpy(v).to(dev) for k, v in feats.items()}
    rgb, ske = {k: v for k, v in x.items() if k[0] == "v"}, {k: v for k, v in x.items() if k[0] == "s"}
    out = model((rgb, ske))
    assert out.shape == (B, 60) and torch.isfinite(out).all()
    if bn:
        assert int(model.fusion_layers[0][2].num_batches_tracked) == 1
        assert not torch.allclose(model.fusion_layers[0][2].running_mean, torch.zeros(R))
    model.train(False)
    out2 = model((rgb, ske))
    assert out2.shape == (B, 60)


def test_per_candidate_sample_orders(dev):
    """args.engine_order = "per_candidate": every candidate walks its OWN per-epoch permutations, as the reference's per-candidate
    DataLoader(shuffle=True) does (models/searchable.py:248-250, train_searchable/ntu.py:35).
    (1) plumbing: K identical tables in the [K][E][N] buffer == the shared-order run, bit for bit, on the resident persistent
        schedule, launch-per-phase (R=16) and the general chain (R=128, fused groups);
    (2) arithmetic: a candidate with its own order equals the oracle's run on that order (dropout on, shared mask stream);
    (3) through train_sampled_models: results depend on the candidate's index only (not on the population it trains in), differ
        from the shared-order results, and the call-mean accuracy does not move (3 standard errors)."""
    import os
    import mfas_amd as M
    from tests.helpers import engine_hyper
    conf = np.array(CONFS["c4"])
    N, Nd, E, K = 640, 320, 2, 5
    rng = np.random.default_rng(8)
    shared = np.stack([rng.permutation(N) for _ in range(E)])
    own = np.stack([np.stack([rng.permutation(N) for _ in range(E)]) for _ in range(K)])
    for R, B, bn, mode in ((16, 20, False, None), (16, 20, False, "0"), (128, 16, True, None)):
        ohp = O.Hyper(R=R, B=B, bn=bn, drpt=0.5, epochs=E)
        ttr, tdv = O.synth_table(N, 3, snr=0.6), O.synth_table(Nd, 4, snr=0.6)
        ta, tb = M.FeatureTable.from_numpy(ttr, dev, torch.bfloat16), M.FeatureTable.from_numpy(tdv, dev, torch.bfloat16)
        ttr_q, tdv_q = O.synth_table(N, 3, snr=0.6, quant="bf16"), O.synth_table(Nd, 4, snr=0.6, quant="bf16")
        nb = -(-N // B)
        etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N / B, E * nb)

        def run(per_cand, order):
            hp = engine_hyper(ohp)
            hp.order_per_candidate, hp.tap_bits = per_cand, 16
            if mode is not None:
                os.environ["MFAS_PERSIST"] = mode
            try:
                pop = M.Population(hp, [conf] * K, dev, drop_seeds=list(range(30, 30 + K)))
            finally:
                os.environ.pop("MFAS_PERSIST", None)
            pop.init(list(range(1, K + 1)))
            stats, status = pop.train(ta, tb, E, etas, order=torch.from_numpy(order.astype(np.int32)))
            planes = [pop.get_params(k, 0).cpu().numpy() for k in range(K)]
            pop.close()
            assert not status.any()
            return stats, planes

        s0, p0 = run(False, shared)
        s1, p1 = run(True, np.stack([shared] * K))
        assert s0.tobytes() == s1.tobytes(), (R, mode)                                  # (1)
        assert all(np.array_equal(a, b) for a, b in zip(p0, p1))
        s2, _ = run(True, own)
        assert s2.tobytes() != s0.tobytes()
        for k in (0, K - 1):                                                           # (2)
            hist = []
            O.train_candidate(conf, ohp, O.init_params(conf, ohp, 1 + k), ttr_q, tdv_q, order=own[k], seed=30 + k, history=hist)
            for e in range(E):
                # (R=128 with BN + dropout is chaotic within tens of steps — tests/test_gpu_parity.py::check_one_step_map — so its epoch
                #  loss gets 1.5 %; the R=16 cases pin the order plumbing at 0.3 %: another order moves an epoch loss by several %)
                tol = 1.5e-2 if R == 128 else 3e-3
                assert abs(s2["train_loss_sum"][k, e] / N - hist[e]["train_loss"]) < tol * max(1.0, hist[e]["train_loss"]), (R, k, e)
                assert abs(int(s2["dev_corrects"][k, e]) - hist[e]["dev_corrects"]) <= (8 if R == 128 else 3), (R, k, e)
    # (3) the driver
    tr = M.FeatureTable.synthetic(1280, 1, dev, torch.bfloat16, snr=0.5)
    dv = M.FeatureTable.synthetic(1280, 2, dev, torch.bfloat16, snr=0.5)
    ld = {"train": M.FeatureLoader(tr, 20, shuffle=True), "dev": M.FeatureLoader(dv, 20, shuffle=False)}
    confs = [conf] * 48
    res = {}
    for order_mode in ("shared", "per_candidate"):
        args = mkargs(inner_representation_size=16, batchnorm=False, drpt=0.5, batchsize=20, epochs=3, engine_init="device",
                      engine_order=order_mode)
        torch.manual_seed(7)
        res[order_mode] = np.array(M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev))
        if order_mode == "per_candidate":
            torch.manual_seed(7)
            sub = np.array(M.train_sampled_models(confs[:6], M.Searchable_Skeleton_Image_Net, ld, args, dev))
            assert np.array_equal(sub, res[order_mode][:6])          # candidate i's order does not depend on the population
    a, b = res["shared"], res["per_candidate"]
    assert not np.array_equal(a, b)
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    assert abs(a.mean() - b.mean()) <= 3.0 * se + 1e-3, (a.mean(), b.mean(), se)


@pytest.mark.parametrize("R,B,bn,drpt,alphas,cname", [(16, 20, False, 0.5, False, "c4"), (16, 16, True, 0.4, True, "l3"),
                                                      (128, 16, True, 0.5, False, "c4"), (64, 11, True, 0.0, False, "l2")])
def test_train_mode_forward_is_differentiable(dev, R, B, bn, drpt, alphas, cname):
    """Searchable_Skeleton_Image_Net.forward under model.train(True) is differentiable in the reference
    (ntu_searchable.py:206-247): a caller may write its own loop — loss = f(model(batch)); loss.backward(); optimizer.step().
    Here the logits carry an autograd edge whose backward is the engine's fused backward run from the caller's dL/dlogits
    (mfas_population_backward).  (1) C ABI: gradients of an ARBITRARY dlogits equal the oracle's backward, parameters untouched;
    (2) module surface: loss.backward() fills .grad of every central parameter like torch's own autograd does on the oracle-pinned
    restatement of the network, and one torch.optim.Adam step moves the parameters."""
    import mfas_amd as M
    from tests.helpers import engine_hyper
    conf = np.array(CONFS[cname])
    ohp = O.Hyper(R=R, B=B, bn=bn, drpt=drpt, alphas=alphas)
    t = O.synth_table(B, 91, snr=0.4)
    tab = M.FeatureTable.from_numpy(t, dev, torch.float32)
    params = O.init_params(conf, ohp, 17, perturb_bn=True)
    rng = np.random.default_rng(5)
    dlog = (rng.standard_normal((B, 60)) * 0.1).astype(np.float32)          # not a softmax gradient: an arbitrary upstream gradient
    # (1) the C ABI
    pop = M.Population(engine_hyper(ohp), [conf], dev, drop_seeds=[77])
    pop.set_state_dict(0, params)
    before = pop.get_params(0).clone()
    gflat = pop.backward(0, tab, torch.from_numpy(dlog).to(dev), 0, B, step=3)
    assert torch.equal(pop.get_state_dict(0)["central_classifier.weight"], torch.from_numpy(params["central_classifier.weight"]))
    feats = {k: v for k, v in t.items() if k != "label"}
    _, cache = O.forward({k: v.copy() for k, v in params.items()}, conf, ohp, feats, True, seed=77, step=3)
    want = O.backward(params, ohp, cache, dlog)
    layout, _ = M.engine.flat_layout(conf, engine_hyper(ohp))
    seen = 0
    for key, shape, off in layout:
        if key not in want:
            continue
        got = gflat[off:off + int(np.prod(shape))].reshape(shape).cpu().numpy()
        sc = float(np.abs(want[key]).max()) + 1e-30
        assert np.abs(got - want[key]).max() <= 2e-4 * sc + 1e-8, (key, np.abs(got - want[key]).max(), sc)
        seen += 1
    assert seen == len(want) >= 2 * len(conf) + 2
    w_after = pop.get_params(0)
    keep = torch.ones_like(before, dtype=torch.bool)
    for key, shape, off in layout:
        if "running" in key:                                                 # (train-mode BN moves its running statistics)
            keep[off:off + int(np.prod(shape))] = False
    assert torch.equal(w_after[keep], before[keep])                          # the parameters are untouched
    pop.close()
    # (2) the module surface
    args = mkargs(inner_representation_size=R, batchnorm=bn, drpt=drpt, batchsize=B, alphas=alphas)
    model = M.Searchable_Skeleton_Image_Net(args, conf)
    sd = model.state_dict()
    for k, v in params.items():
        sd[k].copy_(torch.from_numpy(v))
    model.train(True)
    x = {k: torch.from_numpy(v).to(dev) for k, v in feats.items()}
    rgb, ske = {k: v for k, v in x.items() if k[0] == "v"}, {k: v for k, v in x.items() if k[0] == "s"}
    opt = torch.optim.Adam(model.central_params(), lr=1e-3, weight_decay=1e-4)
    torch.manual_seed(123)
    out = model((rgb, ske))
    assert out.requires_grad and out.shape == (B, 60)
    label = torch.from_numpy(t["label"]).to(dev)
    loss = torch.nn.functional.cross_entropy(out, label) + 0.01 * (out ** 2).mean()      # the caller's own loss
    loss.backward()
    # oracle with the same mask stream: the module drew its dropout seed from torch's RNG right after manual_seed(123)
    torch.manual_seed(123)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) & 0xFFFFFFFF
    logits, cache = O.forward({k: v.copy() for k, v in params.items()}, conf, ohp, feats, True, seed=seed, step=0)
    lt = torch.from_numpy(logits).requires_grad_(True)
    (torch.nn.functional.cross_entropy(lt, torch.from_numpy(t["label"])) + 0.01 * (lt ** 2).mean()).backward()
    want = O.backward(params, ohp, cache, lt.grad.numpy())
    named = dict(model.named_parameters())
    for key, w in want.items():
        g = named[key].grad
        assert g is not None, key
        sc = float(np.abs(w).max()) + 1e-30
        assert np.abs(g.cpu().numpy() - w).max() <= 3e-4 * sc + 1e-8, (key, np.abs(g.cpu().numpy() - w).max(), sc)
    if not alphas:
        assert all(p.grad is None for k, p in named.items() if k.startswith("alphas"))       # ntu_searchable.py:251
    w0 = named["fusion_layers.0.0.weight"].detach().clone()
    opt.step()
    assert not torch.equal(named["fusion_layers.0.0.weight"].detach(), w0)


def test_gpu_surrogate_reproduces_the_pinned_controller_decisions(dev):
    """--surrogate_device gpu (graph-replayed train steps, device GEMM arithmetic) takes the SAME decisions as the CPU path — and as
    the unchanged reference controller — on the reference-pinned runs of golden G9 (every sampled configuration of every call,
    the best accuracies kept).  (At the search script's defaults — 50 surrogate epochs, hundreds of Adam steps — the two decision
    streams part ways after ~900-1,700 decisions, tools/gpu_surrogate_decisions.py / profiles/r03_gpu_surrogate_decisions.log,
    while the CPU path is invariant to its thread count: the device surrogate therefore stays opt-in.)"""
    import random
    import mfas_amd as M
    from mfas_amd.search import ModelSearcher, SimpleRecurrentSurrogate
    g = golden("g9_controller_run.npz")
    for tag, iters, levels, K in (("a", 2, 3, 5), ("b", 3, 4, 6)):
        args = SimpleNamespace(search_iterations=iters, max_progression_levels=levels, num_samples=K,
                               initial_temperature=10.0, final_temperature=0.2, temperature_decay=4.0,
                               lr_surrogate=0.001, epochs_surrogate=8, verbose=False)
        calls = []

        def fake_train(confs, model_type, dataloaders, a, device, state_dict=None):
            calls.append([np.array(c) for c in confs])
            return [O.fake_accuracy(c) for c in confs]

        np.random.seed(3)
        torch.manual_seed(3)
        random.seed(3)
        surrogate = SimpleRecurrentSurrogate(100, 3, 100).to(dev)
        s_data = ModelSearcher(args)._epnas(None, {"model": surrogate, "criterion": torch.nn.MSELoss()}, None,
                                            {"train_sampled_fun": fake_train,
                                             "get_layer_confs": M.get_possible_layer_configurations}, dev)
        flat = np.concatenate([np.concatenate([np.asarray(c).reshape(-1), [-1]]) for call in calls for c in call])
        assert np.array_equal(flat, g[tag + "/calls_flat"]), tag
        _, accs, _ = s_data.get_k_best(5)
        np.testing.assert_allclose(np.sort(np.array(accs)), g[tag + "/best_accs"], rtol=1e-12)


def test_plan_query_equals_the_created_layout(dev):
    """mfas_population_plan (pure query: nothing allocated) answers what mfas_population_create then does — schedule, resident units,
    their workgroups and units per workgroup — for search-sized and bench-sized populations, homogeneous and mixed, with a forced
    chunk and with the persistent schedule forbidden."""
    import os
    import mfas_amd as M
    rng = np.random.default_rng(2)
    cases = []
    for R, B, bn in ((16, 20, False), (16, 16, True), (128, 16, True), (32, 20, False)):
        for K in (1, 6, 9, 16, 24, 28, 29, 40, 50):
            for mixed in (False, True):
                cases.append((R, B, bn, K, mixed, 0))
    cases += [(16, 20, False, 7, False, 512), (16, 20, False, 16, True, 1024), (16, 20, False, 30, False, 256)]
    seen_res = seen_lpp = 0
    for R, B, bn, K, mixed, cc in cases:
        hp = M.Hyper(R=R, C=60, B=B, bn=bn, drpt=0.5, tap_bits=16)
        confs = [np.array(CONFS["c4"])] * K
        if mixed:
            confs = [np.stack([rng.integers(0, 4, L), rng.integers(0, 4, L), rng.integers(0, 2, L)], 1) for L in rng.integers(1, 5, K)]
        plan = M.engine.plan_population(hp, confs, dev, cc)
        pop = M.Population(hp, confs, dev, chunk_cols=cc)
        sched = pop.schedule()
        pop.close()
        assert bool(plan["persistent"]) == bool(sched["persistent"]), (R, B, K, mixed, cc, plan, sched)
        if sched["persistent"]:
            for key in ("resident_units", "resident_workgroups", "units_per_workgroup"):
                assert plan[key] == sched[key], (key, R, B, K, mixed, cc, plan, sched)
            seen_res += 1
        else:
            seen_lpp += 1
    assert seen_res >= 20 and seen_lpp >= 20
    os.environ["MFAS_PERSIST"] = "0"
    try:
        hp = M.Hyper(R=16, C=60, B=20, bn=False, drpt=0.5, tap_bits=16)
        assert not M.engine.plan_population(hp, [np.array(CONFS["c4"])] * 6, dev)["persistent"]
    finally:
        del os.environ["MFAS_PERSIST"]


def test_search_cli_two_ranks_matches_single(dev):
    """main_searchable_ntu.py end to end under 2 processes (gloo, both on cuda:0): every rank runs the seeded controller, the
    population of every call is sharded, accuracies are all-gathered — the search result equals the single-process run."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "main_searchable_ntu.py"), "--synthetic", "600", "300", "--num_samples", "6",
           "--search_iterations", "2", "--max_fusions", "2", "--epochs", "1", "--epochs_surrogate", "5", "--no-verbose",
           "--dist_backend", "gloo", "--seed", "3", "--batchsize", "20"]

    def run(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29591", WORLD_SIZE=str(world))
        procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
                 for r in range(world)]
        outs = []
        for p in procs:
            out, _ = p.communicate(timeout=900)
            assert p.returncode == 0, out.decode()[-3000:]
            outs.append(out.decode())
        text = outs[0]
        listing = text[text.index("Now listing best architectures"):]
        return [l for l in listing.splitlines()[1:] if l.startswith("[[")]

    one, two = run(1), run(2)
    assert len(one) == 5 and one == two, (one, two)


def test_large_share_trains_in_two_resident_rounds(dev, monkeypatch):
    """A share too large for the persistent resident schedule whose halves fit is trained as two populations one after the other
    (ntu_searchable._plan_rounds): same accuracies, candidate by candidate, as the single launch-per-phase population on the
    same column chunks (candidates are independent; every schedule of the same units is bit-identical)."""
    import mfas_amd as M
    from mfas_amd import ntu_searchable as NS
    monkeypatch.setenv("MFAS_NO_TAP_MAJOR", "1")       # per-segment units in both schedules
    rng = np.random.default_rng(3)
    confs = [np.stack([rng.integers(0, 4, 4), rng.integers(0, 4, 4), rng.integers(0, 2, 4)], 1) for _ in range(30)]
    ttr, tdv = O.synth_table(400, 41, snr=0.5), O.synth_table(200, 42, snr=0.5)
    ld = loaders(ttr, tdv, dev, 20, dtype=torch.bfloat16)
    args = mkargs(batchsize=20, epochs=2, engine_init="device", engine_chunk_cols=256, engine_profile=True)

    def run():
        NS.PROFILE.clear()
        torch.manual_seed(11)
        acc = M.train_sampled_models(confs, M.Searchable_Skeleton_Image_Net, ld, args, dev)
        return acc, [p[3] for p in NS.PROFILE]

    monkeypatch.setenv("MFAS_NO_ROUNDS", "1")
    one, sched_one = run()
    monkeypatch.delenv("MFAS_NO_ROUNDS")
    two, sched_two = run()
    assert len(sched_one) == 1 and not sched_one[0]["persistent"] and sched_one[0]["candidates"] == 30
    assert len(sched_two) == 2 and all(s["persistent"] and s["resident_units"] > 0 for s in sched_two)
    assert sum(s["candidates"] for s in sched_two) == 30 and sched_two[0]["candidates"] >= 15      # first round filled to capacity
    assert one == two


def test_graphed_surrogate_trainer_matches_cpu_eager(dev):
    """--surrogate_device gpu: the surrogate's train steps replayed as HIP graphs (padded buckets + mask, LSTM cell written out,
    capturable Adam) follow the CPU eager loop of the reference semantics: same parameters after ONE step (so the warm-up the capture
    needs left no trace and the masked loss is MSELoss), same predictions to 1e-3 after 30 epochs over two buckets."""
    import copy
    import torch.optim as op
    from mfas_amd.search import surrogate as S
    rng = np.random.default_rng(5)
    data = ([torch.from_numpy(rng.integers(0, 4, (L, n, 3)).astype(np.float32)) for L, n in ((2, 40), (4, 30))],
            [torch.from_numpy(rng.random((n, 1)).astype(np.float32)) for n in (40, 30)])
    torch.manual_seed(3)
    cpu = S.SimpleRecurrentSurrogate(100, 3, 100)
    gpu = copy.deepcopy(cpu).to(dev)
    # the written-out cell is nn.LSTM's arithmetic
    x = data[0][1]
    torch.testing.assert_close(cpu.forward_unrolled(x), cpu(x), rtol=1e-5, atol=1e-6)
    crit = torch.nn.MSELoss()
    o_cpu = op.Adam(cpu.parameters(), lr=1e-3)
    o_gpu = op.Adam(gpu.parameters(), lr=1e-3, capturable=True, foreach=True)
    l_cpu = S.train_simple_surrogate(cpu, crit, o_cpu, ([data[0][0]], [data[1][0]]), 1, "cpu")
    l_gpu = S.train_simple_surrogate(gpu, crit, o_gpu, ([data[0][0]], [data[1][0]]), 1, dev)
    assert abs(l_cpu - l_gpu) < 1e-5
    for (k, a), (_, b) in zip(cpu.named_parameters(), gpu.named_parameters()):
        torch.testing.assert_close(b.detach().cpu(), a.detach(), rtol=0, atol=2e-5, msg=k)     # one Adam step = lr * sign-like update
    assert int(o_gpu.state[next(iter(gpu.parameters()))]["step"].item()) == 1                    # the warm-up steps were undone
    gpu._graphed_trainer.cap = 32          # smaller than the 40-row bucket: the trainer must grow its buffers and capture again
    gpu._graphed_trainer.graphs.clear()
    S.train_simple_surrogate(cpu, crit, o_cpu, data, 30, "cpu")
    S.train_simple_surrogate(gpu, crit, o_gpu, data, 30, dev)
    assert gpu._graphed_trainer.cap == 64
    with torch.no_grad():
        for xx in data[0]:
            torch.testing.assert_close(gpu(xx.to(dev)).cpu(), cpu(xx), rtol=0, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("R,bn,alphas,K,mixed,dt", [(16, False, False, 6, False, "bf16"), (16, True, False, 9, True, "f16"), (32, False, True, 7, True, "bf16"),
                                                    (16, True, True, 5, False, "bf16"), (32, True, False, 4, True, "f32")])
def test_small_r_eval_mapping_is_bit_identical(dev, R, bn, alphas, K, mixed, dt):
    """R <= 32 (one or two row blocks): the dev pass splits the m-blocks of a 64-row tile over the four waves and stages 16-bit table
    rows through registers, one chunk ahead (eval.hip.h).  Same products in the same order per logit as the plain mapping
    (MFAS_EVAL_NO_MSPLIT=1: one wave per row block, rows staged at the barrier), so every statistic of a training call — dev
    corrects AND dev loss — must be bit-identical.  Dev sizes with a ragged last row block, mixed depths / taps, batchnorm, alphas
    (including a sigma(alpha) == 1 cell: the V modality is skipped), bf16 / f16 / f32 tables."""
    import os
    import torch
    import mfas_amd as M
    rng = np.random.default_rng(11)
    N, Nd, E, B = 400, 1000 + 37, 2, 20
    hp = M.Hyper(R=R, C=60, B=B, bn=bn, drpt=0.5, alphas=alphas, tap_bits=16 if dt != "f32" else 32)
    confs = [np.array(CONFS["c4"])] * K
    if mixed:
        confs = [np.stack([rng.integers(0, 4, L), rng.integers(0, 4, L), rng.integers(0, 2, L)], 1) for L in rng.integers(1, 5, K)]
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[dt]
    ta = M.FeatureTable.from_numpy(O.synth_table(N, 3, snr=0.6), dev, tdt)
    tb = M.FeatureTable.from_numpy(O.synth_table(Nd, 4, snr=0.6), dev, tdt)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N / B, E * (-(-N // B)))
    order = M.ntu_searchable.make_order(N, E, True, 5, dev)

    def run(plain):
        if plain:
            os.environ["MFAS_EVAL_NO_MSPLIT"] = "1"
        try:
            pop = M.Population(hp, confs, dev, drop_seeds=list(range(40, 40 + K)))
            pop.init(list(range(1, K + 1)))
            if alphas:      # one cell with sigma(alpha) == 1 exactly
                flat = pop.get_params(0, 0)
                flat[0] = 30.0
                pop.set_params(0, flat)
            stats, status = pop.train(ta, tb, E, etas, order=order)
            pop.close()
        finally:
            os.environ.pop("MFAS_EVAL_NO_MSPLIT", None)
        assert not status.any()
        return stats

    s_new, s_old = run(False), run(True)
    assert s_new.tobytes() == s_old.tobytes()
    assert (s_old["dev_corrects"] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("R,bn,alphas,K,mixed,widths", [(128, True, False, 5, False, None), (96, False, True, 6, True, None),
                                                        (128, True, True, 4, True, (64, 208, 96, 1024)), (72, True, False, 3, True, (160, 64, 512, 80))])
def test_bf16x3_eval_products_match_f32_products(dev, R, bn, alphas, K, mixed, widths):
    """R = 72 .. 128 over bf16 tables: the dev pass runs the feature products as three bf16 MFMAs per 32 columns (every f32 weight =
    hi + mid + lo bf16 terms, exactly; the rows are bf16 as stored) instead of f32 MFMAs (eval.hip.h, B3).  Every product is exact
    either way and only the f32 summation order differs, so against the f32-product build of the same kernel (MFAS_EVAL_NO_B3=1):
    logits agree to f32 round-off of a 1,000-term sum, the dev loss sums to 1e-6 relative, and the dev corrects may differ only
    through a last-bit tie (<= 1 row per candidate and epoch).  Ragged dev size, mixed depths and taps, widths that leave an odd
    last k-block / a partial last 128-column chunk, alphas incl. a sigma(alpha) == 1 cell, the eval-mode forward of the C ABI."""
    import os
    import torch
    import mfas_amd as M
    rng = np.random.default_rng(13)
    N, Nd, E, B = 320, 700 + 29, 2, 16
    kw = {} if widths is None else {"s_sizes": widths, "v_sizes": widths[::-1]}
    hp = M.Hyper(R=R, C=60, B=B, bn=bn, drpt=0.5, alphas=alphas, tap_bits=16, **kw)
    confs = [np.array(CONFS["c4"])] * K
    if mixed:
        confs = [np.stack([rng.integers(0, 4, L), rng.integers(0, 4, L), rng.integers(0, 2, L)], 1) for L in rng.integers(1, 5, K)]
    okw = {} if widths is None else {"s_sizes": widths, "v_sizes": widths[::-1]}
    ta = M.FeatureTable.from_numpy(O.synth_table(N, 3, snr=0.6, **okw), dev, torch.bfloat16)
    tb = M.FeatureTable.from_numpy(O.synth_table(Nd, 4, snr=0.6, **okw), dev, torch.bfloat16)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N / B, E * (-(-N // B)))
    order = M.ntu_searchable.make_order(N, E, True, 5, dev)

    def run(f32_products):
        if f32_products:
            os.environ["MFAS_EVAL_NO_B3"] = "1"
        try:
            pop = M.Population(hp, confs, dev, drop_seeds=list(range(40, 40 + K)))
            pop.init(list(range(1, K + 1)))
            if alphas:      # one cell with sigma(alpha) == 1 exactly
                flat = pop.get_params(0, 0)
                flat[0] = 30.0
                pop.set_params(0, flat)
            stats, status = pop.train(ta, tb, E, etas, order=order)
            logits = [pop.forward(k, tb, row0=3, nrows=Nd - 5).cpu().numpy() for k in range(K)]
            params = [{key: v.numpy() for key, v in pop.get_state_dict(k).items()} for k in range(K)]
            pop.close()
        finally:
            os.environ.pop("MFAS_EVAL_NO_B3", None)
        assert not status.any()
        return stats, logits, params

    (s_new, l_new, p_new), (s_old, l_old, _) = run(False), run(True)
    assert s_new["train_loss_sum"].tobytes() == s_old["train_loss_sum"].tobytes()      # training does not depend on the dev pass
    assert np.abs(s_new["dev_corrects"] - s_old["dev_corrects"]).max() <= 1
    np.testing.assert_allclose(s_new["dev_loss_sum"], s_old["dev_loss_sum"], rtol=1e-6)
    for a, b in zip(l_new, l_old):
        assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(b).max())
    # both builds against the float64 reference on the trained parameters, elementwise (tests/ref64.py): a B3 build that lost the
    # low weight bits would still pass the max-scaled bound above
    from tests import ref64 as R64
    from tests.ref64_cases import TAU_LOGITS
    dv = O.synth_table(Nd, 4, snr=0.6, **okw)
    feats = {key: O.bf16_round(v)[3:Nd - 2] for key, v in dv.items() if key[0] in "sv"}
    for k in range(K):
        want, Mw, _ = R64.forward(p_new[k], confs[k], hp, feats, False)
        R64.assert_close64(l_new[k], want, Mw, TAU_LOGITS, f"B3 build R{R} cand {k}")
        R64.assert_close64(l_old[k], want, Mw, TAU_LOGITS, f"f32-product build R{R} cand {k}")
    assert (s_old["dev_corrects"] > 0).any()
