"""The population driver behind every entry point: loader draining, sample orders, initial parameters, resident rounds, sharding glue,
successive halving, weight sharing and the population of one of the single-model trainers.  ``train_sampled_models`` is the drop-in for
/root/reference/models/search/ntu_searchable.py:23-102, ``get_central_states`` / ``set_central_states`` mirror :123-174.
mfas_amd.ntu_searchable (the nn.Module mirror) re-exports these names; this module does not import it."""
from __future__ import annotations

import math
import os
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from typing import List

import numpy as np
import torch
import torch.nn as nn

from . import population as popmod
from .engine import (EPOCH_STATS_DTYPE, FeatureLoader, FeatureTable, Hyper, Population, best_dev_accuracy, best_dev_f1,
                     cell_in_features, flat_layout)
from .scheduler import LRCosineAnnealingScheduler


# ------------------------------------------------------------------------------------------------ weight sharing
def _share_name(idx_layer, layer, conf_row):
    name = str(idx_layer) + ".L_" + str(layer[0].in_features) + "_" + str(layer[0].out_features)
    return name + {0: ".A_relu", 1: ".A_sigmoid", 2: ".A_lrelu"}[int(conf_row[2])]


def get_central_states(model, state_dict, using_dataparallel=False):
    """ntu_searchable.py:123-149: publish every cell under ``"{idx}.L_{in}_{out}.A_{act}"``."""
    model = model.module if using_dataparallel else model
    for idx_layer, layer in enumerate(model.fusion_layers):
        state_dict[_share_name(idx_layer, layer, model.conf[idx_layer])] = \
            {k: v.detach().clone() for k, v in layer.state_dict().items()}
    return state_dict


def set_central_states(model, state_dict, using_dataparallel=False):
    """ntu_searchable.py:152-174: load every cell whose key exists."""
    model = model.module if using_dataparallel else model
    for idx_layer, layer in enumerate(model.fusion_layers):
        name = _share_name(idx_layer, layer, model.conf[idx_layer])
        if name in state_dict:
            layer.load_state_dict(state_dict[name])


# ------------------------------------------------------------------------------------------------ the driver
PROFILE: List[tuple] = []   # (launches, total ms, algorithmic bytes/launch) of k_sweep per call when args.engine_profile
RUNG_CHANGES: List[tuple] = []   # (candidates before, survivors, seconds) of every rung change of engine_halving calls when args.engine_profile


def _require_loader(x, name, device=None) -> FeatureLoader:
    """SURVEY §8(b) dataloaders contract.  Fast path: a FeatureLoader over a HIP-resident table.  Otherwise any iterable
    of reference-shaped batches ``{'rgb': {v0..v3[, vlogit]}, 'ske': {s0..s3[, slogit]}, 'label'}`` whose taps are
    already pooled to (B, width) (train_searchable/ntu.py:35-43 reads exactly these keys): it is drained ONCE into a
    device-resident FeatureTable (cached on the loader object) and from then on only its batch size and shuffle flag
    matter.  Raw video / skeleton tensors are rejected: there are no backbones here."""
    if isinstance(x, FeatureLoader):
        return x
    cached = getattr(x, "_mfas_feature_loader", None)
    if cached is not None:
        return cached
    if device is None or not hasattr(x, "__iter__"):
        raise TypeError(f"dataloaders['{name}'] must be a mfas_amd.FeatureLoader over a HIP-resident FeatureTable (or an "
                        "iterable of pooled-tap batches); there is no raw-video / CPU path")
    taps, labels, extra = {}, [], {}
    bsz = 0
    for batch in x:
        rgb, ske = batch["rgb"], batch["ske"]
        if not hasattr(rgb, "items") or not hasattr(ske, "items"):
            raise TypeError(f"dataloaders['{name}']: 'rgb' / 'ske' must map tap names (v0.., s0..) to pooled (B, width) "
                            "tensors; raw video needs the frozen backbones, which are outside this engine")
        for src in (rgb, ske):
            for k, v in src.items():
                if v is None:
                    continue
                v = torch.as_tensor(v)
                if k in ("vlogit", "slogit"):
                    extra.setdefault(k, []).append(v.reshape(v.shape[0], -1).float())
                elif len(k) >= 2 and k[0] in "sv" and k[1:].isdigit():
                    if v.dim() > 2:          # GlobalPooling2D (aux_models.py:58-64) for un-pooled maps: the k_pool kernel
                        from .pooling import global_pool
                        v = global_pool(v.to(torch.device(device)), torch.float32)
                    taps.setdefault(k, []).append(v)
        lab = torch.as_tensor(batch["label"]).reshape(-1)
        labels.append(lab)
        bsz = max(bsz, int(lab.numel()))
    if not labels:
        raise ValueError(f"dataloaders['{name}'] yielded no batches")
    dev = torch.device(device)
    table = FeatureTable({k: torch.cat(v).to(dev) for k, v in taps.items()},
                         torch.cat(labels).to(dev).to(torch.int32),
                         vlogit=torch.cat(extra["vlogit"]).to(dev) if "vlogit" in extra else None,
                         slogit=torch.cat(extra["slogit"]).to(dev) if "slogit" in extra else None)
    sampler = getattr(x, "sampler", None)
    shuffle = sampler is not None and type(sampler).__name__ == "RandomSampler"
    fl = FeatureLoader(table, int(getattr(x, "batch_size", None) or bsz), shuffle=shuffle)
    try:
        x._mfas_feature_loader = fl
    except Exception:
        pass
    return fl


def make_order(N, epochs, shuffle, seed, device):
    """Per-epoch sample order shared by the population (DataLoader(shuffle=True), models/searchable.py:248)."""
    if not shuffle:
        return None
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    return torch.stack([torch.randperm(N, generator=gen, device=device) for _ in range(epochs)]).to(torch.int32)


def _mix64(z):
    """splitmix64's finaliser on int64 tensors (wrapping multiplies; logical right shifts written as arithmetic shift + mask)."""
    z = (z ^ ((z >> 30) & 0x3FFFFFFFF)) * -4658895280553007687          # 0xBF58476D1CE4E5B9
    z = (z ^ ((z >> 27) & 0x1FFFFFFFFF)) * -7723592293110705685         # 0x94D049BB133111EB
    return z ^ ((z >> 31) & 0x1FFFFFFFF)


def make_order_per_candidate(N, epochs, shuffle, seed, device, indices):
    """args.engine_order = "per_candidate" (the default): the reference's behaviour — every candidate iterates its OWN freshly
    shuffled DataLoader each epoch (models/searchable.py:248-250, train_searchable/ntu.py:35).  Candidate i's permutations are a
    function of (seed, i, epoch) only, so they do not depend on the world size or on which round / rank trains it: every sample
    position gets a 64-bit counter-based key (seed, candidate, epoch, position -> splitmix64) and the permutation is the argsort of
    the keys — ONE batched device sort for the whole share instead of K x E randperm calls (a tie between two of N 64-bit keys has
    probability N^2 / 2^65).  Returns int32 [len(indices)][E][N]."""
    if not shuffle:
        return None
    ep = torch.arange(epochs, dtype=torch.int64, device=device).view(1, -1, 1)
    pos = torch.arange(N, dtype=torch.int64, device=device).view(1, 1, -1)
    s64 = int(seed) & 0x7FFFFFFFFFFFFFFF
    idx = [int(i) for i in indices]
    out = torch.empty((len(idx), epochs, N), dtype=torch.int32, device=device)
    per = max(1, (32 << 20) // max(1, epochs * N))          # <= 32 M keys (256 MB of int64 + the sort's buffers) per slice
    for k0 in range(0, len(idx), per):
        cand = torch.as_tensor(idx[k0:k0 + per], dtype=torch.int64, device=device).view(-1, 1, 1)
        stream = _mix64((cand + 1) * 0x632BE59BD9B4E019 + (ep + 1) * 0x2545F4914F6CDD1D + s64)   # one stream per (seed, candidate, epoch)
        keys = _mix64(stream + pos * -7046029254386353131)                                        # 0x9E3779B97F4A7C15
        out[k0:k0 + per] = torch.argsort(keys, dim=-1)
    return out


_KGAIN = math.sqrt(2.0 / (1 + math.sqrt(5) ** 2))      # init.calculate_gain('leaky_relu', sqrt(5)), as nn.Linear.reset_parameters


def linear_init_bounds(fan_in):
    """(weight bound, bias bound) of the Tensor.uniform_(-bound, bound) draws of nn.Linear.reset_parameters — kaiming_uniform_(a = sqrt 5)
    and 1 / sqrt(fan_in) — in torch's own expressions, evaluated in Python doubles."""
    return math.sqrt(3.0) * (_KGAIN / math.sqrt(fan_in)), 1.0 / math.sqrt(fan_in)


def initial_flat_params(args, conf, hp=None, generator=None, out=None) -> torch.Tensor:
    """The flat parameter vector `Searchable_Skeleton_Image_Net(args, conf).flat_params()` would hold right after
    construction — same draws from torch's global RNG in the same order (per cell Linear weight: kaiming_uniform_(a=sqrt(5)),
    bias: U(+-1/sqrt(fan_in)); the classifier likewise; then alpha_i ~ N(0, 0.1)), BatchNorm at its defaults — without
    building the ~20 module objects per candidate (train_sampled_models initialises every sampled candidate this way:
    ≈ 1 ms per candidate, a fifth of a 50-candidate call's time at R=16).  `generator`: draw from this torch.Generator instead of
    the global stream (seeded alike it yields the same numbers)."""
    conf = np.asarray(conf).reshape(-1, 3)
    hp = hp if hp is not None else Hyper.from_args(args)
    layout, n = flat_layout(conf, hp)
    where = {key: (shape, off) for key, shape, off in layout}
    if out is None:
        flat = torch.zeros(n, dtype=torch.float32)
    else:                       # fill the caller's (pinned) slice
        flat = out
        assert flat.numel() == n and flat.dtype == torch.float32
        flat.zero_()

    def view(key):
        shape, off = where[key]
        return flat[off:off + int(np.prod(shape))].view(shape)

    def linear(wkey, bkey):
        w, b = view(wkey), view(bkey)
        fan_in = w.shape[1]
        wbound, bbound = linear_init_bounds(fan_in)
        w.uniform_(-wbound, wbound, generator=generator)
        bound = bbound if fan_in > 0 else 0.0
        b.uniform_(-bound, bound, generator=generator)

    with torch.no_grad():
        for i, c in enumerate(conf):
            if int(c[2]) not in (0, 1, 2):
                raise ValueError(f"unknown non-linearity {c[2]}")
            if not (args.drpt > 1e-10 or bool(args.batchnorm)):
                raise ValueError("drpt < 1e-10 without --batchnorm is not a legal cell "
                                 "(reference: UnboundLocalError at ntu_searchable.py:284)")
            linear(f"fusion_layers.{i}.0.weight", f"fusion_layers.{i}.0.bias")
            if hp.bn:
                view(f"fusion_layers.{i}.2.weight").fill_(1.0)
                view(f"fusion_layers.{i}.2.running_var").fill_(1.0)
        linear("central_classifier.weight", "central_classifier.bias")
        for i in range(len(conf)):
            view(f"alphas.{i}.alpha_x").normal_(0.0, 0.1, generator=generator)      # nn.init.normal_
    return flat


ROUNDS_MIN_CANDIDATES = 16         # (a share that does not fit the resident schedule has at least ~29 conf-4-sized candidates, or ~50 shallow ones)


def _plan_rounds(hp, confs, mine, device, seed_base, chunk_cols):
    """The rank's share as ONE population, or as several resident rounds trained one after the other (population.split_rounds:
    the decision is the engine's own layout query, mfas_population_plan — nothing is allocated for it; only the populations
    that train are ever created).  Candidates are independent and carry their own seeds, so the split changes nothing but the
    column-chunk summation order (as any change of population size does).  Yields (indices, Population)."""
    if not mine:
        return
    for pos, planned_resident in popmod.split_rounds(hp, [confs[i] for i in mine], device, chunk_cols, ROUNDS_MIN_CANDIDATES):
        idx = [mine[j] for j in pos]
        pop = Population(hp, [confs[i] for i in idx], device, drop_seeds=[(seed_base * 7 + i) & 0xFFFFFFFF for i in idx],
                         chunk_cols=chunk_cols)
        if bool(pop.schedule()["persistent"]) != bool(planned_resident) and hp.R <= 16:
            # (MFAS_PERSIST* read at different times, or a plan / create disagreement: results are unaffected)
            warnings.warn(f"mfas_amd: the layout query planned {'a resident' if planned_resident else 'a launch-per-phase'} round of "
                          f"{len(idx)} candidates but the population was created {'resident' if not planned_resident else 'launch-per-phase'}")
        yield idx, pop


def torch_init_bounds(conf, hp) -> np.ndarray:
    """The Tensor.uniform_(-bound, bound) bounds nn.Linear.reset_parameters uses for every cell and for the classifier (weight:
    kaiming_uniform_(a = sqrt 5), bias: 1 / sqrt(fan_in)), as float32 [2 * (4 + 1)]: what mfas_population_init_torch_streams
    takes (linear_init_bounds, rounded to float32 like torch does)."""
    out = np.zeros(10, np.float32)
    conf = np.asarray(conf).reshape(-1, 3)
    for i in range(len(conf)):
        out[2 * i:2 * i + 2] = linear_init_bounds(cell_in_features(conf, i, hp))
    out[8:10] = linear_init_bounds(hp.R)
    return out


_TEST_FAIL_RANK = -1         # tests only: the rank whose first share of a sharded call raises (never read from the environment)
_DEVICE_STREAMS_OK = {}      # device -> the device-side Mersenne-Twister init reproduces torch's CPU draws on this host (checked once)


def _init_population_device_streams(pop, args, confs, group, hp, seed_base, device, searchable_type) -> bool:
    """The default initialisation, generated on the GPU: mfas_population_init_torch_streams runs torch's own generator
    (at::mt19937 + uniform_real_distribution<float>) per candidate under the seeds the host path uses.  Verified ONCE per process
    and device against torch itself — the first candidate's flat parameters must equal initial_flat_params bit for bit (torch's CPU
    kernels fuse x * (hi - lo) + lo into one fma on AVX2 / AVX512 hosts; a build that does not would differ in last bits) — and
    abandoned for the host path when that check fails (MFAS_HOST_INIT=1 forces the host path)."""
    # one check per device, class (qualified) and geometry incl. the candidate's depth: a later call with another Hyper, another L or
    # an unrelated class of the same __name__ is checked again (one module build per key)
    key = (str(device), getattr(searchable_type, "__module__", ""), getattr(searchable_type, "__qualname__", searchable_type.__name__),
           hp.R, hp.C, bool(hp.bn), bool(hp.alphas), tuple(hp.s_sizes), tuple(hp.v_sizes), len(np.asarray(confs[group[0]]).reshape(-1, 3)))
    if os.environ.get("MFAS_HOST_INIT") or _DEVICE_STREAMS_OK.get(key) is False:
        return False
    seeds = [(seed_base + 2 + i) & 0xFFFFFFFFFFFFFFFF for i in group]
    bounds = np.stack([torch_init_bounds(confs[i], hp) for i in group])
    pop.init_torch_streams(seeds, bounds)
    if key not in _DEVICE_STREAMS_OK:
        with torch.random.fork_rng(devices=[]):           # the check builds the real module ONCE per class and device
            torch.manual_seed(seed_base + 2 + group[0])
            want = searchable_type(args, confs[group[0]]).flat_params()
        ok = bool(torch.equal(pop.get_params(0).cpu(), want))
        _DEVICE_STREAMS_OK[key] = ok
        if not ok:
            warnings.warn("mfas_amd: the device-side torch random stream does not reproduce this host's torch.uniform_ draws; "
                          "initialising candidates on the host instead")
            return False
    return True


_STAGING = {}      # device -> pinned host staging buffer of the initial parameters (grow-only: a 128-candidate R=128 call needs 0.5 GB)


def _staging(device, n):
    buf = _STAGING.get(str(device))
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 1 << 20), dtype=torch.float32, pin_memory=torch.cuda.is_available())
        _STAGING[str(device)] = buf
    return buf[:n]


def _init_population_from_torch(pop, args, confs, group, hp, seed_base, searchable_type, return_model, mods, device):
    """train_sampled_models' default initialisation: every candidate starts from what constructing its module under
    torch.manual_seed(seed_base + 2 + i) draws (ntu_searchable.py:44 builds the model from torch's global stream).  Module-free
    candidates draw from a PRIVATE torch.Generator seeded the same way (same Mersenne-Twister stream, same numbers:
    tests/test_host_cpu.py), which makes the fills independent of each other: a small thread pool fills the candidates' slices of
    ONE pinned staging buffer side by side (torch's uniform_ is serial and releases the GIL; 1 M draws per R=128 candidate), one
    host-to-device copy moves the share, and the per-candidate repacking kernels (mfas_population_set_params) are queued without a
    host synchronisation in between."""
    # (the fills are tiny for torch's intra-op pool: with every host core in it their fork/join dominates — 6 ms instead of 0.7 ms
    #  per candidate on a 256-thread host; the values do not depend on the thread count)
    nthreads = torch.get_num_threads()
    if nthreads > 4:
        torch.set_num_threads(4)
    try:
        if return_model or not getattr(searchable_type, "_construction_is_standard", False):
            for j, i in enumerate(group):
                with torch.random.fork_rng(devices=[]):
                    torch.manual_seed(seed_base + 2 + i)   # world-size independent per-candidate stream
                    m = searchable_type(args, confs[i])
                if return_model:
                    mods[i] = m
                pop.set_params(j, m.flat_params())
            return
        sizes = [flat_layout(confs[i], hp)[1] for i in group]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        host = _staging(device, int(offs[-1]))

        def one(j):
            g = torch.Generator()
            g.manual_seed(seed_base + 2 + group[j])
            initial_flat_params(args, confs[group[j]], hp, generator=g, out=host[offs[j]:offs[j + 1]])

        workers = max(1, min(8, (os.cpu_count() or 1) // 2, len(group)))
        if workers == 1:
            for j in range(len(group)):
                one(j)
        else:
            with ThreadPoolExecutor(workers) as ex:
                list(ex.map(one, range(len(group))))
        dev_flat = host.to(device, non_blocking=True)
        for j in range(len(group)):
            pop.set_params(j, dev_flat[offs[j]:offs[j + 1]], sync=False)
        if torch.device(device).type == "cuda":
            torch.cuda.current_stream(device).synchronize()      # the staging buffer is free for the next call; dev_flat may go
    finally:
        if nthreads > 4:
            torch.set_num_threads(nthreads)


def init_population(pop, group, *, args, confs, hp, seed_base, device, searchable_type, premodels, return_model, mods):
    """The initial parameters of `pop`, whose slots hold confs[i] for i in `group`: copies of `premodels`; or the library's own init
    (args.engine_init == "device"); or, the default, what constructing candidate i's module under torch.manual_seed(seed_base + 2 + i)
    draws — on the device where that reproduces torch and no module is needed, else on the host.  Modules built on the way go to `mods`."""
    if premodels:
        for j, i in enumerate(group):
            src = premodels[i].module if getattr(args, "use_dataparallel", False) else premodels[i]
            m = searchable_type(args, confs[i])
            m.load_state_dict(src.state_dict())
            pop.set_params(j, m.flat_params())
            mods[i] = m
    elif getattr(args, "engine_init", "torch") == "device":
        pop.init([(seed_base + 2 + i) & 0x7FFFFFFF for i in group])
    elif (return_model or not getattr(searchable_type, "_construction_is_standard", False)
          or not _init_population_device_streams(pop, args, confs, group, hp, seed_base, device, searchable_type)):
        _init_population_from_torch(pop, args, confs, group, hp, seed_base, searchable_type, return_model, mods, device)


def _bump_bn_counters(model, steps):
    for m in model.modules():
        if isinstance(m, nn.BatchNorm1d) and m.num_batches_tracked is not None:
            m.num_batches_tracked += steps


def load_trained(model, flat, steps, device=None):
    """Leave in `model` what `steps` train steps of the engine ended with: the flat parameters (BatchNorm running statistics among
    them), num_batches_tracked moved on by the steps, eval mode (train_searchable/ntu.py:85-87)."""
    model.load_flat(flat)
    _bump_bn_counters(model, steps)
    if device is not None:
        model.to(device)
    model.train(False)


def train_one(model, hp, train_l, dev_l, epochs, etas, device, *, drop_seed, order_seed, pos_weight=None, best_threshold=None):
    """`model` trained as a population of one: `epochs` epochs from its own parameters under `etas`, dropout stream `drop_seed`, the
    per-epoch shuffles of `order_seed`; the best-epoch weights are left in the model (load_trained).  best_threshold: the dev metric
    an epoch must exceed to be kept (best_f1 = init_f1, train_searchable/mmimdb.py:18).  Returns train()'s (stats, status)."""
    pop = Population(hp, [model.conf], device, drop_seeds=[drop_seed & 0xFFFFFFFF])
    try:
        if pos_weight is not None:
            pop.set_pos_weight(pos_weight)
        pop.set_params(0, model.flat_params())
        if best_threshold is not None:
            pop.set_best_threshold(float(best_threshold))
        order = make_order(len(train_l.table), epochs, train_l.shuffle, order_seed, device)
        stats, status = pop.train(train_l.table, dev_l.table, epochs, etas, order=order, snapshot_best=True)
        load_trained(model, pop.get_params(0), epochs * -(-len(train_l.table) // hp.B))
    finally:
        pop.close()
    return stats, status


def etas_for(scheduler, optimizer, epochs, nb):
    """The per-batch learning rates of `epochs` epochs of `nb` batches: the cosine scheduler's table; any other scheduler is stepped
    once per epoch and never pushed to the optimizer (train_searchable/ntu.py:24-26), so the run sees the rate it ends on."""
    if isinstance(scheduler, LRCosineAnnealingScheduler):
        return scheduler.eta_table(epochs * nb)
    for _ in range(epochs):
        scheduler.step()
    return [optimizer.param_groups[0]["lr"]] * (epochs * nb)


def print_epoch_stats(stats_row, n_train, n_dev):
    """The two lines per epoch train_ntu_track_acc prints with verbose (train_searchable/ntu.py:76-80)."""
    for e in range(len(stats_row)):
        print("train Loss: {:.4f} Acc: {:.4f}".format(stats_row["train_loss_sum"][e] / n_train, stats_row["train_corrects"][e] / n_train))
        print("dev Loss: {:.4f} Acc: {:.4f}".format(stats_row["dev_loss_sum"][e] / n_dev, stats_row["dev_corrects"][e] / n_dev))


def tap_bits_of(train_table, dev_table):
    """Hyper.tap_bits of a run over these two tables: their element size in bits, 0 (unknown) where they differ."""
    return 8 * train_table.elem_size() if train_table.dtype == dev_table.dtype else 0


def train_sampled_models(sampled_configurations, searchable_type, dataloaders, args, device,
                         return_model=[], premodels=[], preaccuracies=[],
                         train_only_central_params=True, state_dict=dict(), _hp=None, _pos_weight=None):
    """Drop-in for ntu_searchable.py:23-102 (see _train_sampled_models); the call is one profiler range (roctx marker)."""
    from . import _lib
    with _lib.profiler_range(f"train_sampled_models K={len(sampled_configurations)}"):
        return _train_sampled_models(sampled_configurations, searchable_type, dataloaders, args, device, return_model, premodels,
                                     preaccuracies, train_only_central_params, state_dict, _hp, _pos_weight)


def _train_sampled_models(sampled_configurations, searchable_type, dataloaders, args, device,
                          return_model=[], premodels=[], preaccuracies=[],
                          train_only_central_params=True, state_dict=dict(), _hp=None, _pos_weight=None):
    """Drop-in for ntu_searchable.py:23-102.  Every configuration is trained from scratch for
    ``args.epochs`` epochs of {train over dataloaders['train'], eval over dataloaders['dev']} and its best dev
    accuracy returned, in input order.  The whole (per-rank share of the) population trains in lockstep inside
    the HIP engine; with torch.distributed initialised the population is sharded across ranks and the
    accuracies are all-gathered (RCCL).
    """
    if preaccuracies:   # the reference forwards init_f1=, which train_ntu_track_acc does not accept (:86-89)
        raise TypeError("train_ntu_track_acc() got an unexpected keyword argument 'init_f1' "
                        "(reference behaviour, ntu_searchable.py:86-89)")
    if not train_only_central_params:
        raise NotImplementedError("backbone fine-tuning needs raw video; the engine trains central_params() only")
    halving = _check_halving(args, return_model)      # args.engine_halving (None: the path below, as ever); refused before anything is created
    device = torch.device(device)
    train_l = _require_loader(dataloaders["train"], "train", device)
    dev_l = _require_loader(dataloaders["dev"], "dev", device)
    hp = _hp if _hp is not None else Hyper.from_args(args)
    hp.multitask = False    # ntu_searchable.py:82-84 never forwards multitask to the train loop
    hp.tap_bits = tap_bits_of(train_l.table, dev_l.table)
    # sample order: "per_candidate" (default) = the reference's behaviour, every candidate iterates its own freshly shuffled loader
    # (models/searchable.py:248-250, train_searchable/ntu.py:35); "shared" = one shuffle per epoch for the whole call (lockstep): what
    # lets the tap-major sweep stage a batch's rows once for several candidates at R < 128 (costs / gains per workload)
    per_cand = getattr(args, "engine_order", "per_candidate") == "per_candidate"
    if getattr(args, "engine_order", "per_candidate") not in ("shared", "per_candidate"):
        raise ValueError("args.engine_order must be 'shared' or 'per_candidate'")
    hp.order_per_candidate = per_cand
    if getattr(args, "multitask", False) and _hp is None:
        raise TypeError("max() received an invalid combination of arguments: the searchable returns a tuple "
                        "with --multitask in search mode (reference behaviour, train_searchable/ntu.py:54)")
    confs = [np.asarray(c).reshape(-1, 3) for c in sampled_configurations]
    K = len(confs)
    wanted = [i for i in range(K) if (not return_model or i in return_model)]
    N_tr, N_dev, B, E = len(train_l.table), len(dev_l.table), int(args.batchsize), int(args.epochs)
    nb = -(-N_tr // B)
    num_batches_per_epoch = N_tr / B              # float, ntu_searchable.py:30

    seed_base = popmod.broadcast_seed(int(torch.randint(0, 2 ** 31 - 1, (1,)).item()), device, confs)
    if getattr(args, "weightsharing", False):
        if hp.loss_mode != 0:
            raise NotImplementedError("weight sharing is wired for the single-label (NTU) searchable only")
        return _train_weightsharing(confs, wanted, searchable_type, train_l, dev_l, args, device, hp, seed_base,
                                    return_model, premodels, state_dict)

    rank, world = popmod.dist_info()
    wconfs = [confs[i] for i in wanted]
    owner, cap, _ = popmod.shard_call(wconfs, hp, world, device, bool(getattr(args, "engine_all_ranks", False)))
    costs = [popmod.candidate_cost(c, hp.R, hp.s_sizes, hp.v_sizes, hp.C) for c in wconfs]

    models = {}
    sched = LRCosineAnnealingScheduler(args.eta_max, args.eta_min, args.Ti, args.Tm, num_batches_per_epoch)
    etas = sched.eta_table(E * nb)
    if halving is not None:
        return _train_halving(halving, confs, searchable_type, train_l, dev_l, args, device, hp, seed_base, etas, premodels, _pos_weight)
    shared_order = {}
    fail_rank = _TEST_FAIL_RANK      # test hook (module attribute, set by tests only): this rank's FIRST share raises (population.train_sharded re-queues it)
    attempts = [0]

    def train_share(mine):
        """This rank's share (or a re-queued part of a failed rank's): {candidate index: best dev metric}."""
        attempts[0] += 1
        if world > 1 and rank == fail_rank and attempts[0] == 1:
            raise RuntimeError("_TEST_FAIL_RANK: simulated failure of this rank's share")
        acc_by_idx = {}
        if mine and not per_cand and "o" not in shared_order:
            shared_order["o"] = make_order(N_tr, E, train_l.shuffle, seed_base + 1, device)
        order = shared_order.get("o")
        for group, pop in _plan_rounds(hp, confs, mine, device, seed_base, int(getattr(args, "engine_chunk_cols", 0))):
            try:
                if _pos_weight is not None:
                    pop.set_pos_weight(_pos_weight)
                mods = {}
                init_population(pop, group, args=args, confs=confs, hp=hp, seed_base=seed_base, device=device,
                                searchable_type=searchable_type, premodels=premodels, return_model=return_model, mods=mods)
                if getattr(args, "verbose", False):
                    print("Now training: ")
                    for i in group:
                        print(confs[i])
                if getattr(args, "engine_profile", False):
                    pop.set_profiling(True)
                if per_cand:
                    order = make_order_per_candidate(N_tr, E, train_l.shuffle, seed_base + 1, device, group)
                stats, status = pop.train(train_l.table, dev_l.table, E, etas, order=order,
                                          snapshot_best=bool(return_model))
                if getattr(args, "engine_profile", False):
                    PROFILE.append(pop.sweep_profile() + (pop.schedule(),))
                for j, i in enumerate(group):
                    if getattr(args, "verbose", False):
                        print_epoch_stats(stats[j], N_tr, N_dev)
                    acc_by_idx[i] = (best_dev_f1(stats[j], bool(status[j]), N_dev) if hp.loss_mode == 1
                                     else best_dev_accuracy(stats[j], N_dev))
                    if return_model:
                        m = mods.get(i) or searchable_type(args, confs[i])
                        load_trained(m, pop.get_params(j), E * nb, device)
                        models[i] = m
            finally:
                pop.close()
        return acc_by_idx

    # ONE all_gather of (index, accuracy) pairs (RCCL on the GPU box); a rank whose share fails is re-queued, never waited for
    accs_all = popmod.train_sharded(wanted, owner, cap, K, costs, train_share, device)
    real_accuracies = [accs_all[i] for i in wanted]
    if return_model:
        # models live on the rank that trained them; other ranks get None placeholders
        return real_accuracies, [models.get(i) for i in wanted]
    return real_accuracies


def _check_halving(args, return_model):
    """args.engine_halving = (eta, rungs), e.g. (2, (1, 3)): None when unset; refused — before a loader is read or a population
    created — where the ranking or the survivors' move has nothing to stand on."""
    halving = getattr(args, "engine_halving", None)
    if halving is None:
        return None
    eta, rungs = int(halving[0]), tuple(int(r) for r in halving[1])
    E = int(args.epochs)
    if eta < 2 or not rungs or list(rungs) != sorted(set(rungs)) or rungs[0] < 1 or rungs[-1] >= E:
        raise ValueError(f"args.engine_halving = (eta, rungs): eta >= 2 and 1 <= rungs[0] < rungs[1] < ... < epochs = {E}; got {halving!r}")
    if getattr(args, "weightsharing", False):
        raise NotImplementedError("engine_halving with --weightsharing: candidates that start from the cells earlier candidates "
                                  "published train one after the other; there is no population to rank")
    if return_model:
        raise NotImplementedError("engine_halving with return_model: an eliminated candidate has no fully trained model to return")
    if popmod.dist_info()[1] > 1:
        raise NotImplementedError("engine_halving with world > 1: ranking candidates across ranks needs a collective per rung that has "
                                  "never run on hardware; run the search call on one GPU")
    return eta, rungs


def _train_halving(halving, confs, searchable_type, train_l, dev_l, args, device, hp, seed_base, etas, premodels, _pos_weight):
    """train_sampled_models with successive halving (args.engine_halving = (eta, rungs), one GPU): every candidate trains epochs
    [0, rungs[0]); after each rung the candidates are ranked by their best dev metric so far (population.halving_survivors) and the
    best ceil(K_i / eta) go on to the next rung, the last rung's survivors to the end.  The eta table, the per-candidate sample
    orders, the initial parameters and the dropout seeds are those of the full schedule by INPUT index, so a survivor trains exactly
    what it would have trained without halving.  Survivors are regrouped with _plan_rounds — a smaller rung may take another
    schedule — and carried over with Population.move_from; while a rung changes, the old and the new populations are both alive.
    An eliminated candidate returns its best dev metric over the epochs it ran (train_searchable/ntu.py:82-83)."""
    eta, rungs = halving
    K = len(confs)
    N_tr, N_dev, E = len(train_l.table), len(dev_l.table), int(args.epochs)
    per_cand = bool(hp.order_per_candidate)
    chunk_cols = int(getattr(args, "engine_chunk_cols", 0))
    shared = None if per_cand else make_order(N_tr, E, train_l.shuffle, seed_base + 1, device)
    stats_of = {i: np.zeros(E, EPOCH_STATS_DTYPE) for i in range(K)}
    status_of = {i: 0 for i in range(K)}
    ran = {i: 0 for i in range(K)}

    def metric(i):
        row = stats_of[i][:ran[i]]
        return best_dev_f1(row, bool(status_of[i]), N_dev) if hp.loss_mode == 1 else best_dev_accuracy(row, N_dev)

    def order_of(group):      # the full schedule's orders of these candidates (a function of the input index, not of the round)
        return make_order_per_candidate(N_tr, E, train_l.shuffle, seed_base + 1, device, group) if per_cand else shared

    alive = list(range(K))
    rounds = []        # [(input indices, Population, sample orders)]
    try:
        for group, pop in _plan_rounds(hp, confs, alive, device, seed_base, chunk_cols):
            rounds.append((group, pop, order_of(group)))
            if _pos_weight is not None:
                pop.set_pos_weight(_pos_weight)
            init_population(pop, group, args=args, confs=confs, hp=hp, seed_base=seed_base, device=device,
                            searchable_type=searchable_type, premodels=premodels, return_model=[], mods={})
        first = 0
        for stop in list(rungs) + [E]:
            for group, pop, order in rounds:
                stats, status = pop.train(train_l.table, dev_l.table, E, etas, order=order, first_epoch=first, last_epoch=stop)
                for j, i in enumerate(group):
                    stats_of[i][first:stop] = stats[j, first:stop]
                    status_of[i] = int(status[j])
                    ran[i] = stop
            if stop == E:
                break
            keep = popmod.halving_survivors([metric(i) for i in alive], [status_of[i] for i in alive], eta)
            alive = [alive[p] for p in keep]
            where = {i: (pop, j) for group, pop, _ in rounds for j, i in enumerate(group)}
            old, rounds = rounds, []
            t_change = time.perf_counter()       # (the last train() call has synchronised its stream)
            try:
                for group, pop in _plan_rounds(hp, confs, alive, device, seed_base, chunk_cols):
                    rounds.append((group, pop, order_of(group)))
                    if _pos_weight is not None:
                        pop.set_pos_weight(_pos_weight)
                    for j, i in enumerate(group):
                        pop.move_from(where[i][0], where[i][1], j)
                    torch.cuda.current_stream(device).synchronize()
            finally:
                for _, pop, _ in old:
                    pop.close()
            if getattr(args, "engine_profile", False):
                RUNG_CHANGES.append((len(where), len(alive), time.perf_counter() - t_change))
            first = stop
    finally:
        for _, pop, _ in rounds:
            pop.close()
    return [metric(i) for i in range(K)]


def _train_weightsharing(confs, wanted, searchable_type, train_l, dev_l, args, device, hp, seed_base,
                         return_model, premodels, state_dict):
    """--weightsharing makes candidates sequentially dependent (each starts from the cells the previous ones
    published, ntu_searchable.py:74-75,91-92): "replicas only" — every rank trains the whole list serially."""
    N_tr, N_dev, B, E = len(train_l.table), len(dev_l.table), int(args.batchsize), int(args.epochs)
    nb = -(-N_tr // B)
    accs, models = [], []
    for i in wanted:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed_base + 2 + i)
            m = searchable_type(args, confs[i])
        if premodels:
            m.load_state_dict(premodels[i].state_dict())
        set_central_states(m, state_dict, False)
        # (a fresh scheduler per candidate, from N_tr / B like ntu_searchable.py:30,60 — not the call's one table: kept apart on purpose)
        sched = LRCosineAnnealingScheduler(args.eta_max, args.eta_min, args.Ti, args.Tm, N_tr / B)
        if getattr(args, "verbose", False):
            print("Now training: ")
            print(confs[i])
        stats, _ = train_one(m, hp, train_l, dev_l, E, sched.eta_table(E * nb), device,
                             drop_seed=seed_base * 7 + i, order_seed=seed_base + 1 + 1000 * i)
        if getattr(args, "verbose", False):
            print_epoch_stats(stats[0], N_tr, N_dev)
        get_central_states(m, state_dict, False)        # (published from the host copy, before the model moves)
        accs.append(best_dev_accuracy(stats[0], N_dev))
        if return_model:
            m.to(device)
            models.append(m)
    return (accs, models) if return_model else accs
