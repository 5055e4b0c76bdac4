"""Small-population sweep: candidates/s of one train_sampled_models-sized job (E epochs over N_train / N_dev) for K candidates on
one GPU, launch-per-phase schedule (MFAS_PERSIST=0) vs the default policy (persistent resident step loop where it fits), each with its own default unit
decomposition.  usage: popsweep.py R B bn E K1,K2,... [mixed] [N_train N_dev]   |   popsweep.py wide  (batch-64 rows, see wide_rows)
|   popsweep.py halving  (one search call with and without successive halving, see halving_rows)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mfas_amd as M
from oracle import np_oracle as O


def wide_rows():
    """usage: popsweep.py wide — us per train step of conf-4 populations at batch 64 (R = 256: the wide path; R = 128: the widest
    batch-resident shape at that batch) next to the same widths at batch 32, K = 1, 16, 64, bf16 taps, BatchNorm, shared order.
    A step's time is the difference of a 240- and a 40-step call (best of three each, after one warm-up call) over 200 steps;
    bytes per step from the byte model (24 P + B * sum(F) * 2 + 8 B per candidate)."""
    dev = torch.device("cuda:0")
    conf4 = np.array([[3, 1, 1], [1, 3, 0], [1, 1, 1], [3, 3, 0]])
    T1, T2 = 40, 240
    print("# R B K: schedule, us/step, rows/s, MB/step (byte model), fraction of 8 TB/s")
    for R, B in ((256, 64), (256, 32), (128, 64), (128, 32)):
        hp = M.Hyper(R=R, B=B, bn=True, drpt=0.5, tap_bits=16)
        N = T2 * B
        tr = M.FeatureTable.synthetic(N, 1, dev, torch.bfloat16, snr=0.12)
        etas = np.full(T2, 1e-3)
        order = M.ntu_searchable.make_order(N, 1, True, 5, dev)
        feat = sum(hp.s_sizes[c[0]] + hp.v_sizes[c[1]] for c in conf4)
        P = sum(R * (hp.s_sizes[c[0]] + hp.v_sizes[c[1]] + (R if i else 0)) for i, c in enumerate(conf4)) + hp.C * R
        for K in (1, 16, 64):
            pop = M.Population(hp, [conf4] * K, dev, drop_seeds=list(range(100, 100 + K)))
            try:
                pop.init(list(range(1, K + 1)))
                sched = pop.schedule()
                best = {}
                for T in (T1, T1, T2, T1, T2, T1, T2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pop.train(tr, None, 1, etas, order=order, max_steps=T)
                    dt = time.perf_counter() - t0
                    if T != T1 or "warm" in best:
                        best[T] = min(best.get(T, 1e30), dt)
                    best["warm"] = 1
            finally:
                pop.close()
            us = (best[T2] - best[T1]) / (T2 - T1) * 1e6
            mb = K * (24.0 * P + B * feat * 2 + 8 * B) / 1e6
            name = "wide" if sched.get("wide") else ("same-group" if sched["groups"] == -1 else f"{sched['groups']} group(s)")
            print(f"R={R:3d} B={B:2d} K={K:2d}  {name:10s} {us:8.1f} us/step  {K * B / us * 1e6:12.0f} rows/s  {mb:8.1f} MB/step  "
                  f"{mb / us / 8e6 * 1e6:.3f} of 8 TB/s", flush=True)


def halving_rows():
    """usage: popsweep.py halving — seconds per train_sampled_models call at R = 128, B = 16, E = 10 over 10000 / 5600 bf16 rows,
    conf-4 candidates, K = 16 and 128, without and with args.engine_halving = (2, (1, 3)) (best of two calls each after one warm-up
    call at K = 16), and what one rung change costs (regrouping + mfas_population_move of the survivors + destroying the old population)."""
    from types import SimpleNamespace
    dev = torch.device("cuda:0")
    conf4 = np.array([[3, 1, 1], [1, 3, 0], [1, 1, 1], [3, 3, 0]])
    tr = M.FeatureTable.synthetic(10000, 1, dev, torch.bfloat16, snr=0.12)
    dv = M.FeatureTable.synthetic(5600, 2, dev, torch.bfloat16, snr=0.12)
    ld = {"train": M.FeatureLoader(tr, 16, shuffle=True), "dev": M.FeatureLoader(dv, 16, shuffle=False)}
    print("# R=128 B=16 E=10 N=10000/5600 conf 4: K, s/call plain, s/call engine_halving=(2,(1,3)), ratio, rung changes (candidates -> survivors: ms)")
    for K in (16, 16, 128):
        out = {}
        for halving in (None, (2, (1, 3))):
            args = SimpleNamespace(vid_len=(8, 32), num_outputs=60, drpt=0.5, inner_representation_size=128, batchnorm=True, alphas=False,
                                   multitask=False, weightsharing=False, batchsize=16, eta_max=1e-3, eta_min=1e-6, Ti=1, Tm=2,
                                   use_dataparallel=False, verbose=False, epochs=10, engine_halving=halving, engine_profile=True)
            best = None
            for rep in range(2):
                del M.ntu_searchable.RUNG_CHANGES[:]
                torch.manual_seed(3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                M.train_sampled_models([conf4] * K, M.Searchable_Skeleton_Image_Net, ld, args, dev)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            out[halving is not None] = best
        rc = ", ".join(f"{a} -> {b}: {s * 1e3:.2f} ms" for a, b, s in M.ntu_searchable.RUNG_CHANGES)
        print(f"K={K:4d}  plain {out[False]:8.3f} s   halving {out[True]:8.3f} s   x{out[False] / out[True]:.2f}   {rc}", flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "halving":
    halving_rows()
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "wide":
    wide_rows()
    sys.exit(0)

R, B, bn, E = (int(x) for x in sys.argv[1:5])
Ks = [int(x) for x in sys.argv[5].split(",")]
mixed = "mixed" in sys.argv
cc = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("cc=")), 0)
nums = [int(a) for a in sys.argv[6:] if a.isdigit()]
E_show = E
N, Nd = (nums + [10000, 5600])[:2] if len(nums) >= 2 else (10000, 5600)
dev = torch.device("cuda:0")
tr = M.FeatureTable.synthetic(N, 1, dev, torch.bfloat16, snr=0.12)
dv = M.FeatureTable.synthetic(Nd, 2, dev, torch.bfloat16, snr=0.12)
hp = M.Hyper(R=R, B=B, bn=bool(bn), drpt=0.5, tap_bits=16)
conf4 = np.array([[3, 1, 1], [1, 3, 0], [1, 1, 1], [3, 3, 0]])
nb = -(-N // B)
etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N / B, E * nb)
order = M.ntu_searchable.make_order(N, E, True, 5, dev)
print(f"# R={R} B={B} bn={bn} E={E} N={N}/{Nd} {'mixed L=1..4 confs' if mixed else 'conf 4'}: K, cand/s launch-per-phase, cand/s persistent, us/step each, ratio")
for K in Ks:
    confs = [conf4] * K
    if mixed:
        rng = np.random.default_rng(0)
        confs = [np.stack([rng.integers(0, 4, L), rng.integers(0, 4, L), rng.integers(0, 2, L)], 1) for L in rng.integers(1, 5, K)]
    out = {}
    for mode in ("0", "1"):          # "1" = the engine's default policy (persistent where the resident form fits), "0" = forced off
        if mode == "0":
            os.environ["MFAS_PERSIST"] = "0"
        else:
            os.environ.pop("MFAS_PERSIST", None)
        best = None
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                pop = M.Population(hp, confs, dev, drop_seeds=list(range(100, 100 + K)), chunk_cols=cc)
                pop.init(list(range(1, K + 1)))
                stats, status = pop.train(tr, dv, E, etas, order=order)
                pop.close()
            except RuntimeError as e:
                print("  ", K, mode, "failed:", str(e)[:120])
                best = float("nan")
                break
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[mode] = best
    print(f"K={K:4d}  launch {K / out['0']:8.2f} cand/s ({out['0'] / (E * nb) * 1e6:6.1f} us/step)   default {K / out['1']:8.2f} cand/s "
          f"({out['1'] / (E * nb) * 1e6:6.1f} us/step)   x{out['0'] / out['1']:.2f}", flush=True)
