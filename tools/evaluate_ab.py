#!/usr/bin/env python3
"""Time Population.evaluate against what the engine offered before it, in one process.

Workload: K = 128 x NTU conf 4, R = 128, bf16 tables, N = 5,600 rows, C = 60; M in {5, 16, 128} members.
  (a) the Python loop of Population.forward(k, table) into a stacked buffer, then torch softmax, weighted mean, argmax and a
      compare-and-sum;
  (b) Population.evaluate(table, members) with the default scratch (64 MiB: at M = 128 the table is walked in three row blocks);
  (c) the same with scratch_bytes sized for the whole table (one row block).
Both paths are warmed up, then alternated; at least 5 repeats each; a host clock around a device synchronise; medians and spread
(min .. max).  Also prints k_vote's algorithmic bytes per call.  k_vote's own kernel time comes from a separate run under
rocprofv3 --kernel-trace --stats (the program goes after `--`), its bytes/s against --probe (mfas_stream_probe) on the same box.

    python tools/evaluate_ab.py [--repeats 7] [--probe] [--only-evaluate M]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONF4 = [[3, 1, 1], [1, 3, 0], [1, 1, 1], [3, 3, 0]]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pop", type=int, default=128)
    ap.add_argument("--rows", type=int, default=5600)
    ap.add_argument("--probe", action="store_true", help="also print mfas_stream_probe's GB/s")
    ap.add_argument("--only-evaluate", type=int, default=0, metavar="M", help="run evaluate() alone with M members (for a profiler run)")
    args = ap.parse_args(argv)
    assert args.repeats >= 5
    import ctypes
    from mfas_amd import FeatureTable, Hyper, Population, _lib
    dev = torch.device("cuda:0")
    K, N, C = args.pop, args.rows, 60
    hp = Hyper(R=128, C=C, B=16, bn=True, drpt=0.5, tap_bits=16)
    table = FeatureTable.synthetic(N, 3, dev, torch.bfloat16, C=C)
    pop = Population(hp, [np.array(CONF4)] * K, dev)
    pop.init(list(range(1, K + 1)))

    def path_a(members):
        buf = torch.empty((len(members), N, C), dtype=torch.float32, device=dev)
        for j, k in enumerate(members):
            buf[j] = pop.forward(k, table)
        p = torch.softmax(buf, 2)
        w = torch.full((len(members), 1, 1), 1.0 / len(members), device=dev)
        pbar = (w * p).sum(0)
        member = (buf.argmax(2) == table.label[None]).sum(1)
        return member.cpu(), int((pbar.argmax(1) == table.label).sum())

    def path_b(members, scratch_bytes=0):
        res = pop.evaluate(table, members=members, scratch_bytes=scratch_bytes)
        return res["member_stats"]["dev_corrects"], res["ensemble"]["corrects"]

    def path_c(members):
        return path_b(members, 4 * len(members) * N * C)

    def timed(fn, members):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(members)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    if args.only_evaluate:
        members = list(range(min(args.only_evaluate, K)))
        for _ in range(3):
            path_b(members)
        torch.cuda.synchronize(dev)
        print(f"evaluate alone: M = {len(members)}, 3 calls")
        return
    print(f"evaluate_ab: K = {K} x conf 4, R = 128, bf16, N = {N}, C = {C}; {args.repeats} repeats each, alternated; milliseconds")
    for M in (5, 16, 128):
        members = list(range(min(M, K)))
        ma, ea = path_a(members)
        mb, eb = path_b(members)
        mc, ec = path_c(members)
        same = ma.tolist() == list(mb) == list(mc) and eb == ec
        ta, tb, tc = [], [], []
        for _ in range(args.repeats):
            ta.append(timed(path_a, members))
            tb.append(timed(path_b, members))
            tc.append(timed(path_c, members))
        vote_bytes = 4 * len(members) * N * C + 4 * N * (C + 1) + 4 * N       # logits in; scores, row loss, labels
        print(f"M = {len(members):3d}  (a) forward loop + torch: median {statistics.median(ta):8.3f}  [{min(ta):.3f} .. {max(ta):.3f}]   "
              f"(b) evaluate: median {statistics.median(tb):8.3f}  [{min(tb):.3f} .. {max(tb):.3f}]   "
              f"(c) evaluate, one row block: median {statistics.median(tc):8.3f}  [{min(tc):.3f} .. {max(tc):.3f}]   "
              f"a / b = {statistics.median(ta) / statistics.median(tb):.2f}   a / c = {statistics.median(ta) / statistics.median(tc):.2f}   "
              f"counts equal: {same}; ensemble corrects (a) {ea} (b) {eb}   "
              f"k_vote algorithmic bytes {vote_bytes / 1e6:.2f} MB")
    if args.probe:
        gbs = ctypes.c_double(0)
        _lib.check(_lib.lib().mfas_stream_probe(256 << 20, 5, ctypes.byref(gbs)))
        print(f"mfas_stream_probe: {gbs.value:.0f} GB/s")
    pop.close()


if __name__ == "__main__":
    main()
