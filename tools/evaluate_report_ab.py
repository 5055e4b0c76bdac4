#!/usr/bin/env python3
"""Time Population.evaluate(report=True) against the call without a report, at this commit and at its parent, and against the route
a user had before it (scores and decisions back, the tallies with torch on the device).  Writes profiles/evaluate_report.log.

Workload: K = 128 x NTU conf 4, R = 128, bf16 tables, N = 5,600 rows, C = 60; M in {5, 16, 128} members; default scratch.
  (a) evaluate() at the parent commit      — a checkout of the parent with its library built, given as --parent-tree DIR;
  (b) evaluate() at this commit;
  (c) evaluate(report=True);
  (d) evaluate(return_scores=True, return_preds=True), then confusion [M+1][C][C] and the ensemble's rank histogram with torch on
      the device, copied to the host.  (The members' rank histograms cannot be had that way: the call returns no member scores.)
  (t) (c) through another build of the library, given as --alt-lib PATH and described by --alt-note TEXT (how the two forms of
      k_tally's confusion cells were compared: one 64-bit global atomic add per row against a workgroup-private C x C LDS tile).
Every variant runs in a process of its own (one population each), the processes one after another and (a) / (b) alternated, so
that (a) is measured against itself as well.  Per process: 3 warm-up calls, then --repeats calls per M; a host clock around a
device synchronise; milliseconds.

    python tools/evaluate_report_ab.py --parent-tree DIR [--alt-lib PATH --alt-note TEXT] [--repeats 15] [--rounds 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/evaluate_report_ab.py --only-report 128
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF4 = [[3, 1, 1], [1, 3, 0], [1, 1, 1], [3, 3, 0]]
MS = (5, 16, 128)


def worker(args):
    """One variant in this process: prints one JSON line {M: [milliseconds, ...]}."""
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    from mfas_amd import FeatureTable, Hyper, Population
    dev = torch.device("cuda:0")
    K, N, C = 128, 5600, 60
    hp = Hyper(R=128, C=C, B=16, bn=True, drpt=0.5, tap_bits=16)
    table = FeatureTable.synthetic(N, 3, dev, torch.bfloat16, C=C)
    pop = Population(hp, [np.array(CONF4)] * K, dev)
    pop.init(list(range(1, K + 1)))
    lab = table.label.long()

    def plain(members):
        return pop.evaluate(table, members=members)

    def report(members):
        return pop.evaluate(table, members=members, report=True)

    def torch_route(members):
        res = pop.evaluate(table, members=members, return_scores=True, return_preds=True)
        sc = res["scores"]
        dec = torch.cat([res["preds"].long(), sc.argmax(1)[None]], 0)              # (M + 1, N)
        slot = torch.arange(dec.shape[0], device=dev)[:, None]
        conf = torch.bincount(((slot * C + lab[None]) * C + dec).reshape(-1), minlength=dec.shape[0] * C * C)
        xl = sc.gather(1, lab[:, None])
        cls = torch.arange(C, device=dev)[None]
        rank = ((sc > xl) | ((sc == xl) & (cls < lab[:, None]))).sum(1)
        hist = torch.bincount(rank, minlength=C)
        return conf.cpu().numpy(), hist.cpu().numpy()

    if args.only_report:            # for a run under a profiler: the kernels of evaluate(report=True) alone
        for _ in range(3):
            report(list(range(args.only_report)))
        torch.cuda.synchronize(dev)
        pop.close()
        print(f"evaluate(report=True) alone: M = {args.only_report}, 3 calls")
        return
    fn = {"plain": plain, "report": report, "torch": torch_route}[args.worker]
    out = {}
    for M in MS:
        members = list(range(M))
        for _ in range(3):
            fn(members)
        ts = []
        for _ in range(args.repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(members)
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        out[M] = ts
    if args.worker == "report":     # the two routes agree on what both produce
        conf, hist = torch_route(list(range(5)))
        rep = report(list(range(5)))["report"]
        assert (rep["confusion"].reshape(-1) == conf).all() and (rep["rank_hist"][-1] == hist).all()
    pop.close()
    print("RESULT " + json.dumps(out))


def run(variant, tree, repeats, lib=None):
    env = dict(os.environ)
    env.pop("MFAS_LIB", None)
    if lib:
        env["MFAS_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--tree", tree, "--repeats", str(repeats)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"{variant} in {tree} ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return {int(k): v for k, v in json.loads(line[7:]).items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--alt-lib", default="")
    ap.add_argument("--alt-note", default="another build of the library")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_report.log"))
    ap.add_argument("--worker", default="", choices=["", "plain", "report", "torch"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--only-report", type=int, default=0, metavar="M", help="run evaluate(report=True) alone with M members, three times")
    args = ap.parse_args(argv)
    if args.worker or args.only_report:
        return worker(args)
    assert args.repeats >= 5 and args.rounds >= 2
    variants = [("a", "plain", args.parent_tree, None)] if args.parent_tree else []
    variants += [("b", "plain", ROOT, None), ("c", "report", ROOT, None), ("d", "torch", ROOT, None)]
    if args.alt_lib:
        variants.append(("t", "report", ROOT, os.path.abspath(args.alt_lib)))
    runs = {v[0]: [] for v in variants}         # variant -> one {M: [ms]} per round
    for _ in range(args.rounds):
        for name, kind, tree, lib in variants:
            runs[name].append(run(kind, tree, args.repeats, lib))
    med = lambda name, M: [statistics.median(r[M]) for r in runs[name]]      # noqa: E731
    lines = [f"# tools/evaluate_report_ab.py on one MI355X: K = 128 x conf 4, R = 128, bf16, N = 5600, C = 60, default scratch; wall "
             f"milliseconds per call (host clock around a device synchronise)",
             f"# every variant in a process of its own, {args.rounds} rounds of (" + ", ".join(v[0] for v in variants) + f") one after another; "
             f"{args.repeats} calls per process and M after 3 warm-up calls",
             "# per variant: the median of each round's calls, then the smallest and largest single call over all rounds",
             "# (a) evaluate() at the parent commit  (b) evaluate() at this commit  (c) evaluate(report=True)",
             "# (d) evaluate(return_scores, return_preds) + confusion of every slot and the ensemble's rank histogram with torch, to the host",
             "# (t) (c) with " + args.alt_note]
    for M in MS:
        for name in runs:
            allc = [t for r in runs[name] for t in r[M]]
            lines.append(f"M = {M:3d}  ({name})  round medians " + "  ".join(f"{m:8.3f}" for m in med(name, M)) +
                         f"   median of medians {statistics.median(med(name, M)):8.3f}   calls [{min(allc):.3f} .. {max(allc):.3f}]")
        mm = {name: statistics.median(med(name, M)) for name in runs}
        if "a" in mm:
            sa = max(med("a", M)) - min(med("a", M))
            lines.append(f"M = {M:3d}  (a) against itself: round medians spread {sa:.3f};  (b) - (a) = {mm['b'] - mm['a']:+.3f};  "
                         f"(c) - (a) = {mm['c'] - mm['a']:+.3f} ({100 * (mm['c'] - mm['a']) / mm['a']:+.2f} %)")
        lines.append(f"M = {M:3d}  (c) - (b) = {mm['c'] - mm['b']:+.3f};  (d) - (b) = {mm['d'] - mm['b']:+.3f};  (d) / (c) = {mm['d'] / mm['c']:.3f}" +
                     (f";  (t) - (c) = {mm['t'] - mm['c']:+.3f}, round medians of (c) spread {max(med('c', M)) - min(med('c', M)):.3f}" if "t" in mm else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
