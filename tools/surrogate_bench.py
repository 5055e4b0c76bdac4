#!/usr/bin/env python3
"""The surrogate's three backends side by side on one GPU, in one process (profiles/engine_surrogate.log):

* per-train-step time of the 4-thread CPU module, GraphedSurrogateTrainer and EngineSurrogateTrainer at two bucket sets shaped like an
  early and a late search call ([32] rows of length 1; [32, 250, 350, 350] rows of lengths 1..4), repeats interleaved between the
  backends, every timed window ending in a device synchronise;
* one timed_search of the config-4 schedule (50 samples x 5 iterations x 4 levels) per backend: candidate training / controller split;
* the gradient-deviation ratios of tests/test_gpu_surrogate_engine.py (largest per tensor over its cases);
* registers and spills of the three kernels (tools/kernel_resources.py).

usage: python tools/surrogate_bench.py [--out profiles/engine_surrogate.log] [--repeats 5] [--epochs 20] [--no-search]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUCKET_SETS = {"early [32]": [(1, 32)], "late [32, 250, 350, 350]": [(1, 32), (2, 250), (3, 350), (4, 350)]}


def draw(sets, seed=0):
    rng = np.random.default_rng(seed)
    xs = [torch.from_numpy(np.stack([rng.integers(0, 4, (L, n)), rng.integers(0, 4, (L, n)), rng.integers(0, 2, (L, n))], 2).astype(np.float32))
          for L, n in sets]
    ys = [torch.from_numpy(rng.uniform(0.2, 0.9, (n, 1)).astype(np.float32)) for _, n in sets]
    return xs, ys


def step_times(out, repeats, epochs):
    from mfas_amd.search import surrogate as S
    dev = torch.device("cuda:0")
    crit = torch.nn.MSELoss()
    for name, sets in BUCKET_SETS.items():
        data = draw(sets)
        torch.manual_seed(0)
        models = {"cpu (4 threads)": (S.SimpleRecurrentSurrogate(100, 3, 100), "cpu"),
                  "graphed": (S.SimpleRecurrentSurrogate(100, 3, 100).to(dev), dev),
                  "engine": (S.EngineSurrogate(100, 3, 100).to(dev), dev)}
        opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3, **({"capturable": True, "foreach": True} if k == "graphed" else {}))
                for k, (m, _) in models.items()}
        times = {k: [] for k in models}
        for rep in range(repeats + 1):        # (repeat 0 warms up: graph capture, code objects, optimizer state)
            for k, (m, d) in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.train_simple_surrogate(m, crit, opts[k], data, epochs, d)
                torch.cuda.synchronize()
                if rep:
                    times[k].append((time.perf_counter() - t0) / (epochs * len(sets)) * 1e3)
        out(f"bucket set {name} (L, n) = {sets}: ms per train step over {repeats} interleaved repeats of {epochs} epochs "
            f"(whole train call / steps: upload, launches, final synchronise included)")
        for k, v in times.items():
            out(f"  {k:16s} median {np.median(v):8.4f}  min {min(v):8.4f}  max {max(v):8.4f}")
        # prediction: one batched call of 1600 configurations of length 4 (a search step's unfolded candidates)
        x = draw([(4, 1600)], 1)[0][0]
        for k, (m, d) in models.items():
            xd = x.to(d)
            v = []
            with torch.no_grad():
                for rep in range(repeats + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m(xd).cpu()
                    if rep:
                        v.append((time.perf_counter() - t0) * 1e3)
            out(f"  {k:16s} 1600 predictions (L = 4), ms: median {np.median(v):8.4f}")


def searches(out):
    import bench
    import main_searchable_ntu as MS
    from mfas_amd.search import NTUSearcher
    from mfas_amd.search.searcher import timed_search
    dev = torch.device("cuda:0")
    train, devt = bench.synth_tables(10000, 5600, dev, torch.bfloat16)
    sa = MS.parse_args(["--num_samples", "50", "--search_iterations", "5", "--max_fusions", "4", "--epochs", "3", "--no-verbose"])
    torch.set_num_threads(max(1, sa.controller_threads))
    out("config-4 schedule (50 samples x 5 iterations x 4 levels, N_train 10000, N_dev 5600, 3 epochs), one timed_search per backend; "
        "the first search of the process also pays the one-off costs (imports, code objects), so cpu runs twice")
    for backend in ("cpu", "cpu", "gpu", "engine"):
        sd = {"cpu": "cpu", "gpu": dev, "engine": "engine"}[backend]
        _, rep = timed_search(NTUSearcher(sa, dev, {"train": train, "dev": devt}), seed=0, surrogate_device=sd)
        out(f"  {backend:7s} total {rep['total_s']:.2f} s = training {rep['train_s']:.2f} s + controller {rep['controller_s']:.2f} s "
            f"({rep['candidates']} candidates, {rep['calls']} calls, decisions {rep['decision_digest']}, best dev acc {rep['best_dev_acc']:.4f})")


def ratios(out):
    sys.argv = sys.argv[:1]
    import pytest
    from tests import surr_cases as T
    # the test records its ratios in tests/surr_cases.py's RATIOS: run it in this process, then read them there
    rc = pytest.main(["-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_surrogate_engine.py"), "-k", "test_gradient_element_by_element"])
    assert rc == 0, rc
    out("gradient: largest |g_engine - g64| / max(float32-CPU yardstick, 2^-20 max|g64|) per tensor over "
        f"{len(T.CASES)} cases (shapes {T.S.SHAPES}, L in 1, 2, 4, n in {T.TILE_NS}); the test's bound is 4")
    for k, r in T.RATIOS.items():
        out(f"  {k:22s} {r:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "engine_surrogate.log"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--no-search", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.set_num_threads(4)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"tools/surrogate_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, 4 CPU threads")
    step_times(out, a.repeats, a.epochs)
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ratios(lambda s: lines.append(s))
    for s in lines[-9:]:
        print(s, flush=True)
    if not a.no_search:
        searches(out)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    out(KR.HEADER)
    for nm, row in KR.resource_rows(KR.code_object(os.path.join(ROOT, "mfas_amd", "csrc", "libmfas_hip.so"))).values():
        if "k_surr" in nm:
            out(f"{nm[:72]:72s} {row}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
