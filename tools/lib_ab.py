"""Two BUILT engine libraries on the same seeded small populations, each in its own child process (MFAS_LIB, loaded once per process):
the W, m and v planes of every candidate, the per-epoch statistics and the status words must be the same BYTES.
usage: lib_ab.py LIB_A LIB_B                       bytes A/B over every case below; exit status 1 on a difference
       lib_ab.py LIB_A LIB_B --time CASE [ROUNDS]  ms per train() of one case, the libraries alternating (A B A B ...), one process each
                                                   (CASE search_call: ms per create + init + train + destroy of a small resident population)
The cases are the smallest that reach each statement of the general chain (chain_body at 1 / 2 / 4 batch blocks: launch per phase,
fused, same-group), of chain_split (K = 1, K = 3, the two-group launch) and of the wide path, with every head (<= 64 classes, more,
multitask, multi-label), BatchNorm on / off, alphas and dropout: the case and schedule tables of tests/test_gpu_ref64.py,
tests/test_gpu_train_ref64.py and tests/test_gpu_wide_ref64.py, six batches (five full, one ragged), two epochs."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FULL = 5        # full batches in front of the ragged one

SPLIT = lambda s: s["chain_cus"] == 4
# TRAIN_SCHEDULES entries by name, or (base entry name, replacement (R, C, B, env, chunk_cols, K, tap_bits, check) or None, hyper edits)
# Replacement entries take their pieces from existing tables: the per-phase / fused entries are SCHEDULES' general_mb1 / mb2 / mb4 shapes
# under MFAS_SAME_GROUP=0 with K = 3 (one group) or K = 8 (two groups, like two_group_ab); split_k1 is the chain_split entry at K = 1;
# split_two_group draws R = 120, C = 23, B = 12 from tests/test_gpu_parity.py::test_chain_split_bit_identical (R from 128 / 120 / 113,
# C from 60 / 23 / 7, B from 16 / 12 / 5) at K = 8, the smallest two-group population.
SCHED_CASES = {
    "body_mb1": ("general_mb1", None, {}),
    "body_mb2": ("general_mb2", None, {}),
    "body_mb4": ("general_mb4", None, {}),
    "body_mb1_per_phase": ("general_mb1", (65, 60, 16, {"MFAS_CHAIN_SPLIT": "0", "MFAS_SAME_GROUP": "0"}, 0, 3, 0, lambda s: s["groups"] == 1), {}),
    "body_fused_ab": ("two_group_ab", None, {}),
    "body_mb2_fused_ab": ("general_mb2", (65, 17, 20, {"MFAS_SAME_GROUP": "0"}, 0, 8, 0, lambda s: s["groups"] == 2), {}),
    "body_mb4_fused_ab": ("general_mb4", (33, 17, 64, {"MFAS_SAME_GROUP": "0"}, 0, 8, 0, lambda s: s["groups"] == 2), {}),
    "body_tap_major": ("tap_major", None, {}),
    "body_same_group": ("same_group", None, {}),
    "body_mb1_multitask": ("general_mb1", None, {"multitask": True}),
    "body_mb2_nobn_multilabel": ("general_mb2", None, {"bn": False, "loss_mode": 1}),
    "split_k3": ("chain_split", None, {}),
    "split_k1": ("chain_split", (128, 60, 16, {"MFAS_SAME_GROUP": "2"}, 128, 1, 0, lambda s: s["groups"] == -1 and SPLIT(s)), {}),
    "split_two_group": ("chain_split", (120, 23, 12, {"MFAS_SAME_GROUP": "0"}, 128, 8, 0, lambda s: s["groups"] == 2 and SPLIT(s)), {}),
    "split_multitask_nobn": ("chain_split", None, {"multitask": True, "bn": False}),
    "split_multilabel": ("chain_split", None, {"loss_mode": 1}),
    # host-bound: the lean chain launch per phase (R = 16, B = 20, MFAS_PERSIST=0), one group, chain + sweep = two launches per step
    "lean_per_phase": ("lean_chain", None, {}),
}
# single-candidate cases of ref64_cases.CASES (general chain: more than 64 classes, alphas, multi-label, multitask, no BatchNorm)
ENVELOPE_CASES = ("r17a", "r32a", "r33a", "r65b", "r80a", "r128a", "r128b")
# wide_cases.WIDE_CASES: B > 64, R > 128, every head, alphas
WIDE = ("wb65", "wb128", "w177", "w256", "w80", "wc")


def run_search_call(dev, reps):
    """--time search_call: what one round of the search pays per population — create, init, train, destroy of a small resident
    population (R = 16, 6 candidates of 1..4 cells, 16-bit tables, 2 epochs of 20 batches, dev pass, kept best) — timed as ONE call, so
    that allocation and release are inside the measurement.  -> like run_case"""
    import numpy as np
    import torch
    from mfas_amd import FeatureTable, Hyper, Population
    from oracle import np_oracle as O
    from tests.helpers import CONFS
    hp = Hyper(R=16, C=60, B=20, bn=False, drpt=0.5, tap_bits=16)
    confs = [np.array(CONFS[c]) for c in ("c4", "c0", "l1", "l2", "l3", "c4")]
    tr, dv = FeatureTable.synthetic(400, 1, dev, torch.bfloat16, snr=0.5), FeatureTable.synthetic(200, 2, dev, torch.bfloat16, snr=0.5)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, 400 / 20, 2 * 20)
    h, best, sched, ok = hashlib.sha256(), None, None, True
    for rep in range(max(1, reps)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pop = Population(hp, confs, dev, drop_seeds=list(range(1, 7)))
        pop.init(list(range(11, 17)))
        stats, status = pop.train(tr, dv, 2, etas, snapshot_best=True)
        if rep == 0:
            sched = pop.schedule()
            assert sched["persistent"], sched
        pop.close()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        if rep == 0:
            h.update(np.ascontiguousarray(stats).tobytes())
            ok = not np.asarray(status).any()
    return h.hexdigest(), {k: sched[k] for k in ("wide", "lean_chain", "chain_cus", "groups", "persistent")}, best, ok


def run_case(name, dev, reps):
    """-> (sha256 over planes / statistics / status, schedule, best seconds of a train() call)"""
    import numpy as np
    import torch
    from tests import gpu_support as G
    from tests import train_gpu as GT
    from tests import wide_gpu as GW
    if name == "search_call":
        return run_search_call(dev, reps)
    if name in SCHED_CASES:
        base, entry, edits = SCHED_CASES[name]
        entry = entry or GT.TRAIN_SCHEDULES[base]

        def hyper(hp):
            for k, v in edits.items():
                setattr(hp, k, v)
            return hp
        inp = GT.schedule_inputs(name, "shared", FULL, entry=entry, hyper=hyper)
        pop = GT.schedule_pop(name, inp, dev, entry=entry)
        if inp["hp"].loss_mode == 1:
            pop.set_pos_weight(G.pos_weight(inp["hp"]))
        p0s, t, dtype, order, etas = inp["p0s"], inp["t"], inp["dtype"], inp["order"], inp["etas"]
    elif name in WIDE:
        case = GW.WIDE_CASES[GW.WIDE_IDS.index(name)]
        hp, ehp, seed, confs, p0s, seeds, pop = GW.setup(case, dev)
        assert pop.schedule()["wide"] == 1, pop.schedule()
        N, t, order, etas = GW.train_inputs(case, hp, ehp, seed, FULL)
        dtype = case[9]
    else:
        case = G.CASES[G.CASE_IDS.index(name)]
        hp = G.case_hyper(case)
        seed = GT.SEED0 + G.CASE_IDS.index(name)
        conf, p0 = G.case_params(case, hp, seed)
        N = GT.train_rows(hp.B, FULL)
        t, dtype, order, etas, p0s = G.case_table(case, hp, N, seed, GT.case_dtype(name)), GT.case_dtype(name), GT.make_order(N, seed), GT.step_etas(N, hp.B), [p0]
        pop = G.make_pop(hp, conf, dev, seed)
    try:
        sched = pop.schedule()
        tab, order_t = G.gpu_table(t, dtype, dev), torch.from_numpy(order).to(dev)
        h, best = hashlib.sha256(), None
        for rep in range(max(1, reps)):
            for k, p0 in enumerate(p0s):
                pop.set_state_dict(k, p0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats, status = pop.train(tab, None, GT.EPOCHS, etas, order=order_t, max_steps=len(etas))     # (every step of both epochs; no dev table)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            if rep == 0:
                h.update(np.ascontiguousarray(stats).tobytes())
                h.update(np.ascontiguousarray(status).tobytes())
                for k in range(len(p0s)):
                    for plane in range(3):
                        h.update(pop.get_params(k, plane).cpu().numpy().tobytes())
                ok = not np.asarray(status).any()
    finally:
        pop.close()
    return h.hexdigest(), {k: sched[k] for k in ("wide", "lean_chain", "chain_cus", "groups", "persistent")}, best, ok


def child(out, names, reps):
    import torch
    from mfas_amd import _lib
    dev = torch.device("cuda:0")
    res = {"lib": _lib.LIB_PATH}
    for name in names:
        sha, sched, best, ok = run_case(name, dev, reps)
        res[name] = {"sha": sha, "sched": sched, "ms": best * 1e3, "status_clean": ok}
        print(f"  {name:28s} {sha[:16]} {best * 1e3:8.2f} ms  {sched}", flush=True)
    with open(out, "w") as f:
        json.dump(res, f)


def run_lib(lib, names, reps):
    """One fresh process for one library; a child that fails ends the whole run (nothing more is started on the device)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "res.json")
        print(f"# {os.path.basename(lib)}", flush=True)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, ",".join(names), str(reps)],
                       env=dict(os.environ, MFAS_LIB=os.path.abspath(lib)), check=True, timeout=600)
        return json.load(open(out))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3].split(","), int(sys.argv[4]))
    lib_a, lib_b = sys.argv[1], sys.argv[2]
    if len(sys.argv) > 3 and sys.argv[3] == "--time":
        name, rounds = sys.argv[4], int(sys.argv[5]) if len(sys.argv) > 5 else 5
        ms = {lib_a: [], lib_b: []}
        for r in range(rounds):
            for lib in (lib_a, lib_b) if lib_a != lib_b else (lib_a,):
                ms[lib].append(run_lib(lib, [name], 10)[name]["ms"])
        for lib, v in ms.items():
            v = sorted(v)
            print(f"{name} {os.path.basename(lib)}: best-of-10 ms per train() over {len(v)} processes: min {v[0]:.3f} median {v[len(v) // 2]:.3f} max {v[-1]:.3f}")
        return 0
    names = list(SCHED_CASES) + list(ENVELOPE_CASES) + list(WIDE)
    a, b = run_lib(lib_a, names, 1), run_lib(lib_b, names, 1)
    bad = 0
    for name in names:
        same = a[name]["sha"] == b[name]["sha"] and a[name]["sched"] == b[name]["sched"]
        bad += not same
        print(f"{'identical' if same else 'DIFFERS  '} {name:28s} {a[name]['sha'][:16]} {b[name]['sha'][:16]} status_clean={a[name]['status_clean']} {a[name]['sched']}")
    print(f"{len(names)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
