"""The sweep unit's prologue (sweep.hip.h: sweep_body of the k_step builds) requests the first pass of a unit's staged streams — its rows
of up to three batches, its dy of up to two steps — together and writes the LDS afterwards (common.hip.h: staging in two halves); what a
stream has beyond one pass still goes through the loops.  None of that changes a value, so everything a train() call leaves must equal,
BYTE FOR BYTE, what the library gave before the prologue was rearranged: tests/golden/sweep_prologue_digests.json holds, per case, the
SHA-256 of every candidate's W, m and v planes, of the statistics and of the status words, and the launch record, written by this
module run as a script (`python -m tests.test_gpu_sweep_prologue --record`, MFAS_LIB naming a build of the commit before the change).

Inputs come from numpy seeds alone (O.synth_table, numpy permutations, pop.init), so a digest does not depend on torch's generators.

Shapes: K = 8 (two groups of 4) two-cell configurations, chunk_cols = 64 over taps of 64, 48, 16 and 128 columns: chunks of 4, 3 and 1
k-blocks (a full first batch of U = 2 tiles and a second one; a second batch of one tile; a first batch of one tile).  Four batches per
epoch, the last ragged, two epochs with the dev pass: the forward-only prologue, virtual, double, plain-last and update-without-forward
launches all occur and the second epoch starts from stored planes.
  r128:   R = 128, B = 16, one row block per wave; table dtype x order (per candidate = gathered rows, shared = the table through `ord`,
          per candidate under MFAS_NO_GATHER=1) x MFAS_NT
  r32:    R = 32: k-split units (4 k-blocks: waves 4-7 own no tile; 1 k-block: wave 0 alone), xp / dyp over the reduction slabs
  b12/b5: nvalid < Bp in every batch, the zero padding
  mb2/4:  B = 32 at R = 65, B = 64 at R = 33: more than one staging pass per stream
  alphas: a two-group plan that defers nothing (the plain pass, gsc)
  k3:     one group of three, sweep launches without a chain"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as O  # noqa: E402
from tests.gpu_dev import dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep_prologue_digests.json")
S_SIZES, V_SIZES = (64, 48, 16, 128), (128, 16, 48, 64)
CHUNK, EPOCHS, FULL, N_DEV = 64, 2, 3, 50
SWITCHES = ("MFAS_GROUPS", "MFAS_NT", "MFAS_NO_GATHER", "MFAS_SAME_GROUP", "MFAS_CHAIN_SPLIT")
TWO = {"MFAS_GROUPS": "2"}
ONE = {"MFAS_SAME_GROUP": "0", "MFAS_CHAIN_SPLIT": "0"}


def _case(R, B, C=60, K=8, dtype="bfloat16", order="cand", env=TWO, groups=2, alphas=False, mb=1, wpe=4):
    return dict(R=R, B=B, C=C, K=K, dtype=dtype, order=order, env=dict(env), groups=groups, alphas=alphas, mb=mb, wpe=wpe)


CASES = {}
for _dt in ("bfloat16", "float16", "float32"):
    for _ord in ("cand", "shared", "nogather"):
        CASES[f"r128-{_dt}-{_ord}"] = _case(128, 16, dtype=_dt, order=_ord)
for _ord in ("cand", "shared"):
    CASES[f"r32-{_ord}"] = _case(32, 16, order=_ord)
CASES["b12"] = _case(128, 12)
CASES["b5"] = _case(128, 5, dtype="float32")
CASES["mb2"] = _case(65, 32, C=17, mb=2)
CASES["mb4"] = _case(33, 64, C=17, mb=4, wpe=2)
CASES["alphas"] = _case(128, 16, alphas=True)
CASES["k3"] = _case(128, 16, K=3, env=ONE, groups=1)
IDS = [f"{name}-nt{nt}" for name in CASES for nt in (0, 1)]


def confs_of(K):
    """Two cells each; over the population every tap of both modalities is read, as a first and as a second cell."""
    return [np.array([[k % 4, (k + 1) % 4, k % 2], [(k + 2) % 4, (3 * k + 3) % 4, (k + 1) % 2]]) for k in range(K)]


def run_case(name, nt, dev):
    """-> {"planes": [[sha W, sha m, sha v] per candidate], "stats": sha, "status": sha, "record": launch record}"""
    import torch
    from mfas_amd import FeatureTable, Hyper, Population
    c = CASES[name]
    assert not any(s in os.environ for s in SWITCHES)
    R, B, K = c["R"], c["B"], c["K"]
    N = FULL * B + (5 if B > 5 else 3)
    nb = -(-N // B)
    per = c["order"] != "shared"
    hp = Hyper(R=R, C=c["C"], B=B, bn=True, drpt=0.5, alphas=c["alphas"], order_per_candidate=per, s_sizes=S_SIZES, v_sizes=V_SIZES)
    dtype = getattr(torch, c["dtype"])
    tr = FeatureTable.from_numpy(O.synth_table(N, 3, snr=0.6, C=c["C"], s_sizes=S_SIZES, v_sizes=V_SIZES), dev, dtype)
    dv = FeatureTable.from_numpy(O.synth_table(N_DEV, 4, snr=0.6, C=c["C"], s_sizes=S_SIZES, v_sizes=V_SIZES), dev, dtype)
    etas = O.eta_sequence(1e-3, 1e-6, 1, 2, N / B, EPOCHS * nb)
    rng = np.random.default_rng(5)
    perm = lambda: np.stack([rng.permutation(N) for _ in range(EPOCHS)])  # noqa: E731
    order = torch.from_numpy((np.stack([perm() for _ in range(K)]) if per else perm()).astype(np.int32)).to(dev)
    env = dict(c["env"], MFAS_NT=str(nt))
    if c["order"] == "nogather":
        env["MFAS_NO_GATHER"] = "1"
    os.environ.update(env)
    try:
        pop = Population(hp, confs_of(K), dev, drop_seeds=list(range(70, 70 + K)), chunk_cols=CHUNK)
        try:
            sched = pop.schedule()
            assert not sched["persistent"] and not sched["wide"] and not sched["lean_chain"] and sched["groups"] == c["groups"], sched
            pop.init(list(range(1, K + 1)))
            stats, status = pop.train(tr, dv, EPOCHS, etas, order=order, snapshot_best=True)
            sha = lambda b: hashlib.sha256(b).hexdigest()  # noqa: E731
            out = {"planes": [[sha(pop.get_params(k, pl).cpu().numpy().tobytes()) for pl in range(3)] for k in range(K)],
                   "stats": sha(np.ascontiguousarray(stats).tobytes()), "status": sha(np.ascontiguousarray(status).tobytes()),
                   "record": pop.launch_record()}
        finally:
            pop.close()
    finally:
        for key in env:
            os.environ.pop(key, None)
    assert not status.any(), (name, nt, status)
    return out


def target_build(name, nt):
    """The k_step build whose sweep units the case is there for: the launches without a chain (the prologue, a two-group epoch's last
    launch, a one-group plan's sweeps) take the 128-register build of the batch-tile count; four batch tiles have the one build."""
    c = CASES[name]
    return f"k_step<{c['mb']},{nt},{c['wpe']},0,1>"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("cid", IDS)
def test_sweep_prologue_bit_identical(dev, golden, cid):
    name, nt = cid.rsplit("-nt", 1)
    got = run_case(name, int(nt), dev)
    want = golden[cid]
    assert target_build(name, int(nt)) in got["record"], (cid, got["record"])
    assert got["record"] == want["record"], (cid, got["record"], want["record"])
    assert got["status"] == want["status"] and got["stats"] == want["stats"], (cid, "status words / statistics")
    for k, (g, w) in enumerate(zip(got["planes"], want["planes"])):
        assert g == w, (cid, "candidate %d: W / m / v differ in plane(s) %s" % (k, [i for i in range(3) if g[i] != w[i]]))
    assert len(got["planes"]) == len(want["planes"])


def record():
    import torch
    from mfas_amd import _lib
    dev = torch.device("cuda:0")
    cases, bad = {}, 0
    for cid in IDS:
        name, nt = cid.rsplit("-nt", 1)
        try:
            cases[cid] = run_case(name, int(nt), dev)
        except AssertionError as e:      # (a schedule the case does not expect: say so and go on, nothing has run)
            print(f"{cid:32s} REFUSED {e}", flush=True)
            bad += 1
            continue
        ok =target_build(name, int(nt)) in cases[cid]["record"]
        bad += not ok
        print(f"{cid:32s} {cases[cid]['planes'][0][0][:16]} {cases[cid]['record']}{'' if ok else '   <- lacks ' + target_build(name, int(nt))}", flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"recorded_with": _lib.lib().mfas_source_digest().decode(), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {GOLDEN}; {bad} lack their target build")
    return 3 if bad else 0


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python -m tests.test_gpu_sweep_prologue --record   (MFAS_LIB = the library to record)"
    sys.exit(record())
