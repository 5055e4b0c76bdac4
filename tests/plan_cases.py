"""The inputs, the dump plumbing and the pins of tests/test_plan_cpu.py, moved here unchanged so that tests/test_lds_cpu.py can read the same
plans: a test module is imported by nobody (tests/test_host_cpu.py::test_nothing_imports_a_test_module)."""
import functools
import os

import numpy as np

from oracle import np_oracle as O
from tests import builds_header as BH
from tests import devmem_header as DH
from tests import plan_header as PH
from tests import axes_cases as AX
from tests import ref64_cases as G
from tests import resident_cases as GR
from tests import wide_cases as GW
from tests import step_build_cases as SB
from tests import wide_plans as TW
from tests.helpers import CONFS, engine_hyper

GRID_SEED = 20261
N_GRID = 320
# every slot of both modalities used: widths that are no multiple of 16, one beyond 4096, one that pads to an odd number of tiles
W_88 = dict(s=(1, 16, 9, 15, 17, 63, 65, 1000), v=(8, 2048, 40, 256, 33, 600, 4100, 129))
SWITCHES = [{"MFAS_PERSIST": "0"}, {"MFAS_NO_LEAN_CHAIN": "1"}, {"MFAS_GROUPS": "1"}, {"MFAS_GROUPS": "2"}, {"MFAS_SAME_GROUP": "0"},
            {"MFAS_SAME_GROUP": "2"}, {"MFAS_NO_TAP_MAJOR": "1"}, {"MFAS_FORCE_TAP_MAJOR": "1"}, {"MFAS_NO_RED_IN_SWEEP": "1"},
            {"MFAS_OCC_BYTES": "0"}, {"MFAS_OCC_BYTES": "3e8"}, {"MFAS_NO_XCD_PLACEMENT": "1"}, {"MFAS_XCDS": "4"}, {"MFAS_NT": "0"},
            {"MFAS_NT": "1"}, {"MFAS_CHAIN_SPLIT": "0"}]
PAIRS = [{"MFAS_PERSIST": "0", "MFAS_GROUPS": "2"}, {"MFAS_SAME_GROUP": "0", "MFAS_GROUPS": "2"}, {"MFAS_SAME_GROUP": "2", "MFAS_CHAIN_SPLIT": "0"},
         {"MFAS_PERSIST": "0", "MFAS_FORCE_TAP_MAJOR": "1"}, {"MFAS_XCDS": "4", "MFAS_NO_TAP_MAJOR": "1"}, {"MFAS_GROUPS": "2", "MFAS_NT": "1"},
         {"MFAS_NO_LEAN_CHAIN": "1", "MFAS_PERSIST": "0"}, {"MFAS_SAME_GROUP": "0", "MFAS_NO_RED_IN_SWEEP": "1"}]


def _case(cid, hp, confs, cc=0, n_cus=256, persist=True, env=None, seeds=None):
    hp = engine_hyper(hp) if isinstance(hp, O.Hyper) else hp
    return dict(id=cid, hp=hp, confs=[np.asarray(c, np.int32).reshape(-1, 3) for c in confs], cc=cc, n_cus=n_cus, persist=persist,
                env=dict(env or {}), seeds=seeds)


def _suite_cases():
    """What the suite already holds: G.CASES, GW.WIDE_CASES, SB.SWEEP_FORMS and the natural populations, the resident rows, the
    populations of test_axes_cpu, the baseline geometries."""
    out = [_case("ref64-" + c[0], G.case_hyper(c), [c[5]]) for c in G.CASES]
    out += [_case("wide-" + c[0], G.case_hyper(GW.base_case(c)), GW.case_confs(c)) for c in GW.WIDE_CASES]
    for row in list(SB.SWEEP_FORMS) + list(SB.NATURAL.values()) + [SB.natural_sibling(SB.NATURAL["natural_nt"])]:
        fl = set(filter(None, row["flags"].split(",")))
        hp = engine_hyper(G.case_hyper((row["id"], row["R"], row["C"], row["B"], row["widths"], None, "bn" in fl, 0.5, "")))
        mode = row.get("order_mode") or SB.row_order_mode(row["id"])
        hp.order_per_candidate = mode == "per_candidate"
        sib = "-sibling" if row["id"] == "natural_nt" and len(row["confs"][-1]) == 3 else ""
        out.append(_case("forms-" + row["id"] + sib, hp, row["confs"], row["cc"], env=row["env"]))
    for row in GR.RESIDENT_BUILDS:
        hp = engine_hyper(G.case_hyper(GR.base_case(row)))
        hp.tap_bits = row[8]
        hp.order_per_candidate = GR.row_order_mode(row[0]) == "per_candidate"
        out.append(_case("resident-" + row[0], hp, row[5][:row[10]], row[9]))
    for spec in AX.POPS:
        inp = AX.pop_inputs(spec)
        entry = AX.pop_entry(spec[1])
        out.append(_case("axes-" + spec[0], inp["ehp"], inp["confs"], entry[4], env=entry[3], seeds=inp["seeds"]))
    out += [_case("axes-" + c[0], G.case_hyper(c), [c[5]]) for c in AX.TAP_CASES]
    out += [_case("baseline-" + name, hp, confs) for name, hp, confs in TW.baseline_geometries()]
    return out


def big_cells(n):
    """n cells of W_C's two widest taps (s2048 + v4100): 128 x 6160 padded columns each."""
    return [SB.BIG + [i % 3] for i in range(n)]


STATE_EDGE = {"under": (4, 4, 3, 2), "over": (4, 4, 3, 3)}     # cells per candidate at R = 128 over the two widest taps of W_C


def state_stream_bytes(R, C, widths, confs):
    """plan.hip.h: what the same-group launch compares with 260 MB — 24 bytes per PADDED weight of every segment and head."""
    Rp, Cp = GW.ceil16(R), GW.ceil16(C)
    return 24.0 * sum(Rp * (GW.ceil16(widths["s"][c[0]]) + GW.ceil16(widths["v"][c[1]]) + (Rp if i else 0)) for conf in confs
                      for i, c in enumerate(conf)) + 24.0 * Cp * Rp * len(confs)


def _edge_cases():
    out = []
    c4, l2 = CONFS["c4"], CONFS["l2"]
    depth = [CONFS["l1"], l2, CONFS["l3"], c4]
    for K in (7, 8, 27, 28, 39, 40, 223, 224, 64, 65):
        for R in (16, 128):
            out.append(_case(f"edge-K{K}-R{R}", O.Hyper(R=R, C=60, B=16, bn=False, drpt=0.5), [depth[k % 4] for k in range(K)]))
        out.append(_case(f"edge-K{K}-R128-two", O.Hyper(R=128, C=60, B=16, bn=False, drpt=0.5), [depth[k % 4] for k in range(K)],
                         env={"MFAS_SAME_GROUP": "0"}))
    for R in (16, 17, 112, 113, 128, 129):
        for K in (3, 12):
            out.append(_case(f"edge-R{R}-K{K}", O.Hyper(R=R, C=60, B=16, bn=True, drpt=0.5), [depth[(k + 1) % 4] for k in range(K)]))
    for B in (16, 17, 32, 33, 48, 64, 65):
        for R in (16, 64, 128):
            out.append(_case(f"edge-B{B}-R{R}", O.Hyper(R=R, C=23, B=B, bn=True, drpt=0.5, alphas=R == 64), [l2, c4, CONFS["l3"]]))
    for bits in (0, 16):
        for cc in (0, 1024):
            hp = engine_hyper(O.Hyper(R=16, C=60, B=20, bn=True, drpt=0.5, s_sizes=GR.W_R["s"], v_sizes=GR.W_R["v"]))
            hp.tap_bits = bits
            out.append(_case(f"edge-tapbits{bits}-cc{cc}", hp, GR.POP_W, cc))
    for side, cells in STATE_EDGE.items():
        out.append(_case(f"edge-state260-{side}", G.case_hyper(("", 128, 60, 16, G.W_C, None, False, 0.5, "")), [big_cells(n) for n in cells]))
    small = [[[0, 0, 0]]] * 20          # W_A: one 16- and one 32-column unit per candidate
    for n_cus in (8, 64, 256, 304):
        out.append(_case(f"edge-rechunk-cus{n_cus}", G.case_hyper(("", 16, 60, 20, G.W_A, None, True, 0.5, "")), small, n_cus=n_cus))
        out.append(_case(f"edge-c4x6-cus{n_cus}", O.Hyper(R=16, C=60, B=20, bn=False, drpt=0.5), [c4] * 6, n_cus=n_cus))
        out.append(_case(f"edge-c4x6-cus{n_cus}-nopersist", O.Hyper(R=16, C=60, B=20, bn=False, drpt=0.5), [c4] * 6, n_cus=n_cus, persist=False))
    # 20 one-cell candidates of s1024 + v2048: 12 units of 256 columns each, 6 of 512 — one unit per workgroup does not fit 256 CUs at 256
    # columns, and both two 256-column units per workgroup and one 512-column unit do: the order of plan_chunk's options decides
    out.append(_case("edge-two-256-before-one-512", O.Hyper(R=16, C=60, B=16, bn=False, drpt=0.5), [[[2, 2, 0]]] * 20))
    # the largest geometry the library accepts (one dev-pass tile per workgroup) and large ones short of it
    out.append(_case("edge-largest", O.Hyper(R=512, C=256, B=128, bn=True, drpt=0.5), [l2]))
    out.append(_case("edge-r512-c256-b16", O.Hyper(R=512, C=256, B=16, bn=True, drpt=0.5), [l2, c4]))
    out.append(_case("edge-r400-c200-b64", O.Hyper(R=400, C=200, B=64, bn=False, drpt=0.5), [c4]))
    base = [("sw-r16", O.Hyper(R=16, C=60, B=20, bn=True, drpt=0.5), [c4] * 5, 256),
            ("sw-r16k48", O.Hyper(R=16, C=60, B=20, bn=False, drpt=0.5), [depth[k % 4] for k in range(48)], 64),
            ("sw-r32", O.Hyper(R=32, C=17, B=20, bn=True, drpt=0.5), [depth[k % 4] for k in range(40)], 256),
            ("sw-r128", O.Hyper(R=128, C=60, B=16, bn=False, drpt=0.5), [depth[k % 4] for k in range(12)], 256),
            ("sw-r128b20", O.Hyper(R=128, C=60, B=20, bn=True, drpt=0.5, alphas=True), [depth[k % 4] for k in range(20)], 304)]
    for name, hp, confs, n_cus in base:
        for env in [{}] + SWITCHES + PAIRS:
            tag = "+".join(f"{k[5:]}={v}" for k, v in env.items()) or "none"
            out.append(_case(f"{name}-{tag}", hp, confs, n_cus=n_cus, env=env))
    return out


def _grid_cases():
    from mfas_amd.mmimdb_searchable import MM_IMAGE_SIZES, MM_TEXT_SIZES
    rng = np.random.default_rng(GRID_SEED)
    wsets = [("88", W_88), ("53", AX.W_AV), ("mm", dict(s=MM_TEXT_SIZES, v=MM_IMAGE_SIZES))]
    out = []
    for n in range(N_GRID):
        wname, w = wsets[n % 3]
        R = int(rng.choice([1, 8, 11, 16, 17, 32, 33, 64, 65, 80, 112, 113, 128, 129, 177, 256, 300, 512]))
        C = int(rng.choice([1, 2, 17, 23, 60, 64, 65, 128, 200]))
        B = int(rng.choice([2, 7, 16, 17, 20, 32, 33, 48, 64, 65, 100, 128]))
        K = int(rng.choice([1, 2, 3, 5, 7, 8, 11, 16, 20, 27, 28, 33, 40, 64, 100, 230]))
        if wname == "88" and R >= 64:
            K = min(K, 40)              # (keeps the largest dumps to a few MB of text)
        confs = [[[int(rng.integers(len(w["s"]))), int(rng.integers(len(w["v"]))), int(rng.integers(3))] for _ in range(1 + (k + n) % 4)]
                 for k in range(K)]
        if n < 8:                       # every slot of the 8 + 8 set in the first candidates, whatever the draw
            confs[0] = [[(n + i) % len(w["s"]), (n + 2 * i) % len(w["v"]), i % 3] for i in range(4)]
        hp = engine_hyper(O.Hyper(R=R, C=C, B=B, bn=bool(rng.integers(2)), drpt=0.5, alphas=bool(rng.integers(4) == 0),
                                  multitask=bool(rng.integers(5) == 0), s_sizes=w["s"], v_sizes=w["v"]))
        hp.tap_bits = int(rng.choice([0, 16, 32]))
        hp.order_per_candidate = bool(rng.integers(4) == 0)
        env = {} if rng.integers(2) else dict((SWITCHES + PAIRS)[int(rng.integers(len(SWITCHES) + len(PAIRS)))])
        seeds = [int(x) for x in rng.integers(0, 2 ** 32, K)] if rng.integers(2) else None
        out.append(_case(f"grid-{n:03d}-{wname}", hp, confs, int(rng.choice([0, 0, 0, 64, 128, 256, 512, 1024, 100])),
                         int(rng.choice([8, 64, 256, 304])), bool(rng.integers(5)), env, seeds))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = _suite_cases() + _edge_cases() + _grid_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


# ------------------------------------------------------------------------------------------------ the dump
def hooks_lib():
    """What dump() asks: the g++ program of tests/plan_header.py.  (The name is from when the dump was an export of the test-hooks
    library; the test bodies below, which the pins were recorded with, still call it.)"""
    return PH.program()


def fnv64(text):
    h = 1469598103934665603
    for b in text.encode():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def dump(lib, case, mode=0):
    """The plan dump of a case under the case's switches and no other (tests/plan_header.py sets the program's environment)."""
    assert lib == PH.program()
    return PH.dumps([case], mode)[0][0]


def parse(text):
    """mode-0 text -> (scalars {name: string}, {section: record count})."""
    scal, counts = {}, {}
    for line in text.splitlines():
        if line.startswith("["):
            counts[line[1:line.index("]")]] = int(line.split("records=")[1].split()[0])
        else:
            name, _, val = line.strip().partition("=")
            scal[name] = val
    return scal, counts


@functools.lru_cache(maxsize=None)
def all_dumps():
    return dict(zip((c["id"] for c in all_cases()), PH.dumps(all_cases())[0]))


# ------------------------------------------------------------------------------------------------ the pins
# FNV-1a of the mode-0 dump of every case, recorded from a build of the parent commit with only the dump added (profiles/plan_stages.log)
PINNED = {
    "ref64-r1a": "f50c5c789c5c8901", "ref64-r1b": "ec885880b1029b26", "ref64-r16a": "ef36b418abc4393a", "ref64-r16b": "82cde56cdc29bfd2",
    "ref64-r17a": "aafb71fd07131c47", "ref64-r17b": "490366b5f4df326e", "ref64-r32a": "6394fd21012d8502", "ref64-r32b": "e9778415e583306a",
    "ref64-r33a": "0dbd058c174c8e04", "ref64-r33b": "f454f6d8ef578e3f", "ref64-r65a": "3894f989d2b679d7", "ref64-r65b": "45702dd3ccdb5faa",
    "ref64-r80a": "767a33dde37f3bdc", "ref64-r80b": "5cdb5dc479a3832e", "ref64-r128a": "47402bb9d3939a7b", "ref64-r128b": "bdbfa074ce1b0e49",
    "ref64-r129a": "69ec487edb0b7258", "ref64-r129b": "de9ca98730289706", "ref64-r256a": "31de917c237d4753", "ref64-r256b": "afd60dca6191b1d7",
    "ref64-r257a": "3ffd792b9729aa3f", "ref64-r257b": "2a7b09c423b75a18", "ref64-r300": "f941a0b920a1cbe5", "ref64-r320a": "4507203fca1bf1f8",
    "ref64-r320b": "efcc8940583ddd9d", "ref64-r448a": "552be9212140ac00", "ref64-r448b": "02c584db7a8192bd", "ref64-r449a": "e0087864a0730adc",
    "ref64-r449b": "05393859725cb1e2", "ref64-r512a": "eabb54847ff84c37", "ref64-r512b": "76decb21cc55c8ff", "wide-w65": "53dad8f04b1e3157",
    "wide-w80": "202ca4b68afb177a", "wide-w177": "4eb53cc8480f1b1d", "wide-w256": "e9427760d0e75f33", "wide-w512a": "bedfa230a787f3de",
    "wide-w512b": "b7fead38af7fd8d7", "wide-wc": "df2a92ee673387e1", "wide-wb65": "a899e96e3056dad0", "wide-wb100": "cc65986eaee254fc",
    "wide-wb128": "c0c358b99816c3b2", "forms-step-mb1": "b01c39d3d2eac1d6", "forms-step-split": "7535ad3b4a213f7c",
    "forms-step-mb2-w2": "fba508e78ae4d42e", "forms-step-mb2-w4-chain": "9358cc8f3d51ca18", "forms-step-mb4": "80581b2e06d82850",
    "forms-lean-mb1": "3903ebbdbe33cafa", "forms-lean-mb2": "8191df43e6d852ed", "forms-same-mb1": "5b8395da4d0ecfcd",
    "forms-same-mb2": "525f63cba64ad2e6", "forms-same-split": "042692b65103cbce", "forms-wide": "96f00d984239bec3",
    "forms-natural_nt": "328017e12479a9eb", "forms-natural_occ": "1552db67e0bcb93f", "forms-natural_nt-sibling": "56690ebd47a8afb4",
    "resident-mb1-plain0-f32-nu1": "3521c525c63b6995", "resident-mb1-plain0-f32-nu2": "3d48f00a8cce0a2e",
    "resident-mb1-plain0-x16-nu1": "bef683beb0f3e1de", "resident-mb1-plain0-x16-nu2": "546b9e6a6f293042",
    "resident-mb1-plain0-x16-wide": "50b5594bccc7468f", "resident-mb1-plain1-f32-nu1": "57e76bd94a9107df",
    "resident-mb1-plain1-f32-nu2": "a8d069ad9efae8f3", "resident-mb1-plain1-x16-nu1": "565651fc2e5fd859",
    "resident-mb1-plain1-x16-nu2": "1a1e2758f1ef3fe7", "resident-mb1-plain1-x16-wide": "a3f15c0e006b81f7",
    "resident-mb1-plain2-f32-nu1": "257fdcbfa1c01232", "resident-mb1-plain2-f32-nu2": "8b57cc86204ae71e",
    "resident-mb1-plain2-x16-nu1": "9a6fde26908bcc38", "resident-mb1-plain2-x16-nu2": "50b392f7cb252b71",
    "resident-mb1-plain2-x16-wide": "217a5d436c1bbcc6", "resident-mb2-plain0-f32-nu1": "54cf0a72190dad3f",
    "resident-mb2-plain0-f32-nu2": "098b863f463afc13", "resident-mb2-plain0-x16-nu1": "8fb20fe63315dabd",
    "resident-mb2-plain0-x16-nu2": "59c4439b6f3ded4e", "resident-mb2-plain0-x16-wide": "79ea05538e59a2c1",
    "resident-mb2-plain1-f32-nu1": "2da251017ea45dc7", "resident-mb2-plain1-f32-nu2": "cf09c3a3da5c6313",
    "resident-mb2-plain1-x16-nu1": "a2afa31c6ab040d5", "resident-mb2-plain1-x16-nu2": "0202aa8fb331f1a4",
    "resident-mb2-plain1-x16-wide": "18da102965adc8f8", "resident-mb2-plain2-f32-nu1": "90ed67752b35e299",
    "resident-mb2-plain2-f32-nu2": "6a5f36efc7a436de", "resident-mb2-plain2-x16-nu1": "61f1c0ad85826b3d",
    "resident-mb2-plain2-x16-nu2": "a2a2867e4f6a692a", "resident-mb2-plain2-x16-wide": "78dae172d8ed89c5",
    "axes-tap-lean_chain-shared": "67fb62c196b2e7f0", "axes-tap-lean_chain-per_candidate": "016797fb341ff10c",
    "axes-tap-general_mb1-shared": "035844c23d862811", "axes-tap-general_mb1-per_candidate": "035844c23d862811",
    "axes-tap-general_mb2-shared": "29137ca259f9e309", "axes-tap-general_mb2-per_candidate": "29137ca259f9e309",
    "axes-tap-general_mb4-shared": "6b47c7084dd147ab", "axes-tap-general_mb4-per_candidate": "6b47c7084dd147ab",
    "axes-tap-same_group-shared": "0a0eee8f3b6b626a", "axes-tap-same_group-per_candidate": "0a0eee8f3b6b626a",
    "axes-tap-chain_split-shared": "55df0fb8186e399c", "axes-tap-chain_split-per_candidate": "55df0fb8186e399c",
    "axes-tap-persistent-shared": "7b86c81461e9f243", "axes-tap-persistent-per_candidate": "7b86c81461e9f243",
    "axes-tap-two_group_ab-shared": "8798734859370156", "axes-tap-two_group_ab-per_candidate": "1373cfd392272d1a",
    "axes-tap-tap_major-shared": "0aa6a3cbf65333c1", "axes-tap-tap_major-per_candidate": "c85533e2be449e44",
    "axes-tap-wide_b65-shared": "c09e84c77b1af297", "axes-plain-lean_chain": "b09283942a7b51c2", "axes-plain-general_mb1": "bfe403bc96d99d72",
    "axes-plain-general_mb2": "4cfb10f8e384f40a", "axes-plain-general_mb4": "e7455864d65bbff3", "axes-plain-same_group": "d837031d7b1cc480",
    "axes-plain-chain_split": "e24eb730cfcb1fd8", "axes-plain-persistent": "373d9969c63c4d3a", "axes-plain-two_group_ab": "99ba26b6938bdc90",
    "axes-plain-wide_b65": "93d115b707281ef5", "axes-sa-lean_chain-shared": "0c99025484a6dc52", "axes-sa-general_mb1-shared": "bc9e5dda843c6069",
    "axes-sa-general_mb2-shared": "a1ca6aee0476aa4f", "axes-sa-general_mb4-shared": "a448882cca26aedd",
    "axes-sa-same_group-shared": "2d01f2ebf2a038c3", "axes-sa-chain_split-shared": "a71d6568669b2a99",
    "axes-sa-persistent-shared": "b3e5ccb847a32242", "axes-sa-two_group_ab-shared": "a321735728beff2f",
    "axes-sa-tap_major-shared": "7971504ea109e31f", "axes-sa-wide_b65-shared": "ebddbde4f0865260",
    "axes-sa-two_group_ab-per_candidate": "a321735728beff2f", "axes-sa-persistent-per_candidate": "b3e5ccb847a32242",
    "axes-sb-lean_chain-shared": "914e0629c77114f7", "axes-sb-general_mb1-shared": "4f010d5075c8095c",
    "axes-sb-general_mb2-shared": "1f8d048bf735076f", "axes-sb-general_mb4-shared": "e162ebbb9580f017",
    "axes-sb-same_group-shared": "72465916d5dd1412", "axes-sb-chain_split-shared": "fb180bd76e085772",
    "axes-sb-persistent-shared": "d11e1289246fa4eb", "axes-sb-two_group_ab-shared": "32aac39cbd1401cc",
    "axes-sb-tap_major-shared": "1ead51a9a4bef9cc", "axes-sb-wide_b65-shared": "1448fe95ff8dac05",
    "axes-sb-two_group_ab-per_candidate": "32aac39cbd1401cc", "axes-sb-persistent-per_candidate": "d11e1289246fa4eb",
    "axes-sc-lean_chain-shared": "646e2e28f9b57396", "axes-sc-general_mb1-shared": "52afa63d97962970",
    "axes-sc-general_mb2-shared": "e46aab7e017e64f0", "axes-sc-general_mb4-shared": "5bfc76ef80d7d991",
    "axes-sc-same_group-shared": "161557cd17ab0063", "axes-sc-chain_split-shared": "87b550fe69143e39",
    "axes-sc-persistent-shared": "9c8c57a50c51e97d", "axes-sc-two_group_ab-shared": "5605d74f5fa6c525",
    "axes-sc-tap_major-shared": "9184a440da8dc08a", "axes-sc-wide_b65-shared": "83af279e5f497ef2",
    "axes-sc-two_group_ab-per_candidate": "5605d74f5fa6c525", "axes-sc-persistent-per_candidate": "9c8c57a50c51e97d",
    "axes-sd-lean_chain-shared": "e42bf5084272e1c9", "axes-sd-general_mb1-shared": "e2db0a93d4cb73eb",
    "axes-sd-general_mb2-shared": "977b174315090831", "axes-sd-general_mb4-shared": "f6b71e1934aa225d",
    "axes-sd-same_group-shared": "2a766c1eab4cfdd9", "axes-sd-chain_split-shared": "600aad41fa927d79",
    "axes-sd-persistent-shared": "064a49fa6a0b513a", "axes-sd-two_group_ab-shared": "7438ea6e4ef41e57",
    "axes-sd-tap_major-shared": "0b0bacb161b09c10", "axes-sd-wide_b65-shared": "a5891818fbd40571",
    "axes-sd-two_group_ab-per_candidate": "7438ea6e4ef41e57", "axes-sd-persistent-per_candidate": "064a49fa6a0b513a", "axes-t8a": "b94cda13cd81eb8c",
    "axes-t8b": "922c76979f957162", "axes-t8c": "cd980e0354db8275", "axes-t8d": "80730566ed61fadc", "axes-t8w": "40b30084ec2f6367",
    "axes-tav_a": "193ec6a0d06ad2a5", "axes-tav_b": "10cc21f78bba61e3", "axes-t26a": "3941bef60c518d5e", "axes-t26b": "1d6a09086a1e4103",
    "axes-t26c": "cebb5b3b1f528579", "baseline-r16_b20_k1": "b55f6414c87e1270", "baseline-r128_b16_k1": "5c6242b2392cb01d",
    "baseline-mmimdb_k1": "1c2ffb7b75139611", "baseline-r16_b20_k16": "4daed5301cc08300", "baseline-r128_b16_k16": "eeacc7f9f26f2d1e",
    "baseline-mmimdb_k16": "5d57198be3654249", "baseline-r16_b20_k64": "653ef2eec4a888ea", "baseline-r128_b16_k64": "1a70f0df801b126f",
    "baseline-mmimdb_k64": "3af12b8abbaaedc8", "edge-K7-R16": "13a9a6d087494280", "edge-K7-R128": "a93276d8478d98c0",
    "edge-K7-R128-two": "2fbf7ffee73fd81d", "edge-K8-R16": "45cdf9403fbec244", "edge-K8-R128": "347e60925362c4c5",
    "edge-K8-R128-two": "80c8082ed3498a6c", "edge-K27-R16": "b32356f3860a6be9", "edge-K27-R128": "325547467f878fc2",
    "edge-K27-R128-two": "325547467f878fc2", "edge-K28-R16": "17492aa402bf7e69", "edge-K28-R128": "e4b2ec65b4a4e782",
    "edge-K28-R128-two": "e4b2ec65b4a4e782", "edge-K39-R16": "bb23b9096b1c8a6a", "edge-K39-R128": "32e5e7612b7203c7",
    "edge-K39-R128-two": "32e5e7612b7203c7", "edge-K40-R16": "89b7dbb1fa36768e", "edge-K40-R128": "467b8e68b75e6a3a",
    "edge-K40-R128-two": "467b8e68b75e6a3a", "edge-K223-R16": "60c9f4070adf5e45", "edge-K223-R128": "4b2113b49f034a9f",
    "edge-K223-R128-two": "4b2113b49f034a9f", "edge-K224-R16": "e79b482b08925f08", "edge-K224-R128": "9efc1934c514f664",
    "edge-K224-R128-two": "9efc1934c514f664", "edge-K64-R16": "d4825a0860d8047f", "edge-K64-R128": "e40ebe3af6b59fb2",
    "edge-K64-R128-two": "e40ebe3af6b59fb2", "edge-K65-R16": "6f2663eba7212611", "edge-K65-R128": "dfa7c996fd8df39d",
    "edge-K65-R128-two": "dfa7c996fd8df39d", "edge-R16-K3": "f3a08c5c87a10989", "edge-R16-K12": "a449f8d809071bbd", "edge-R17-K3": "95cc560ce018271c",
    "edge-R17-K12": "c72430fe84408d85", "edge-R112-K3": "28800845bc92c631", "edge-R112-K12": "049f85cdd3c71835", "edge-R113-K3": "4bcacb908a1ffc00",
    "edge-R113-K12": "9540e78546b9b52f", "edge-R128-K3": "bf8bf6d88974c2e9", "edge-R128-K12": "5d51220f0a6b8fce", "edge-R129-K3": "bdfe808afd520841",
    "edge-R129-K12": "59f31874970a62d0", "edge-B16-R16": "75b09a7515a5b619", "edge-B16-R64": "3d71577734716bc2", "edge-B16-R128": "5108949ca2f2c003",
    "edge-B17-R16": "d5b5af1b762ce17d", "edge-B17-R64": "328d84464a3b2df2", "edge-B17-R128": "24681b4609817d47", "edge-B32-R16": "11e867ab66d7c775",
    "edge-B32-R64": "2262f2ccb937f2b0", "edge-B32-R128": "ab223c6bdc4c4f0b", "edge-B33-R16": "1f04bd7f98afdcc8", "edge-B33-R64": "dc6cafe29c49f060",
    "edge-B33-R128": "76432259baec25d3", "edge-B48-R16": "ca8f8fc8bb597427", "edge-B48-R64": "aa0bfb263293e663", "edge-B48-R128": "1b4f4dd5560dbca7",
    "edge-B64-R16": "6e731ee5c5b39959", "edge-B64-R64": "0e7ffe87ef8053cc", "edge-B64-R128": "6b790a5772c6f52a", "edge-B65-R16": "2d9d12f8ce7dc381",
    "edge-B65-R64": "0f86315fcd526683", "edge-B65-R128": "cc7ff8c5aca29468", "edge-tapbits0-cc0": "9d0ad456158c7bbf",
    "edge-tapbits0-cc1024": "761929601df3cb1c", "edge-tapbits16-cc0": "4578537686ae13c6", "edge-tapbits16-cc1024": "3db2ee4502977aba",
    "edge-state260-under": "d2b72eacb20ab583", "edge-state260-over": "0434459d59fcbb96", "edge-rechunk-cus8": "13638b5882754d39",
    "edge-c4x6-cus8": "ee9c3cf2ef25152e", "edge-c4x6-cus8-nopersist": "ee9c3cf2ef25152e", "edge-rechunk-cus64": "6286d34b075faaaa",
    "edge-c4x6-cus64": "f0f89c75b51393fd", "edge-c4x6-cus64-nopersist": "f0f89c75b51393fd", "edge-rechunk-cus256": "b9f00046d5065110",
    "edge-c4x6-cus256": "1a97ef78a758e281", "edge-c4x6-cus256-nopersist": "79577add4981815f", "edge-rechunk-cus304": "a16b341c2d608c59",
    "edge-c4x6-cus304": "6dc617c78f79e391", "edge-c4x6-cus304-nopersist": "178071dadba2471b", "edge-two-256-before-one-512": "2cce0bec695aa25b",
    "edge-largest": "aaf51b2199015755", "edge-r512-c256-b16": "325b3896d79f3716", "edge-r400-c200-b64": "8b59eeff0524d12e",
    "sw-r16-none": "780923396118116a", "sw-r16-PERSIST=0": "79b89d526e3e4565", "sw-r16-NO_LEAN_CHAIN=1": "509d9669913227e3",
    "sw-r16-GROUPS=1": "780923396118116a", "sw-r16-GROUPS=2": "780923396118116a", "sw-r16-SAME_GROUP=0": "780923396118116a",
    "sw-r16-SAME_GROUP=2": "780923396118116a", "sw-r16-NO_TAP_MAJOR=1": "780923396118116a", "sw-r16-FORCE_TAP_MAJOR=1": "780923396118116a",
    "sw-r16-NO_RED_IN_SWEEP=1": "780923396118116a", "sw-r16-OCC_BYTES=0": "aed70460cf46da95", "sw-r16-OCC_BYTES=3e8": "b7a6f2b8738525c4",
    "sw-r16-NO_XCD_PLACEMENT=1": "f0893339e3fe9462", "sw-r16-XCDS=4": "ff069240e134e4e9", "sw-r16-NT=0": "780923396118116a",
    "sw-r16-NT=1": "1ec9165be180ffbb", "sw-r16-CHAIN_SPLIT=0": "780923396118116a", "sw-r16-PERSIST=0+GROUPS=2": "fc75f8e24225c91e",
    "sw-r16-SAME_GROUP=0+GROUPS=2": "780923396118116a", "sw-r16-SAME_GROUP=2+CHAIN_SPLIT=0": "780923396118116a",
    "sw-r16-PERSIST=0+FORCE_TAP_MAJOR=1": "85759098d1677b1f", "sw-r16-XCDS=4+NO_TAP_MAJOR=1": "ff069240e134e4e9",
    "sw-r16-GROUPS=2+NT=1": "1ec9165be180ffbb", "sw-r16-NO_LEAN_CHAIN=1+PERSIST=0": "509d9669913227e3",
    "sw-r16-SAME_GROUP=0+NO_RED_IN_SWEEP=1": "780923396118116a", "sw-r16k48-none": "82339fa94d751a44", "sw-r16k48-PERSIST=0": "82339fa94d751a44",
    "sw-r16k48-NO_LEAN_CHAIN=1": "2bfd40c1afb6aa85", "sw-r16k48-GROUPS=1": "78b3aadd48fe627f", "sw-r16k48-GROUPS=2": "82339fa94d751a44",
    "sw-r16k48-SAME_GROUP=0": "82339fa94d751a44", "sw-r16k48-SAME_GROUP=2": "82339fa94d751a44", "sw-r16k48-NO_TAP_MAJOR=1": "82339fa94d751a44",
    "sw-r16k48-FORCE_TAP_MAJOR=1": "e976d075380dc3ec", "sw-r16k48-NO_RED_IN_SWEEP=1": "82339fa94d751a44", "sw-r16k48-OCC_BYTES=0": "05c3f63c53b33f68",
    "sw-r16k48-OCC_BYTES=3e8": "2dfa21735ee4b763", "sw-r16k48-NO_XCD_PLACEMENT=1": "82339fa94d751a44", "sw-r16k48-XCDS=4": "82339fa94d751a44",
    "sw-r16k48-NT=0": "82339fa94d751a44", "sw-r16k48-NT=1": "ed26aec9823e0cf5", "sw-r16k48-CHAIN_SPLIT=0": "82339fa94d751a44",
    "sw-r16k48-PERSIST=0+GROUPS=2": "82339fa94d751a44", "sw-r16k48-SAME_GROUP=0+GROUPS=2": "82339fa94d751a44",
    "sw-r16k48-SAME_GROUP=2+CHAIN_SPLIT=0": "82339fa94d751a44", "sw-r16k48-PERSIST=0+FORCE_TAP_MAJOR=1": "e976d075380dc3ec",
    "sw-r16k48-XCDS=4+NO_TAP_MAJOR=1": "82339fa94d751a44", "sw-r16k48-GROUPS=2+NT=1": "ed26aec9823e0cf5",
    "sw-r16k48-NO_LEAN_CHAIN=1+PERSIST=0": "2bfd40c1afb6aa85", "sw-r16k48-SAME_GROUP=0+NO_RED_IN_SWEEP=1": "82339fa94d751a44",
    "sw-r32-none": "4ac144020f83f792", "sw-r32-PERSIST=0": "4ac144020f83f792", "sw-r32-NO_LEAN_CHAIN=1": "4ac144020f83f792",
    "sw-r32-GROUPS=1": "4ac144020f83f792", "sw-r32-GROUPS=2": "22577fa35ac50e86", "sw-r32-SAME_GROUP=0": "22577fa35ac50e86",
    "sw-r32-SAME_GROUP=2": "4ac144020f83f792", "sw-r32-NO_TAP_MAJOR=1": "4ac144020f83f792", "sw-r32-FORCE_TAP_MAJOR=1": "4ac144020f83f792",
    "sw-r32-NO_RED_IN_SWEEP=1": "4ac144020f83f792", "sw-r32-OCC_BYTES=0": "8fbc9c65170bee8f", "sw-r32-OCC_BYTES=3e8": "897a15b76b33e483",
    "sw-r32-NO_XCD_PLACEMENT=1": "4ac144020f83f792", "sw-r32-XCDS=4": "4ac144020f83f792", "sw-r32-NT=0": "4ac144020f83f792",
    "sw-r32-NT=1": "8ee60247e03c2f7a", "sw-r32-CHAIN_SPLIT=0": "4ac144020f83f792", "sw-r32-PERSIST=0+GROUPS=2": "22577fa35ac50e86",
    "sw-r32-SAME_GROUP=0+GROUPS=2": "22577fa35ac50e86", "sw-r32-SAME_GROUP=2+CHAIN_SPLIT=0": "4ac144020f83f792",
    "sw-r32-PERSIST=0+FORCE_TAP_MAJOR=1": "4ac144020f83f792", "sw-r32-XCDS=4+NO_TAP_MAJOR=1": "4ac144020f83f792",
    "sw-r32-GROUPS=2+NT=1": "978deeafa6957557", "sw-r32-NO_LEAN_CHAIN=1+PERSIST=0": "4ac144020f83f792",
    "sw-r32-SAME_GROUP=0+NO_RED_IN_SWEEP=1": "22577fa35ac50e86", "sw-r128-none": "97bda8719d26fcb4", "sw-r128-PERSIST=0": "97bda8719d26fcb4",
    "sw-r128-NO_LEAN_CHAIN=1": "97bda8719d26fcb4", "sw-r128-GROUPS=1": "97bda8719d26fcb4", "sw-r128-GROUPS=2": "13bc2969418e7590",
    "sw-r128-SAME_GROUP=0": "13bc2969418e7590", "sw-r128-SAME_GROUP=2": "97bda8719d26fcb4", "sw-r128-NO_TAP_MAJOR=1": "97bda8719d26fcb4",
    "sw-r128-FORCE_TAP_MAJOR=1": "97bda8719d26fcb4", "sw-r128-NO_RED_IN_SWEEP=1": "97bda8719d26fcb4", "sw-r128-OCC_BYTES=0": "a678d8ffcbafd6f3",
    "sw-r128-OCC_BYTES=3e8": "3c05543616903ae1", "sw-r128-NO_XCD_PLACEMENT=1": "97bda8719d26fcb4", "sw-r128-XCDS=4": "97bda8719d26fcb4",
    "sw-r128-NT=0": "97bda8719d26fcb4", "sw-r128-NT=1": "8c5e176db0322f7c", "sw-r128-CHAIN_SPLIT=0": "22e2fc608fc28568",
    "sw-r128-PERSIST=0+GROUPS=2": "13bc2969418e7590", "sw-r128-SAME_GROUP=0+GROUPS=2": "13bc2969418e7590",
    "sw-r128-SAME_GROUP=2+CHAIN_SPLIT=0": "22e2fc608fc28568", "sw-r128-PERSIST=0+FORCE_TAP_MAJOR=1": "97bda8719d26fcb4",
    "sw-r128-XCDS=4+NO_TAP_MAJOR=1": "97bda8719d26fcb4", "sw-r128-GROUPS=2+NT=1": "be43d0b04a7b289d",
    "sw-r128-NO_LEAN_CHAIN=1+PERSIST=0": "97bda8719d26fcb4", "sw-r128-SAME_GROUP=0+NO_RED_IN_SWEEP=1": "bf91d96325fcb9f7",
    "sw-r128b20-none": "ad7850b42f0e9f74", "sw-r128b20-PERSIST=0": "ad7850b42f0e9f74", "sw-r128b20-NO_LEAN_CHAIN=1": "ad7850b42f0e9f74",
    "sw-r128b20-GROUPS=1": "d693ae509ebe0b13", "sw-r128b20-GROUPS=2": "ad7850b42f0e9f74", "sw-r128b20-SAME_GROUP=0": "ad7850b42f0e9f74",
    "sw-r128b20-SAME_GROUP=2": "5454d457fa6e447a", "sw-r128b20-NO_TAP_MAJOR=1": "ad7850b42f0e9f74",
    "sw-r128b20-FORCE_TAP_MAJOR=1": "ad7850b42f0e9f74", "sw-r128b20-NO_RED_IN_SWEEP=1": "b795f23c5c71ba17",
    "sw-r128b20-OCC_BYTES=0": "d9e62c03d53daf2e", "sw-r128b20-OCC_BYTES=3e8": "e8dde8f859b7b658", "sw-r128b20-NO_XCD_PLACEMENT=1": "ad7850b42f0e9f74",
    "sw-r128b20-XCDS=4": "ad7850b42f0e9f74", "sw-r128b20-NT=0": "ad7850b42f0e9f74", "sw-r128b20-NT=1": "cb57cc0e2ae1e1cc",
    "sw-r128b20-CHAIN_SPLIT=0": "ad7850b42f0e9f74", "sw-r128b20-PERSIST=0+GROUPS=2": "ad7850b42f0e9f74",
    "sw-r128b20-SAME_GROUP=0+GROUPS=2": "ad7850b42f0e9f74", "sw-r128b20-SAME_GROUP=2+CHAIN_SPLIT=0": "5454d457fa6e447a",
    "sw-r128b20-PERSIST=0+FORCE_TAP_MAJOR=1": "ad7850b42f0e9f74", "sw-r128b20-XCDS=4+NO_TAP_MAJOR=1": "ad7850b42f0e9f74",
    "sw-r128b20-GROUPS=2+NT=1": "cb57cc0e2ae1e1cc", "sw-r128b20-NO_LEAN_CHAIN=1+PERSIST=0": "ad7850b42f0e9f74",
    "sw-r128b20-SAME_GROUP=0+NO_RED_IN_SWEEP=1": "b795f23c5c71ba17", "grid-000-88": "59361f7f0877ef12", "grid-001-53": "eac2e9c095a7410d",
    "grid-002-mm": "b35c5efc0b5a1fca", "grid-003-88": "d563c249cac9ddbb", "grid-004-53": "f9618181e263f40c", "grid-005-mm": "fd2ace1a02a3d64c",
    "grid-006-88": "74bffa259964b0eb", "grid-007-53": "7b6ccafe9503d410", "grid-008-mm": "dbed1b3f88f951d1", "grid-009-88": "80ca642d6e4c4e75",
    "grid-010-53": "bbded67966862f03", "grid-011-mm": "8fc6459a934c11e4", "grid-012-88": "d5c0611cfeb10a94", "grid-013-53": "a084a3fdea31892c",
    "grid-014-mm": "1141f8615d43f519", "grid-015-88": "93759ada0c0f72d5", "grid-016-53": "8c8ed1eb9680435c", "grid-017-mm": "a1165974fca0fdfe",
    "grid-018-88": "f774ba16d77c3e5b", "grid-019-53": "9f6f933a51d93cfd", "grid-020-mm": "aa70e9446ca212b8", "grid-021-88": "95574c38edecc996",
    "grid-022-53": "960e98b6c9c3c824", "grid-023-mm": "81ac4bc182bc6d00", "grid-024-88": "b54cbf550498bd9f", "grid-025-53": "c865a0c3238d3e16",
    "grid-026-mm": "2a9a5b516a6fb2c9", "grid-027-88": "b43e98153c6c36ad", "grid-028-53": "5a453d8024c7fd2c", "grid-029-mm": "d006230f3d236d74",
    "grid-030-88": "d2622cd655f18cb6", "grid-031-53": "15d8a88f062cf67c", "grid-032-mm": "3bcb239cf12c7dc9", "grid-033-88": "391036aa2b740459",
    "grid-034-53": "aad299a69b8e8cfa", "grid-035-mm": "a83e678fc9e548e1", "grid-036-88": "0d062c74d4ac1fd2", "grid-037-53": "3954104f136a8acc",
    "grid-038-mm": "558a7b5279164e9a", "grid-039-88": "174c93d853fbd9a8", "grid-040-53": "05ffee936f1a89d0", "grid-041-mm": "8e81d0ffa9df469d",
    "grid-042-88": "4b69a64141a573c5", "grid-043-53": "261378a80ab72c72", "grid-044-mm": "625276257fa22675", "grid-045-88": "ba4f4ea80045c9ad",
    "grid-046-53": "7839845d0b63ea03", "grid-047-mm": "b9237f417f90dad2", "grid-048-88": "86c2bffc82f20292", "grid-049-53": "722bfeaa0d5be205",
    "grid-050-mm": "a2eae392c8e6da6b", "grid-051-88": "7783901c46553af3", "grid-052-53": "4f0f9042fc81873a", "grid-053-mm": "07d86676e727dc72",
    "grid-054-88": "5abc1886613ad6fb", "grid-055-53": "ccee52c1af466563", "grid-056-mm": "8e68e6029205b9f1", "grid-057-88": "15c78a0e25203378",
    "grid-058-53": "3ca918686fc8d412", "grid-059-mm": "85d1298d3a082bb1", "grid-060-88": "346c9b7c619efad7", "grid-061-53": "1a54acb259139d1e",
    "grid-062-mm": "0bb55c0aeb87f234", "grid-063-88": "de9b18a286743da3", "grid-064-53": "7b18b315a416c0ca", "grid-065-mm": "6bb89b0c4f56b41d",
    "grid-066-88": "dc25fb6388d4b0da", "grid-067-53": "5de752b8eca8cc9a", "grid-068-mm": "cc0fee9dfe71dbc4", "grid-069-88": "74ba8ecf95d61fc7",
    "grid-070-53": "cc3c3ec845b4a00c", "grid-071-mm": "53f47fd21272eda7", "grid-072-88": "126ad8141e8a69e1", "grid-073-53": "69badf61207ec2da",
    "grid-074-mm": "a7968e8127e62c81", "grid-075-88": "c79fc69364b44f86", "grid-076-53": "c6601f45f9b065df", "grid-077-mm": "abc45e1de4f7af49",
    "grid-078-88": "f2064487a88e9aa4", "grid-079-53": "2d5413128472b38f", "grid-080-mm": "3b4bff3e16244a07", "grid-081-88": "74dfec11b8d32bf7",
    "grid-082-53": "1fb361e48e6aea74", "grid-083-mm": "186fc1c312473a64", "grid-084-88": "c06423dac7844837", "grid-085-53": "2264a1eefe0eec19",
    "grid-086-mm": "c11c7a43a00a05ff", "grid-087-88": "a20c595480e1bf45", "grid-088-53": "4b3440d33aa4996e", "grid-089-mm": "0147eea1494644ad",
    "grid-090-88": "a79c422e1a49a5ba", "grid-091-53": "ba01bc66c523efcb", "grid-092-mm": "136cdac1fe64815a", "grid-093-88": "db4f48bbfe685e12",
    "grid-094-53": "01fd9141a226cc1a", "grid-095-mm": "31c9caa6497e7aff", "grid-096-88": "b59658b7bdd63df7", "grid-097-53": "75d0c99df53fb58e",
    "grid-098-mm": "08d7561e19b2731d", "grid-099-88": "6b24430bf64065f7", "grid-100-53": "86895c8c089e8a88", "grid-101-mm": "313c752ed95737e5",
    "grid-102-88": "131ee1bd668befe4", "grid-103-53": "c7bb612dc6d804dc", "grid-104-mm": "d7a059ede501d152", "grid-105-88": "e9b8be0c8b2e6de6",
    "grid-106-53": "f0753b878fc0f04f", "grid-107-mm": "1a7068c73e2d0d15", "grid-108-88": "8bdeb9822bf57979", "grid-109-53": "b4caf4ba4f034c37",
    "grid-110-mm": "5a287a310c128a0e", "grid-111-88": "a359b508a9414075", "grid-112-53": "a05527f78f0b7ea9", "grid-113-mm": "c1c1fd6326b0d62e",
    "grid-114-88": "bf08ab0f060f0f4b", "grid-115-53": "7e8ff466e23be71f", "grid-116-mm": "f1eaf0ec46d4bde8", "grid-117-88": "c042606906906e42",
    "grid-118-53": "5665c40c006c624e", "grid-119-mm": "2886618d7b1e8aad", "grid-120-88": "475422683bf34499", "grid-121-53": "b4f89ccaa577f19e",
    "grid-122-mm": "55d3c913c2607046", "grid-123-88": "d49d6f98c851d58c", "grid-124-53": "6f46bd0e9ebf7a69", "grid-125-mm": "6c02b0b6a98f8db2",
    "grid-126-88": "501cfe3acd04f6a4", "grid-127-53": "7b49c55e32e470ab", "grid-128-mm": "2a55a4744f1f0cca", "grid-129-88": "2b92c633fc78b857",
    "grid-130-53": "5b94a6ff772f7a0e", "grid-131-mm": "e1b0ebe431a40546", "grid-132-88": "81d7ce7533b6dc25", "grid-133-53": "9f669792241cd7d4",
    "grid-134-mm": "c5ded772759cb9d1", "grid-135-88": "d45303326d1cde5d", "grid-136-53": "1ab2713a9ab5f2de", "grid-137-mm": "9d2de5e7f4eb2527",
    "grid-138-88": "7e0d1d436f9437d1", "grid-139-53": "e143ec742965848f", "grid-140-mm": "36ad06cfc99fa99a", "grid-141-88": "dcb84acbc0c11c43",
    "grid-142-53": "27cdc4fda61bdadc", "grid-143-mm": "5498b187e3d4191a", "grid-144-88": "e08b8e75e9b9b533", "grid-145-53": "ecd29d4ded012501",
    "grid-146-mm": "1b3b87f352bae23d", "grid-147-88": "404c936c930f539a", "grid-148-53": "10b81cc0946d2be9", "grid-149-mm": "f7f4b8e7334ea7e4",
    "grid-150-88": "0221e507eb6f6b39", "grid-151-53": "cf27952a72376c60", "grid-152-mm": "18ae885ca5f12e6e", "grid-153-88": "6dd86a5b98e70152",
    "grid-154-53": "495392666bdc7ad4", "grid-155-mm": "2cbcf82a7c8e1e5e", "grid-156-88": "14c0eab9249a615c", "grid-157-53": "33d680f6fc638d75",
    "grid-158-mm": "4114a5c7160c4594", "grid-159-88": "480631fecda4fb65", "grid-160-53": "60b5d73b1b37033d", "grid-161-mm": "b20bf78e3565ff5f",
    "grid-162-88": "7f352172df5af5bc", "grid-163-53": "c9f275a96080f8f1", "grid-164-mm": "3d7384303973f837", "grid-165-88": "a5f47e3077d9632c",
    "grid-166-53": "4e052f35ff107a8a", "grid-167-mm": "8b8246d57357e47d", "grid-168-88": "ba4c6aac0bfe54e5", "grid-169-53": "393de5aaa67adffe",
    "grid-170-mm": "cb5b3b1984f4a38e", "grid-171-88": "6084dad1cebde9a1", "grid-172-53": "aa4d152ee0781532", "grid-173-mm": "0301b4611c373679",
    "grid-174-88": "4e8156ddd3d845dd", "grid-175-53": "0a6bc762208bee8e", "grid-176-mm": "bc51a76e26b2bfc6", "grid-177-88": "6c2e50649b2fd898",
    "grid-178-53": "ed727df9aa0970ba", "grid-179-mm": "a9d8d1aed0f2861f", "grid-180-88": "43037549a26861ab", "grid-181-53": "81867d310b6c6f3d",
    "grid-182-mm": "d58f7bc5abbd7699", "grid-183-88": "1fb7f02d24ab0857", "grid-184-53": "c08a7187811b0ccc", "grid-185-mm": "02c1e7048e32da0d",
    "grid-186-88": "e7a2e7a769ab4103", "grid-187-53": "8ca128f6f779855f", "grid-188-mm": "c442f5ea78c63ac8", "grid-189-88": "b60b741e2316c644",
    "grid-190-53": "97ec64dab51a2629", "grid-191-mm": "b9f4685e80685b9c", "grid-192-88": "6c6401fa7d05fdc4", "grid-193-53": "ddd13c32ddecb692",
    "grid-194-mm": "e65ae8f2969d6d68", "grid-195-88": "2fd4ab154a4badd3", "grid-196-53": "7a4aba4405d8bdb3", "grid-197-mm": "728148d120af5be2",
    "grid-198-88": "02d71a0442cef5c3", "grid-199-53": "7a6d401d73580a1d", "grid-200-mm": "4281ef2400de4530", "grid-201-88": "aef1899af4034e9a",
    "grid-202-53": "139a854028c90bbd", "grid-203-mm": "e32c9be777805e1a", "grid-204-88": "b5be6e54bc1cbd6a", "grid-205-53": "944bb0e9c4c43420",
    "grid-206-mm": "02191354295cf122", "grid-207-88": "230808036c985ea9", "grid-208-53": "cf958b485a1c5e9c", "grid-209-mm": "6a63a7ea5f16f8b2",
    "grid-210-88": "e79870dcb8ccebc9", "grid-211-53": "e9498b9086475c5a", "grid-212-mm": "be8ed24d3ae39fbe", "grid-213-88": "6aadf95e0ec6838a",
    "grid-214-53": "3de5d2d44f0ae4e5", "grid-215-mm": "1f3c2a4b497e8a1b", "grid-216-88": "e90768a9f0e38f08", "grid-217-53": "ce4ca0c67f3ba42c",
    "grid-218-mm": "77fe9150cc0b3cca", "grid-219-88": "eef892e1f06c87f9", "grid-220-53": "b2db4235d26352a0", "grid-221-mm": "532a62c217e83d9d",
    "grid-222-88": "763288cf1bd45eff", "grid-223-53": "a7cbe1ff68a9c33d", "grid-224-mm": "2b02537f858915d1", "grid-225-88": "8518bfcabc3f8c98",
    "grid-226-53": "cc57748212c3c000", "grid-227-mm": "59d296a6872a5531", "grid-228-88": "541d8675426f969f", "grid-229-53": "5e5e95e5913a7bc2",
    "grid-230-mm": "d0c4d0e74d6d720e", "grid-231-88": "2d223215c8f71821", "grid-232-53": "636ae530135819eb", "grid-233-mm": "d6bba4c7b34ecdc3",
    "grid-234-88": "d31689f752100893", "grid-235-53": "66352faaeb74ab19", "grid-236-mm": "e99c09e8abb1cdd1", "grid-237-88": "276f16fb0efb6d01",
    "grid-238-53": "cc03af6a43bff41f", "grid-239-mm": "b2cb4994cb4be80f", "grid-240-88": "b37f1e365a9f01a3", "grid-241-53": "1e0dbe090cdb464c",
    "grid-242-mm": "13197c5347083dac", "grid-243-88": "ab3683c875252bab", "grid-244-53": "11999fdd2d4da2c9", "grid-245-mm": "5a585fe4cec26dc9",
    "grid-246-88": "2aa6b9ad5f11d7f1", "grid-247-53": "ea178e1f00d95970", "grid-248-mm": "689426ec0909cf09", "grid-249-88": "dd22840bce534cc0",
    "grid-250-53": "f24c81feaf8726ca", "grid-251-mm": "10e898f60a8b535c", "grid-252-88": "c481d8851073f23e", "grid-253-53": "f780c518f659c5b3",
    "grid-254-mm": "cfedca41e36a383d", "grid-255-88": "04eda012a3a6e482", "grid-256-53": "379a50e99990c2d8", "grid-257-mm": "bff13b06bb3958c2",
    "grid-258-88": "2c3808c9f7bdcac3", "grid-259-53": "aa3a705e8a633a9b", "grid-260-mm": "a3681363618f46c0", "grid-261-88": "bfed1450a9006b96",
    "grid-262-53": "c65c37e242ab02ee", "grid-263-mm": "0029699732b94605", "grid-264-88": "b4e26f094303bb70", "grid-265-53": "567ca66c509611f7",
    "grid-266-mm": "a90d0fa53b2ed92f", "grid-267-88": "f8efe4409a7a5f32", "grid-268-53": "542e70d599abf0ce", "grid-269-mm": "0fd4d67ef6c26cec",
    "grid-270-88": "363cbdb6dbe3e473", "grid-271-53": "abc2d0017c1785e5", "grid-272-mm": "fa885ad9cbe18acb", "grid-273-88": "39fce731ae82481f",
    "grid-274-53": "87cd51ae305f9ce0", "grid-275-mm": "c5e10041e2cd8ffb", "grid-276-88": "d1b2eaa74143d2ca", "grid-277-53": "563069c82bc3cd91",
    "grid-278-mm": "784e6287e181b391", "grid-279-88": "b244ef421bc07a48", "grid-280-53": "64d6567d8e104e87", "grid-281-mm": "a8f485e9e1b6b7a8",
    "grid-282-88": "05320bdf0fd7c0e7", "grid-283-53": "c3e406e0b8feee5c", "grid-284-mm": "ec2af9cb40095f3b", "grid-285-88": "b9b7122f84a54b9f",
    "grid-286-53": "7196e515d6c97f07", "grid-287-mm": "9f2e53b97922c39a", "grid-288-88": "8718a334dc940d7d", "grid-289-53": "2880de6a2e2fa243",
    "grid-290-mm": "15231cfeed93f407", "grid-291-88": "c47831677c1b2056", "grid-292-53": "7214443d99a01c5e", "grid-293-mm": "90637935cdc99f61",
    "grid-294-88": "d35b3f873874c0b8", "grid-295-53": "c34396dae5683385", "grid-296-mm": "dd9684d07191f1a3", "grid-297-88": "512bc657d5cdd82b",
    "grid-298-53": "460af22c2a25220c", "grid-299-mm": "ca0ca185fee96055", "grid-300-88": "626102ae5512db6e", "grid-301-53": "db84560a3795d4df",
    "grid-302-mm": "0e0d0ec361ba9447", "grid-303-88": "978fae71759d3e20", "grid-304-53": "6475b208442d2551", "grid-305-mm": "684daf21a5093ac8",
    "grid-306-88": "fdf49306cf09d161", "grid-307-53": "1eba2627874d7bba", "grid-308-mm": "1648c6f6d356f954", "grid-309-88": "0b3764db9fc1bf65",
    "grid-310-53": "f94055d8f006ec6c", "grid-311-mm": "cabe5c0221cc0609", "grid-312-88": "451e0642a6240140", "grid-313-53": "2e54115ac51858fd",
    "grid-314-mm": "3beb5168e861ce30", "grid-315-88": "b8ea0fb845e4a122", "grid-316-53": "1610e297faed9f20", "grid-317-mm": "316b7bdb5faa1fab",
    "grid-318-88": "30a7f30420fd563b", "grid-319-53": "e243da367f769c1e",
}
