"""The whole layout plan, pinned on the CPU (plan.hip.h: plan_layout, compiled by g++ alone with tests/plan_dump.h: tests/plan_header.py).

mfas_population_plan answers eight integers; every kernel reads the rest — descriptor lists, offsets, the group split, tap units, the
unit order of the same-group launch, the role table, LDS budgets, the step-buffer layout.  Here the dump of the complete plan is
compared, case by case, with what a build of the commit BEFORE plan_layout was cut into stages gave (mode 0: the scalars in clear, of
every other section its record count and the FNV-1a digest of its text; PINNED holds the FNV-1a of that whole answer, the record run
with every section's digest is profiles/plan_stages.log).  A moved digest is a changed plan: mode 1 of the case is what one diffs.

The inputs are what the suite already trains (by import) plus the edges of every threshold the planner has, every switch, and a seeded
grid; the test itself asserts that they reach every value of every boolean or enumerated field, that every pinned plan's PlanFacts
name builds the tables hold (builds.hip.h), and that the six values test_wide_cpu.py pins are the dump's."""
import os

import pytest

from tests import builds_header as BH
from tests import devmem_header as DH
from tests import plan_header as PH
from tests import ref64_cases as G
from tests import wide_cases as GW
from tests import step_build_cases as SB
from tests import wide_plans as TW
from tests.plan_cases import PINNED, STATE_EDGE, all_cases, all_dumps, big_cells, dump, fnv64, hooks_lib, parse, state_stream_bytes


# ------------------------------------------------------------------------------------------------ the tests
def test_every_plan_is_the_pinned_one():
    got = {cid: fnv64(text) for cid, text in all_dumps().items()}
    assert set(got) == set(PINNED)
    moved = [cid for cid in got if got[cid] != PINNED[cid]]
    assert not moved, (len(moved), moved[:20], all_dumps()[moved[0]])


def test_mode_one_is_the_text_the_digests_are_of():
    """Mode 1 of a few plans: the same headers as mode 0, every digest the FNV-1a of the section's lines, every count their number."""
    lib = hooks_lib()
    for cid in ("baseline-r128_b16_k16", "baseline-r16_b20_k16", "wide-wb100", "forms-same-split"):
        case = next(c for c in all_cases() if c["id"] == cid)
        full, heads, body = dump(lib, case, 1).splitlines(keepends=True), [], {}
        for line in full:
            if line.startswith("["):
                heads.append(line)
                body[line] = []
            else:
                body[heads[-1]].append(line)
        assert [h for h in all_dumps()[cid].splitlines(keepends=True) if h.startswith("[")] == heads
        for h in heads:
            assert f"records={len(body[h])} fnv={fnv64(''.join(body[h]))}" in h, (cid, h)
        assert len(heads) >= 14 and sum(len(b) for b in body.values()) > 100


def test_the_pinned_cases_reach_every_value():
    """Conditions on the inputs, so that the pin cannot be empty: every boolean or enumerated plan field takes each of its values."""
    seen, taps, roles = {}, set(), set()
    for c in all_cases():
        s, n = parse(all_dumps()[c["id"]])
        for k in ("persist", "res_chain", "res_wide", "res_nu", "wide", "lean_chain", "same_group", "chain_split", "red_in_sweep", "nontemporal",
                  "defer", "yf_in_lds", "vec_in_lds", "fits_lds", "groups", "nrbw", "mbe"):
            seen.setdefault(k, set()).add(int(s[k]))
        assert (int(s["defer"]) == 1) == (int(s["sb_dy_alt"]) > 0), c["id"]
        tap_major_conditions = (not int(s["wide"]) and int(s["nrb"]) in (1, 2, 4) and not int(s["persist"]) and not int(s["same_group"])
                                and "MFAS_NO_TAP_MAJOR" not in c["env"] and not c["hp"].order_per_candidate)
        if tap_major_conditions:
            taps.add(n["group0.taps"] > 0)
        else:
            assert all(n[f"group{g}.taps"] == 0 for g in range(int(s["groups"]))), c["id"]
        if int(s["persist"]):
            roles.add(n["role"] > 0)
            assert n["pdescs"] == int(s["nres"]) > 0 and n["need"] == int(s["K"]), c["id"]
        else:
            assert n["role"] == n["pdescs"] == n["need"] == 0, c["id"]
        assert n["cands"] == n["nparams"] == n["cand_plane_base"] == n["cand_plane_size"] == n["desc_start"] - 1 == int(s["K"]), c["id"]
        assert n["wide_start"] == (int(s["K"]) + 1 if int(s["wide"]) else 0), c["id"]
    # fits_lds: plan_layout answers the wide plan wherever the batch-resident one does not fit, and the wide kernels' budgets fit at the
    # largest R, C and B validate_inputs lets through ("edge-largest"), so no accepted input gives 0
    two = {0, 1}
    want = dict(persist=two, res_chain=two, res_wide=two, res_nu={1, 2}, wide=two, lean_chain=two, same_group=two, chain_split={0, 4},
                red_in_sweep=two, nontemporal=two, defer=two, yf_in_lds=two, vec_in_lds=two, fits_lds={1}, groups={1, 2}, nrbw={1, 2, 4, 8},
                mbe={1, 2, 4})
    assert seen == want, {k: (seen[k], want[k]) for k in want if seen[k] != want[k]}
    assert taps == {True, False} and roles == {True, False}


def test_the_edges_lie_on_both_sides():
    """The thresholds the edge cases are named after, computed from the inputs: 260 MB of state, 200 MiB of planes, a resident plan
    that does not stand."""
    d = {cid: parse(text)[0] for cid, text in all_dumps().items()}
    sizes = {side: state_stream_bytes(128, 60, G.W_C, [big_cells(n) for n in cells]) for side, cells in STATE_EDGE.items()}
    assert sizes["under"] <= 260e6 < sizes["over"], sizes
    assert d["edge-state260-under"]["same_group"] == "1" and d["edge-state260-over"]["same_group"] == "0"
    nt, sib = SB.NATURAL["natural_nt"], SB.natural_sibling(SB.NATURAL["natural_nt"])
    planes = [12.0 * SB.plane_floats(r["R"], r["C"], r["widths"], r["confs"]) for r in (sib, nt)]
    assert planes[0] <= SB.NT_BYTES < planes[1]
    assert d["forms-natural_nt"]["nontemporal"] == "1" and d["forms-natural_nt-sibling"]["nontemporal"] == "0"
    assert int(d["forms-natural_nt"]["plane_stride"]) * 12.0 == planes[1]
    assert 20 + 12 * 20 > 256 >= 20 + 6 * 20
    assert [d["edge-two-256-before-one-512"][k] for k in ("persist", "chunk", "res_nu", "nres")] == ["1", "256", "2", "240"]
    # 20 candidates of two units each: 60 resident workgroups fit 64 CUs, but 20 chains are more than a quarter of them — the units
    # chosen for the resident schedule (256 columns) give way to the launch-per-phase chunk; with 256 CUs the same population is resident
    assert 20 + 2 * 20 <= 64 and 20 > 64 // 4
    assert (d["edge-rechunk-cus256"]["persist"], d["edge-rechunk-cus256"]["chunk"]) == ("1", "256")
    assert (d["edge-rechunk-cus64"]["persist"], d["edge-rechunk-cus64"]["res_chain"]) == ("0", "0") and d["edge-rechunk-cus64"]["chunk"] != "256"


def test_every_pinned_plan_names_builds_the_tables_hold():
    """The dump's PlanFacts through the compiled builds.hip.h: a non-empty key list, every key a row of the kernel tables."""
    facts = sorted({parse(t)[0]["facts"] for t in all_dumps().values()})
    assert len(facts) >= 20
    queries = [("plan", dict(zip(BH.FIELDS, map(int, f.split(","))))) for f in facts]
    rows = set(BH.ask1("tables", None))
    for f, keys in zip(facts, BH.ask(queries)):
        assert keys and set(keys) <= rows, (f, keys)


def test_the_plan_query_pins_are_the_dumps():
    """The six values test_wide_cpu.py pins (mfas_population_plan on a device-less host: 256 compute units) are the same fields here."""
    d = {cid: parse(text)[0] for cid, text in all_dumps().items()}
    six = lambda s: tuple(int(s[k]) for k in ("persist", "nres", "nres_wg", "res_nu", "chunk", "lean_chain"))  # noqa: E731
    for cid, want in TW.PINNED_CASES.items():
        assert six(d["ref64-" + cid]) == want and d["ref64-" + cid]["wide"] == "0", cid
    for cid, want in TW.PINNED_BASELINE.items():
        assert six(d["baseline-" + cid]) == want and d["baseline-" + cid]["wide"] == "0", cid
    for cid in GW.WIDE_IDS:
        assert d["wide-" + cid]["wide"] == "1", cid


def test_the_planner_that_ships_answers_what_the_pinned_one_does():
    """The pins are of plan.hip.h as g++ compiles it; the library holds it as clang does.  Every pinned case the product library's
    mfas_population_plan can be asked — 256 compute units (what the query assumes without a device, and what an MI355X has), the
    resident schedule allowed — under its switches: persistent, resident units and workgroups, units per workgroup, chunk, lean, wide
    and K are the dump's scalars."""
    from mfas_amd.engine import plan_population
    asked = [c for c in all_cases() if c["n_cus"] == 256 and c["persist"]]
    assert len(asked) >= 300 and len({tuple(sorted(c["env"].items())) for c in asked}) >= 20
    outer = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("MFAS_")}
    try:
        for c in asked:
            os.environ.update(c["env"])
            try:
                plan = plan_population(c["hp"], c["confs"], "cuda:0", c["cc"])
            finally:
                for k in c["env"]:
                    os.environ.pop(k, None)
            assert plan["compute_units"] == 256, plan
            s = parse(all_dumps()[c["id"]])[0]
            want = dict(persistent=s["persist"], resident_units=s["nres"], resident_workgroups=s["nres_wg"], units_per_workgroup=s["res_nu"],
                        chunk_cols=s["chunk"], lean_chain=s["lean_chain"], wide=s["wide"], candidates=s["K"])
            assert {k: int(plan[k]) for k in want} == {k: int(v) for k, v in want.items()}, (c["id"], plan, want)
    finally:
        os.environ.update(outer)


def test_the_planner_under_address_and_undefined_sanitizers():
    """The same program built with -fsanitize=address,undefined -fno-sanitize-recover=all and run directly — a stand-alone executable,
    no sanitizer runtime is preloaded into anything — over ALL cases (some 30 s in all, the build included: profiles/plan_header.log):
    it ends clean, reports nothing, and every plan is still the pinned one."""
    why = DH.sanitizer_missing()
    if why:
        pytest.skip(why)
    texts, err = PH.dumps(all_cases(), flags=PH.SANITIZE)
    assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
    moved = [c["id"] for c, t in zip(all_cases(), texts) if fnv64(t) != PINNED[c["id"]]]
    assert len(texts) == len(PINNED) and not moved, (len(moved), moved[:20])


@pytest.mark.parametrize("what,mutation", [
    ("pick_chunk: a chunk that does not divide the padded columns", ("if (cols_p % c == 0) best = c;", "best = c;")),
    ("balanced_split: the first group stops one candidate late at an exact half", ("if (run >= tot / 2) break;", "if (run > tot / 2) break;")),
], ids=["pick_chunk", "balanced_split"])
def test_a_wrong_planner_moves_pinned_digests(what, mutation):
    """plan.hip.h with one piece of text replaced, over the same cases: pinned digests move, and the message a failure of
    test_every_plan_is_the_pinned_one would carry names the cases."""
    texts = PH.dumps(all_cases(), mutation=mutation)[0]
    moved = [c["id"] for c, t in zip(all_cases(), texts) if fnv64(t) != PINNED[c["id"]]]
    assert moved, what
    message = repr((len(moved), moved[:20], texts[[c["id"] for c in all_cases()].index(moved[0])]))
    assert moved[0] in message and all(m in PINNED for m in moved)
