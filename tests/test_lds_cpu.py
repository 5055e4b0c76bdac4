"""The LDS layouts of mfas_amd/csrc/lds.hip.h, on the CPU (through the g++ program of tests/lds_header.py).

A budget a few floats short is no test failure on the GPU: LDS is granted in granules, an overrun of that size lands inside the grant
or in the CU's other workgroup.  Here every layout a plan can ask for — k_sweep_wide's, the one layout in that header, over the geometries of all
plan cases (tests/test_plan_cpu.py) — is printed area by area and checked: ascending, disjoint but for the declared aliases, aliases
inside what they name, everything under `total`, every buffer 16-byte aligned, and `total * 4` the budget the plan dump shows for the
schedule that uses the layout.  A mutation test shows that the planner has no statement of THIS layout of its own.  The other
kernel bodies (chain_split, chain_body, chain_lean, sweep_body, k_president's units, k_chain_wide, k_eval) still walk their LDS against a formula of
the planner's, and nothing here checks those: DESIGN.md section 8."""
import functools
import re

import pytest

from tests import devmem_header as DH
from tests import lds_header as LH
from tests import plan_header as PH
from tests import plan_cases as T

LDS_BYTES = 160 * 1024
WIDE_UNIT = 128      # records.hip.h: 16 * WIDE_KB columns, 16 * WIDE_RBG rows of a wide unit


@functools.lru_cache(maxsize=None)
def plans():
    """{case id: (scalars, layout chunks as a set of (cc, rows_p), wide units as a set of (sub_nkb, rows_p))} of every plan case: the
    scalars from the mode-0 dumps the plan tests share; from the mode-1 dump of the wide cases the chunks, which a wide plan's budget is
    a maximum over, and the units of its work list, whose sub_nkb * 16 columns and rows_p rows are what k_sweep_wide asks its layout with."""
    scal = {cid: T.parse(text)[0] for cid, text in T.all_dumps().items()}
    wide = [c for c in T.all_cases() if int(scal[c["id"]]["wide"])]
    seg, unit, chunks, units = re.compile(r" cc=(\d+) rows_p=(\d+) "), re.compile(r" rows_p=(\d+) .* sub_nkb=(\d+)"), {}, {}

    def section(text, name):
        body = text[text.index("[" + name + "]"):]
        return body[body.index("\n") + 1:body.index("[", 1)].splitlines()
    for c, text in zip(wide, PH.dumps(wide, 1)[0]):
        chunks[c["id"]] = {tuple(map(int, seg.search(line).groups())) for line in section(text, "descs")}
        units[c["id"]] = {tuple(map(int, unit.search(line).groups()))[::-1] for line in section(text, "group0.descs")}
    return {cid: (s, chunks.get(cid, set()), units.get(cid, set())) for cid, s in scal.items()}


def case_queries(cid):
    """The layout queries of case `cid`: (what the planner asks for a wide plan's chunks, what k_sweep_wide asks for the units of the
    plan's work list)."""
    s, chunks, units = plans()[cid]
    wide = [("widesweep", min(WIDE_UNIT, cc), min(WIDE_UNIT, rows)) for cc, rows in sorted(chunks)] if int(s["wide"]) else []
    return wide, [("widesweep", nkb * 16, rows) for nkb, rows in sorted(units)]


@functools.lru_cache(maxsize=None)
def answers(flags=()):
    """({query: (areas, total)} over every query of every case, each asked once, and the loop words; stderr of the run)."""
    qs = {("words",), ("scratch",)}
    for cid in plans():
        wide, kernel = case_queries(cid)
        qs.update(wide + kernel)
    qs = sorted(qs)
    got, err = LH.ask(qs, flags)
    return dict(zip(qs, got)), err


def check_areas(q, areas, tot, align=4):
    by_name, end = {a[0]: a for a in areas}, 0
    assert len(by_name) == len(areas), q
    for name, off, length, alias in areas:
        assert off >= 0 and length > 0 and off % align == 0, (q, name, off, length)      # (every buffer is read 16 bytes at a time)
        if alias is None:
            assert off >= end, (q, name, off, end)          # ascending and disjoint
            end = off + length
        else:
            _, aoff, alen, aalias = by_name[alias]
            assert aalias is None and aoff <= off and off + length <= aoff + alen, (q, name, alias)
    assert end <= tot and tot * 4 <= LDS_BYTES, (q, end, tot)


def test_every_layout_is_ordered_disjoint_aligned_and_within_its_total():
    got, err = answers()
    assert not err
    kinds = {}
    for q, (areas, tot) in got.items():
        if q[0] == "widesweep":
            check_areas(q, areas, tot)
            kinds[q[0]] = kinds.get(q[0], 0) + 1
    assert kinds["widesweep"] >= 10, kinds      # units narrower and shorter than a full one
    assert {q[1] < WIDE_UNIT for q in got if q[0] == "widesweep"} == {q[2] < WIDE_UNIT for q in got if q[0] == "widesweep"} == {True, False}


def test_the_parts_of_the_lean_chains_scratch():
    areas, tot = answers()[0][("scratch",)]
    check_areas(("scratch",), areas, tot)
    parts = sorted((a[1], a[2]) for a in areas if a[3] == "scr")
    assert len(parts) == 6 and all(x[0] + x[1] <= y[0] for x, y in zip(parts, parts[1:])), areas


def test_the_loop_words_of_the_resident_workgroup():
    areas, tot = answers()[0][("words",)]
    check_areas(("words",), areas, tot, align=1)
    by_name = {a[0]: a for a in areas}
    assert by_name["stats"][1] % 2 == 0                                 # LeanRes holds a double
    assert by_name["wait"][1:3] == by_name["pick"][1:3]                 # one word, a chain workgroup's and a unit workgroup's
    own = sorted((a[1], a[2]) for a in areas if a[3] == "words" and a[0] != "wait")
    assert all(x[0] + x[1] <= y[0] for x, y in zip(own, own[1:])), areas


def test_the_totals_are_the_budgets_of_the_plan_dump():
    """total * 4: lds_step of a wide plan as the maximum over the chunks it budgets."""
    got, seen = answers()[0], {"wide": 0}
    for cid, (s, _, units) in plans().items():
        wide, kernel = case_queries(cid)
        if wide:
            assert int(s["lds_step"]) == max(got[q][1] for q in wide) * 4, cid
            # the kernel asks with its unit's own columns and rows, the planner with the chunk's cut to a unit's size: no unit is larger
            # than that cut (WIDE_KB k-blocks, WIDE_RBG row blocks), and the largest unit is what the launch was sized for
            assert all(0 < nkb * 16 <= WIDE_UNIT and 0 < rows <= WIDE_UNIT for nkb, rows in units), cid
            assert int(s["lds_step"]) == max(got[q][1] for q in kernel) * 4, cid
            seen["wide"] += 1
    assert seen["wide"] >= 10, seen


def test_the_layouts_under_address_and_undefined_sanitizers():
    """The same program built with -fsanitize=address,undefined and run directly, stand-alone, over the same queries: clean, same answers."""
    why = DH.sanitizer_missing()
    if why:
        pytest.skip(why)
    got, err = answers(PH.SANITIZE)
    assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
    assert got == answers()[0]


@pytest.mark.parametrize("field,pick,mutation", [
    ("lds_step", "wide", ("m.xn = w.take(WIDE_SLICE * m.SN);", "m.xn = w.take(WIDE_SLICE * m.SN + 4);")),
], ids=["wide_sweep"])
def test_a_grown_area_moves_the_planners_budget(field, pick, mutation):
    """lds.hip.h with one area 4 floats longer, under the unchanged planner: pinned digests move, and in them the budget that is this
    layout's total grows by those 16 bytes — the planner has no second statement that would have kept it."""
    cases = [c for c in T.all_cases() if int(plans()[c["id"]][0][pick])][:12]
    assert len(cases) >= 5
    texts = LH.mutated_dumps(cases, mutation)
    moved = [(c["id"], t) for c, t in zip(cases, texts) if T.fnv64(t) != T.PINNED[c["id"]]]
    assert moved, field
    grown = [cid for cid, t in moved if int(T.parse(t)[0][field]) == int(plans()[cid][0][field]) + 16]
    assert grown, (field, [cid for cid, _ in moved][:10])
