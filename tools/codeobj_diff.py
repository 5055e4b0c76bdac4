#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two BUILT libraries: `llvm-objdump -d` of both gfx950 code objects, per kernel symbol `same` or
`differs` (instruction text + encoding; addresses dropped) with the two resource rows of tools/kernel_resources.py.  Exit status 1 if
a kernel OUTSIDE the expected set differs (or exists on one side only).  The expected set = the builds that contain the general chain:
k_step<., ., ., false, .>, k_step_same, k_chain<., false>.  --absent REGEX: kernels of that name are expected on the `before` side ONLY (builds
a change removes): each is reported, none counts as outside, and status 1 too if one of them is still there afterwards or none was there.
usage: python tools/codeobj_diff.py before.so after.so [expected regex] [--absent REGEX]"""
import re
import sys

from kernel_resources import HEADER, code_object, resource_rows, run_on

GENERAL_CHAIN = r"^(k_step<\d+, \w+, \d+, false, \d+>|k_step_same<.*>|k_chain<\d+, false>)$"


def kernels(co: bytes) -> dict:
    """{symbol: [instruction lines without their addresses]}"""
    out, cur = {}, None
    for line in run_on(co, "llvm-objdump", "-d").splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and "//" in line:
            text, enc = line.split("//", 1)
            cur.append(text.strip() + " | " + re.sub(r"^\s*[0-9A-Fa-f]+:|<.*>", "", enc).strip())
    return out


def main() -> int:
    argv = list(sys.argv)
    absent = re.compile(argv.pop(argv.index("--absent") + 1)) if "--absent" in argv else None
    argv = [a for a in argv if a != "--absent"]
    before, after = code_object(argv[1]), code_object(argv[2])
    expected = re.compile(argv[3] if len(argv) > 3 else GENERAL_CHAIN)
    ka, kb = kernels(before), kernels(after)
    ra, rb = resource_rows(before), resource_rows(after)
    print(f"{'':8s}{HEADER}")
    bad = ndiff = gone = 0
    for sym in list(ra) + [s for s in rb if s not in ra]:
        name = (ra.get(sym) or rb[sym])[0]
        same = sym in ra and sym in rb and ka.get(sym) == kb.get(sym) and ra[sym][1] == rb[sym][1]
        if same:
            print(f"{'same':8s}{name[:72]:72s} {ra[sym][1]}")
            continue
        if absent is not None and absent.match(name):
            gone += sym not in rb
            bad += sym in rb
            print(f"{'absent' if sym not in rb else 'PRESENT':8s}{name[:72]:72s} {ra[sym][1] if sym in ra else '(absent)'}" + ("   (expected)" if sym not in rb else "   <-- expected to be gone"))
            continue
        ndiff += 1
        ok = sym in ra and sym in rb and expected.match(name)
        bad += not ok
        print(f"{'differs':8s}{name[:72]:72s} {ra[sym][1] if sym in ra else '(absent)'}" + ("" if ok else "   <-- NOT in the expected set"))
        print(f"{'':8s}{'  after:':72s} {rb[sym][1] if sym in rb else '(absent)'}  ({len(ka.get(sym, []))} -> {len(kb.get(sym, []))} instructions)")
    print(f"{len(ra)} kernels, {ndiff} differ, {bad} outside the expected set" + (f", {gone} expected absent and absent" if absent is not None else ""))
    return 1 if bad or (absent is not None and not gone) else 0


if __name__ == "__main__":
    sys.exit(main())
