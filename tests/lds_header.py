"""mfas_amd/csrc/lds.hip.h (plain C++17) on the CPU, in the manner of tests/plan_header.py and tests/builds_header.py: compiled with g++
alone, together with tests/lds_dump.h, into a program that reads one layout query per line and prints the layout's areas.  Also the
planner's program (tests/plan_header.py) over a copy of lds.hip.h with one piece of text replaced, for the tests that show the planner
takes the budgets of the layouts in that header from it and from nowhere else."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

from tests import plan_header as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfas_amd", "csrc")
HERE = os.path.join(ROOT, "tests")

MAIN = r"""
#include "lds_dump.h"
int main() {
    char line[256], what[32];
    while (fgets(line, sizeof(line), stdin)) {
        int v[12], n = 0, used = 0, step = 0;
        if (sscanf(line, "%31s%n", what, &used) != 1) continue;
        while (n < 12 && sscanf(line + used, "%d%n", &v[n], &step) == 1) { used += step; ++n; }
        if (!lds_query(what, v, n)) return 2;
    }
    return 0;
}
"""

# a layout's arguments, in the order of its function in lds.hip.h (after `base`)
ARGS = dict(widesweep=("cols", "rows"), words=(), scratch=())


@functools.lru_cache(maxsize=None)
def program(flags=()):
    """The compiled program (once per process and variant).  flags: further g++ flags (the sanitizer build)."""
    d = tempfile.mkdtemp(prefix="mfas_lds_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with open(os.path.join(d, "main.cpp"), "w") as f:
        f.write(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-I" + HERE, os.path.join(d, "main.cpp"), "-o",
                           os.path.join(d, "main")])
    return os.path.join(d, "main")


def ask(queries, flags=()):
    """queries: (layout, int...) in ARGS' order -> per query (areas, total, stderr of the run): areas = [(name, offset, length,
    alias-of or None)] in the layout's order.  One run of the program, directly, as a stand-alone executable."""
    for q in queries:
        assert len(q) == 1 + len(ARGS[q[0]]), q
    text = "".join(" ".join([q[0]] + [str(int(x)) for x in q[1:]]) + "\n" for q in queries)
    env = {k: v for k, v in os.environ.items() if not (flags and k == "LD_PRELOAD")}
    res = subprocess.run([program(tuple(flags))], input=text, capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    lines, out, pos = res.stdout.splitlines(), [], 0
    for q in queries:
        tag, n, total = lines[pos].split()
        assert tag == "==", (q, lines[pos])
        rows = [ln.split() for ln in lines[pos + 1:pos + 1 + int(n)]]
        out.append(([(r[0], int(r[1]), int(r[2]), None if r[3] == "-" else r[3]) for r in rows], int(total)))
        pos += 1 + int(n)
    assert pos == len(lines), (pos, len(lines))
    return out, res.stderr


@functools.lru_cache(maxsize=None)
def planner_over(mutation):
    """The planner's program (tests/plan_header.py: MAIN, tests/plan_dump.h) with lds.hip.h compiled from a copy in which mutation =
    (old, new) is replaced.  plan.hip.h is copied beside it unchanged, so that its `#include "lds.hip.h"` finds the copy."""
    d = tempfile.mkdtemp(prefix="mfas_lds_plan_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with open(os.path.join(d, "main.cpp"), "w") as f:
        f.write(PH.MAIN)
    src = open(os.path.join(CSRC, "lds.hip.h")).read()
    assert src.count(mutation[0]) == 1, mutation
    with open(os.path.join(d, "lds.hip.h"), "w") as f:
        f.write(src.replace(mutation[0], mutation[1]))
    shutil.copy(os.path.join(CSRC, "plan.hip.h"), d)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + d, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-I" + HERE,
                           os.path.join(d, "main.cpp"), "-o", os.path.join(d, "main")])
    return os.path.join(d, "main")


def mutated_dumps(cases, mutation):
    """The mode-0 plan dump of every case from planner_over(mutation), as PH.dumps gives it for the planner that ships."""
    return PH.dumps(cases, exe=planner_over(mutation))[0]
