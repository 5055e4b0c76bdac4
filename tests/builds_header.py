"""mfas_amd/csrc/builds.hip.h (plain C++17) on the CPU, for the tests that hold build names: compiled with g++ alone into a program
that answers queries — the choice functions over plan facts and launch-time inputs, plan_keys, the kernel tables' keys — with the
names the launch record spells.  Nothing here restates a choice: the tests compare their literals with what the header answers."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfas_amd", "csrc")

# PlanFacts, in the order the program reads them
FIELDS = ("wide", "MB", "lean", "same_group", "chain_split", "groups", "nt", "persist", "res_wide", "res_nu", "mbe", "nrbw", "nrb")
DEFAULTS = dict(wide=0, MB=1, lean=0, same_group=0, chain_split=0, groups=1, nt=0, persist=0, res_wide=0, res_nu=1, mbe=4, nrbw=1, nrb=1)
DTYPE = {"float32": 0, "bfloat16": 1, "float16": 2}

MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "builds.hip.h"
static void names(const std::vector<BuildKey>& keys) {
    for (size_t i = 0; i < keys.size(); ++i) printf("%s%s", i ? " " : "", keys[i].name().c_str());
    printf("\n");
}
int main() {
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        int v[13], a[5] = {0, 0, 0, 0, 0};
        if (!strcmp(cmd, "tables")) { names(table_keys()); continue; }
        if (!strcmp(cmd, "plain")) {
            if (scanf("%d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4) != 5) return 2;
            printf("%d\n", president_plain(a[0], a[1], a[2], a[3], a[4]));
            continue;
        }
        for (int& x : v) if (scanf("%d", &x) != 1) return 2;
        PlanFacts f;
        f.wide = v[0]; f.MB = v[1]; f.lean_chain = v[2]; f.same_group = v[3]; f.chain_split = v[4]; f.ngroups = v[5]; f.nontemporal = v[6];
        f.persist = v[7]; f.res_wide = v[8]; f.res_nu = v[9]; f.mbe = v[10]; f.nrbw = v[11]; f.nrb = v[12];
        const int extra = !strcmp(cmd, "step") ? 3 : !strcmp(cmd, "president") ? 2 : !strcmp(cmd, "eval") ? 4 : 0;
        for (int i = 0; i < extra; ++i) if (scanf("%d", a + i) != 1) return 2;
        if (!strcmp(cmd, "plan")) names(plan_keys(f));
        else if (!strcmp(cmd, "step")) names({step_key(f, (unsigned)a[0], a[1], a[2])});
        else if (!strcmp(cmd, "chain")) names({chain_key(f)});
        else if (!strcmp(cmd, "president")) names({president_key(f, a[0], a[1])});
        else if (!strcmp(cmd, "eval")) names({eval_key(f, a[0], a[1], a[2], a[3])});
        else if (!strcmp(cmd, "sb_step")) names({single_batch_step_key(f)});
        else if (!strcmp(cmd, "sb_chain")) names({single_batch_chain_key(f)});
        else return 3;
    }
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def program(mutation=None):
    """The compiled program (once per process).  mutation: (old, new) — the header is compiled from a copy with that one piece of
    text replaced, for the tests that show a wrong choice is caught."""
    d = tempfile.mkdtemp(prefix="mfas_builds_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with open(os.path.join(d, "main.cpp"), "w") as f:
        f.write(MAIN)
    inc = CSRC
    if mutation is not None:
        src = open(os.path.join(CSRC, "builds.hip.h")).read()
        assert src.count(mutation[0]) == 1, mutation
        with open(os.path.join(d, "builds.hip.h"), "w") as f:
            f.write(src.replace(mutation[0], mutation[1]))
        inc = d
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + inc, "-I" + CSRC, os.path.join(d, "main.cpp"), "-o", os.path.join(d, "main")])      # (CSRC: records.hip.h beside a mutated copy)
    return os.path.join(d, "main")


def facts(**kw):
    """PlanFacts as a dict: the defaults with `kw` over them (booleans and ints alike)."""
    assert set(kw) <= set(FIELDS), kw
    return dict(DEFAULTS, **{k: int(v) for k, v in kw.items()})


def ask(queries, mutation=None):
    """queries: (command, facts or None, further ints...) -> one answer per query: a list of names for "plan" and "tables", an int
    for "plain", else one name."""
    text = "".join(" ".join([q[0]] + [str(int(q[1][k])) for k in FIELDS if q[1] is not None] + [str(int(x)) for x in q[2:]]) + "\n" for q in queries)
    out = subprocess.run([program(mutation)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(queries), (len(out), len(queries))
    return [o.split() if q[0] in ("plan", "tables") else int(o) if q[0] == "plain" else o for q, o in zip(queries, out)]


def ask1(*query, mutation=None):
    return ask([query], mutation)[0]
