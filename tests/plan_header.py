"""mfas_amd/csrc/plan.hip.h (plain C++17) on the CPU, in the manner of tests/builds_header.py and tests/devmem_header.py: compiled with
g++ alone, together with tests/plan_dump.h, into a program that reads cases from stdin — the mfas_hyper fields, the configurations,
optional drop seeds, K, chunk_cols, n_cus, allow_persist, mode — and prints the dump of each plan.  The switches are the program's
environment (tuning_from_env), so it runs once per distinct `env` of the cases, under that environment and no other MFAS_* variable."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from mfas_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfas_amd", "csrc")
HERE = os.path.join(ROOT, "tests")

# One case: "case mode K chunk_cols n_cus allow_persist has_seeds", the mfas_hyper fields in declaration order (doubles as C99 hex
# floats: exact), per candidate its cell count and 4 x 3 configuration entries, then the K drop seeds if there are any.
# One answer: "== <rc> <bytes>\n" and that many bytes of text (the dump, or the error message).
MAIN = r"""
#include <stdio.h>
#include "plan_dump.h"
static bool rd(int32_t& x) { long long v; if (scanf("%lld", &v) != 1) return false; x = (int32_t)v; return true; }
static bool rd(uint32_t& x) { long long v; if (scanf("%lld", &v) != 1) return false; x = (uint32_t)v; return true; }
static bool rd(double& x) { return scanf("%lf", &x) == 1; }
int main() {
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        int32_t mode, K, cc, n_cus, persist, has_seeds;
        if (strcmp(cmd, "case") || !rd(mode) || !rd(K) || !rd(cc) || !rd(n_cus) || !rd(persist) || !rd(has_seeds) || K < 0) return 2;
        mfas_hyper hp;
        memset(&hp, 0, sizeof(hp));
        bool ok = rd(hp.R) && rd(hp.C) && rd(hp.B) && rd(hp.bn) && rd(hp.alphas) && rd(hp.multitask) && rd(hp.drpt) && rd(hp.wd) && rd(hp.beta1) &&
                  rd(hp.beta2) && rd(hp.adam_eps) && rd(hp.bn_eps) && rd(hp.bn_momentum);
        for (int j = 0; j < MFAS_MAX_TAPS; ++j) ok = ok && rd(hp.s_sizes[j]);
        for (int j = 0; j < MFAS_MAX_TAPS; ++j) ok = ok && rd(hp.v_sizes[j]);
        ok = ok && rd(hp.loss_mode) && rd(hp.allow_plain_cell) && rd(hp.f1_threshold) && rd(hp.tap_bits) && rd(hp.order_per_candidate);
        std::vector<int32_t> confs((size_t)K * 12), n_cells((size_t)K);
        std::vector<uint32_t> seeds(has_seeds ? (size_t)K : 0);
        for (int k = 0; k < K; ++k) {
            ok = ok && rd(n_cells[k]);
            for (int q = 0; q < 12; ++q) ok = ok && rd(confs[(size_t)k * 12 + q]);
        }
        for (uint32_t& s : seeds) ok = ok && rd(s);
        if (!ok) return 2;
        std::string text;
        const int rc = plan_dump(&hp, confs.data(), n_cells.data(), has_seeds ? seeds.data() : nullptr, K, cc, n_cus, persist, mode, text);
        if (rc) text = g_err;
        printf("== %d %zu\n", rc, text.size());
        fwrite(text.data(), 1, text.size(), stdout);
    }
    return 0;
}
"""

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")


@functools.lru_cache(maxsize=None)
def program(mutation=None, flags=()):
    """The compiled program (once per process and variant).  mutation: (old, new) — plan.hip.h is compiled from a copy with that one
    piece of text replaced, for the tests that show a wrong plan is caught.  flags: further g++ flags (the sanitizer build)."""
    d = tempfile.mkdtemp(prefix="mfas_plan_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with open(os.path.join(d, "main.cpp"), "w") as f:
        f.write(MAIN)
    if mutation is not None:
        src = open(os.path.join(CSRC, "plan.hip.h")).read()
        assert src.count(mutation[0]) == 1, mutation
        with open(os.path.join(d, "plan.hip.h"), "w") as f:
            f.write(src.replace(mutation[0], mutation[1]))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + d, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-I" + HERE,
                           os.path.join(d, "main.cpp"), "-o", os.path.join(d, "main")])
    return os.path.join(d, "main")


def case_text(case, mode):
    K = len(case["confs"])
    cf, nc = np.zeros((K, 4, 3), np.int32), np.zeros(K, np.int32)
    for k, c in enumerate(case["confs"]):
        cf[k, :len(c)], nc[k] = c, len(c)
    hc, words = case["hp"].to_c(), []
    for name, ctype in _lib.mfas_hyper._fields_:
        v = getattr(hc, name)
        words += [float(v).hex()] if isinstance(v, float) else [str(int(x)) for x in (v if hasattr(v, "__len__") else [v])]
    seeds = case["seeds"]
    head = ["case", mode, K, case["cc"], case["n_cus"], int(case["persist"]), int(seeds is not None)]
    rows = [" ".join(map(str, [nc[k], *cf[k].ravel()])) for k in range(K)]
    return "\n".join([" ".join(map(str, head)), " ".join(words), *rows, " ".join(str(int(s)) for s in (seeds or []))]) + "\n"


def dumps(cases, mode=0, mutation=None, flags=(), exe=None):
    """-> (texts, stderr): the dump of every case, in the cases' order, and what the runs wrote to stderr.  One run of the program —
    directly, as a stand-alone executable — per distinct env.  exe: another build of the same program (tests/lds_header.py's, over a
    changed lds.hip.h) in place of program(mutation, flags)."""
    exe = exe or program(mutation, tuple(flags))
    by_env, texts, errs = {}, {}, []
    for c in cases:
        by_env.setdefault(tuple(sorted(c["env"].items())), []).append(c)
    # (the pins hold for the case's switches alone; a sanitizer build runs with nothing preloaded, as tests/test_devmem_cpu.py's does)
    base = {k: v for k, v in os.environ.items() if not k.startswith("MFAS_") and not (flags and k == "LD_PRELOAD")}
    for env, group in by_env.items():
        res = subprocess.run([exe], input="".join(case_text(c, mode) for c in group).encode(), capture_output=True, env=dict(base, **dict(env)), timeout=1200)
        errs.append(res.stderr.decode(errors="replace"))
        assert res.returncode == 0, (dict(env), res.returncode, errs[-1][-2000:])
        out, pos = res.stdout, 0
        for c in group:
            eol = out.index(b"\n", pos)
            tag, rc, n = out[pos:eol].split()
            assert tag == b"==" and int(rc) == 0, (c["id"], out[pos:eol + 1 + int(n)])
            texts[c["id"]] = out[eol + 1:eol + 1 + int(n)].decode()
            pos = eol + 1 + int(n)
        assert pos == len(out), (dict(env), len(out) - pos)
    return [texts[c["id"]] for c in cases], "".join(errs)
