"""The work list of k_tap_grad (mfas_amd/csrc/tapgrad.hip.h: tap_grad_units, plain C++17) on the CPU, in the manner of
tests/plan_header.py: compiled with g++ alone into a program that reads plan_header's cases from stdin, plans each and prints, for the
first and the last candidate, the units of every declared tap slot (requested whether the candidate selects it or not).  One line per
candidate — `cand k base size L | s t n per cell` — and one per unit — `unit kind tap kb0 nkb width nitems nrb | cell w_off rb_stride ...`.
The same program also builds under the address and undefined sanitizers; it is a stand-alone executable."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

from tests import plan_header as PH

MAIN = r"""
#include <stdio.h>
#include "tapgrad.hip.h"
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
        char tmp[256];
        LayoutPlan pl;
        int rc = validate_inputs(&hp, confs.data(), n_cells.data(), K);
        if (!rc) rc = plan_layout(&hp, confs.data(), n_cells.data(), has_seeds ? seeds.data() : nullptr, K, cc, n_cus, persist != 0, tuning_from_env(), pl);
        for (int k = 0; k < K && !rc; k += (K > 1 ? K - 1 : 1)) {
            bool want[2][MFAS_MAX_TAPS];
            for (int j = 0; j < MFAS_MAX_TAPS; ++j) { want[KIND_S][j] = hp.s_sizes[j] > 0; want[KIND_V][j] = hp.v_sizes[j] > 0; }
            std::vector<TapGradDesc> units;
            rc = tap_grad_units(pl, hp, k, want, units);
            if (rc) break;
            snprintf(tmp, sizeof(tmp), "cand %d %lld %lld %d %d |", k, (long long)pl.cand_plane_base[k], (long long)pl.cand_plane_size[k], n_cells[k], pl.g.nrb);
            text += tmp;
            for (int i = 0; i < n_cells[k]; ++i) { snprintf(tmp, sizeof(tmp), " %d %d", confs[(k * 4 + i) * 3], confs[(k * 4 + i) * 3 + 1]); text += tmp; }
            text += "\n";
            for (const TapGradDesc& u : units) {
                snprintf(tmp, sizeof(tmp), "unit %d %d %d %d %d %d %d |", u.kind, u.tap, u.kb0, u.nkb, u.width, u.nitems, u.nrb);
                text += tmp;
                for (int it = 0; it < u.nitems; ++it) { snprintf(tmp, sizeof(tmp), " %d %lld %d", u.cell[it], (long long)u.w_off[it], u.rb_stride[it]); text += tmp; }
                text += "\n";
            }
            // a slot of width 0 is refused, naming the slot, and leaves no unit
            for (int j = 0; j < MFAS_MAX_TAPS; ++j)
                if (hp.v_sizes[j] == 0) {
                    bool w0[2][MFAS_MAX_TAPS] = {};
                    w0[KIND_V][j] = true;
                    const int r0 = tap_grad_units(pl, hp, k, w0, units);
                    snprintf(tmp, sizeof(tmp), "refused v%d %d %d %s\n", j, r0, (int)units.size(), g_err.c_str());
                    text += tmp;
                    break;
                }
        }
        if (rc) text = g_err;
        printf("== %d %zu\n", rc, text.size());
        fwrite(text.data(), 1, text.size(), stdout);
    }
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def program(mutation=None, flags=()):
    """The compiled program (once per process and variant).  mutation: (old, new) — tapgrad.hip.h is compiled from a copy with that one
    piece of text replaced.  flags: further g++ flags (PH.SANITIZE)."""
    d = tempfile.mkdtemp(prefix="mfas_tapgrad_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with open(os.path.join(d, "main.cpp"), "w") as f:
        f.write(MAIN)
    if mutation is not None:
        src = open(os.path.join(PH.CSRC, "tapgrad.hip.h")).read()
        assert src.count(mutation[0]) == 1, mutation
        with open(os.path.join(d, "tapgrad.hip.h"), "w") as f:
            f.write(src.replace(mutation[0], mutation[1]))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + d, "-I" + PH.CSRC, "-I" + os.path.join(PH.ROOT, "include"),
                           os.path.join(d, "main.cpp"), "-o", os.path.join(d, "main")])
    return os.path.join(d, "main")


def dumps(cases, mutation=None, flags=()):
    """-> the work-list text of every case, in the cases' order (plan_header.dumps runs the program once per distinct env)."""
    return PH.dumps(cases, 0, exe=program(mutation, tuple(flags)), flags=flags)[0]


def parse(text):
    """-> [(cand record, [unit records])], refusals: cand = dict(k, base, size, L, nrb, conf [(s, v)]), unit = dict(kind, tap, kb0, nkb, width,
    nitems, nrb, items [(cell, w_off, rb_stride)])."""
    out, refused = [], []
    for line in text.splitlines():
        head, _, tail = line.partition("|")
        h, t = head.split(), [int(x) for x in tail.split()]
        if h[0] == "cand":
            k, base, size, L, nrb = (int(x) for x in h[1:])
            out.append((dict(k=k, base=base, size=size, L=L, nrb=nrb, conf=list(zip(t[0::2], t[1::2]))), []))
        elif h[0] == "unit":
            kind, tap, kb0, nkb, width, nitems, nrb = (int(x) for x in h[1:])
            out[-1][1].append(dict(kind=kind, tap=tap, kb0=kb0, nkb=nkb, width=width, nitems=nitems, nrb=nrb,
                                   items=list(zip(t[0::3], t[1::3], t[2::3]))))
        else:
            assert h[0] == "refused", line
            refused.append((h[1], int(h[2]), int(h[3]), " ".join(h[4:])))
    return out, refused
