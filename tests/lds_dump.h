// lds_dump.h — every area of every layout of mfas_amd/csrc/lds.hip.h as text, for tests/test_lds_cpu.py: one query per line (a layout's
// name and the arguments of its function, in the function's order), one answer "== <areas> <total>" followed by a line
// "name offset length alias-of" per area ("-": the area lies in no other).  The layouts are asked with base 0, as the planner asks
// them.  What is an alias of what is read off the layout functions: an area they do not take from the walk, but place in another one.
// Plain C++17: part of the g++ program of tests/lds_header.py, of no library.
#pragma once
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "lds.hip.h"

struct LdsRow { const char* name; LdsArea<int32_t> a; const char* alias; };

static void lds_answer(const std::vector<LdsRow>& rows, int32_t total) {
    printf("== %zu %d\n", rows.size(), total);
    for (const LdsRow& r : rows) printf("%s %d %d %s\n", r.name, r.a.at, r.a.len, r.alias);
}
#define A(m, x) LdsRow{#x, (m).x, "-"}

// one query; false: unknown layout or malformed arguments
static bool lds_query(const char* what, const int* v, int n) {
    auto args = [&](int want) { return n == want; };
    if (!strcmp(what, "widesweep") && args(2)) {
        const auto m = wide_sweep_lds(0, v[0], v[1]);
        lds_answer({A(m, xt), A(m, xn), A(m, dy)}, m.total);
    } else if (!strcmp(what, "words") && args(0)) {
        // k_president's loop words inside their PERSIST_LDS_WORDS (wait and pick: one word, the two kinds of workgroup)
        const LdsArea<int32_t> all{0, PERSIST_LDS_WORDS};
        lds_answer({LdsRow{"words", all, "-"}, LdsRow{"wait", {PresWords::wait, 1}, "words"}, LdsRow{"pick", {PresWords::pick, 1}, "words"},
                    LdsRow{"roll", {PresWords::roll, 1}, "words"}, LdsRow{"arrive", {PresWords::arrive, 1}, "words"},
                    LdsRow{"next", {PresWords::next, 2}, "words"}, LdsRow{"stats", {PresWords::stats, 6}, "words"}}, PERSIST_LDS_WORDS);
    } else if (!strcmp(what, "scratch") && args(0)) {
        // the parts of chain_lean's exchange scratch inside its LEAN_SCR floats
        const LdsArea<int32_t> all{0, LEAN_SCR};
        lds_answer({LdsRow{"scr", all, "-"}, LdsRow{"bn_fwd", {LeanScr::bn_fwd, 256}, "scr"}, LdsRow{"gv2", {LeanScr::gv2, 128}, "scr"},
                    LdsRow{"bnf", {LeanScr::bnf, 16}, "scr"}, LdsRow{"bnv", {LeanScr::bnv, 64}, "scr"},
                    LdsRow{"bn_bwd", {LeanScr::bn_bwd, 256}, "scr"}, LdsRow{"bst", {LeanScr::bst, 256}, "scr"}}, LEAN_SCR);
    } else {
        return false;
    }
    return true;
}
#undef A
