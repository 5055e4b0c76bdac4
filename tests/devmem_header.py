"""mfas_amd/csrc/devmem.hip.h (plain C++17) on the CPU, in the manner of tests/builds_header.py: compiled with g++ alone against a
stand-in for the runtime names it uses, into a program that walks DevBuf through every promise it makes and checks each one against
the stand-in's books (blocks handed out, blocks freed, calls made).  The stand-in keeps every live block in a set, aborts on a free
of a pointer it never handed out, and fails the n-th hipMalloc on request (leaving garbage in the out pointer)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfas_amd", "csrc")

STANDIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
static std::set<void*> g_live;                     // blocks handed out and not yet freed
static long g_mallocs, g_frees, g_copies, g_fail_in;     // calls made; g_fail_in = n: the n-th hipMalloc from now fails
static hipError_t hipMalloc(void** p, size_t bytes) {
    ++g_mallocs;
    if (g_fail_in && --g_fail_in == 0) { *p = reinterpret_cast<void*>(0x10); return hipErrorOutOfMemory; }
    g_live.insert(*p = malloc(bytes));
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    ++g_frees;
    if (p && !g_live.erase(p)) { fprintf(stderr, "hipFree(%p): never handed out, or freed twice\n", p); abort(); }
    free(p);
    return hipSuccess;
}
static hipError_t hipMemcpy(void* d, const void* s, size_t bytes, hipMemcpyKind) { ++g_copies; memcpy(d, s, bytes); return hipSuccess; }
"""

MAIN = r"""
#include "devmem.hip.h"
#include <utility>
static int g_bad = 0;
#define CHECK(what, x) do { if (!(x)) { printf("FAILED %s: %s (line %d)\n", what, #x, __LINE__); ++g_bad; } } while (0)
static long calls() { return g_mallocs + g_frees + g_copies; }
struct Owner {      // like mfas_population: members that own, a destructor of its own, defaulted moves
    DevBuf<float> a; DevBuf<int> b; std::vector<DevBuf<char>> v;
    Owner() = default;
    Owner(Owner&&) = default;
    Owner& operator=(Owner&&) = default;
    ~Owner() {}
};
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "wild_free")) { int x = 0; hipFree(&x); return 0; }      // (the stand-in aborts)
    {
        DevBuf<float> b;
        CHECK("empty", !b && b.get() == nullptr && b.size() == 0 && calls() == 0);
        CHECK("first reserve", b.reserve(8) == hipSuccess && b && b.size() == 8 && g_mallocs == 1 && g_frees == 0);
        float* p8 = b.get();
        long n = calls();
        CHECK("reserve within capacity", b.reserve(8) == hipSuccess && b.reserve(3) == hipSuccess && b.reserve(0) == hipSuccess);
        CHECK("reserve within capacity", calls() == n && b.get() == p8 && b.size() == 8);
        CHECK("growth", b.reserve(16) == hipSuccess && b.size() == 16 && g_mallocs == 2 && g_frees == 1 && g_live.size() == 1);
        CHECK("growth", g_live.count(b.get()) == 1);
        g_fail_in = 1;
        CHECK("failed growth", b.reserve(32) == hipErrorOutOfMemory);
        CHECK("failed growth", !b && b.get() == nullptr && b.size() == 0 && g_frees == 2 && g_live.empty());
        n = g_mallocs;
        CHECK("smaller reserve after a failed growth", b.reserve(4) == hipSuccess && g_mallocs == n + 1 && b.get() != nullptr && b.size() == 4);
        CHECK("smaller reserve after a failed growth", g_live.count(b.get()) == 1);
        g_fail_in = 1;
        CHECK("failed alloc", b.alloc(2) == hipErrorOutOfMemory && !b && b.size() == 0 && g_live.empty());
        CHECK("alloc is exact", b.alloc(9) == hipSuccess && b.size() == 9 && b.alloc(5) == hipSuccess && b.size() == 5 && g_live.size() == 1);
        n = g_mallocs;
        CHECK("alloc(0)", b.alloc(0) == hipSuccess && !b && b.size() == 0 && g_mallocs == n && g_live.empty());
        CHECK("upload of an empty vector", b.upload(std::vector<float>()) == hipSuccess && !b && b.size() == 0 && g_mallocs == n && g_copies == 0);
        const std::vector<float> v = {1.f, 2.f, 3.f};
        CHECK("upload", b.upload(v) == hipSuccess && b.size() == 3 && g_copies == 1 && !memcmp(b.get(), v.data(), sizeof(float) * 3));
        CHECK("upload of an empty vector over a full buffer", b.upload(std::vector<float>()) == hipSuccess && !b && g_live.empty());
        b.reset(); b.reset();
        CHECK("reset of an empty buffer", !b && g_live.empty());
    }
    {
        DevBuf<int> a, c, d;
        CHECK("setup", a.alloc(4) == hipSuccess && c.alloc(2) == hipSuccess && d.alloc(5) == hipSuccess && g_live.size() == 3);
        int *pa = a.get(), *pd = d.get();
        long n = calls();
        DevBuf<int> b(std::move(a));
        CHECK("move construction", calls() == n && a.get() == nullptr && a.size() == 0 && b.get() == pa && b.size() == 4);
        const long f = g_frees;
        c = std::move(b);
        CHECK("move assignment", g_frees == f + 1 && calls() == n + 1 && b.get() == nullptr && b.size() == 0 && c.get() == pa && c.size() == 4);
        CHECK("move assignment", g_live.size() == 2 && g_live.count(pa) && g_live.count(pd));
        n = calls();
        std::swap(c, d);
        CHECK("swap", calls() == n && c.get() == pd && c.size() == 5 && d.get() == pa && d.size() == 4 && g_live.size() == 2);
    }
    CHECK("scope end", g_live.empty());
    {
        Owner p, q;
        p.v.resize(3);
        CHECK("owner setup", p.a.alloc(7) == hipSuccess && p.v[1].alloc(1) == hipSuccess && q.a.alloc(2) == hipSuccess && q.b.alloc(3) == hipSuccess);
        float* pa = p.a.get(); char* pv = p.v[1].get(); int* qb = q.b.get();
        const long n = calls();
        std::swap(p, q);
        CHECK("swap of two owners", calls() == n && g_live.size() == 4 && q.a.get() == pa && q.a.size() == 7 && q.v.size() == 3 && q.v[1].get() == pv);
        CHECK("swap of two owners", p.b.get() == qb && p.a.size() == 2 && p.v.empty() && !q.b);
    }
    long failed = 2;     // (the two hipMallocs told to fail)
    CHECK("program end", g_live.empty() && g_mallocs - failed == g_frees);
    printf("live=%zu mallocs=%ld frees=%ld copies=%ld bad=%d\n", g_live.size(), g_mallocs, g_frees, g_copies, g_bad);
    return g_bad ? 1 : 0;
}
"""

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")


@functools.lru_cache(maxsize=None)
def program(mutation=None, flags=()):
    """The compiled program (once per process and variant).  mutation: (old, new) — the header is compiled from a copy with that one
    piece of text replaced.  flags: further g++ flags (the sanitizer build)."""
    d = tempfile.mkdtemp(prefix="mfas_devmem_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with open(os.path.join(d, "main.cpp"), "w") as f:
        f.write(STANDIN + MAIN)
    inc = CSRC
    if mutation is not None:
        src = open(os.path.join(CSRC, "devmem.hip.h")).read()
        assert src.count(mutation[0]) == 1, mutation
        with open(os.path.join(d, "devmem.hip.h"), "w") as f:
            f.write(src.replace(mutation[0], mutation[1]))
        inc = d
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + inc, os.path.join(d, "main.cpp"), "-o", os.path.join(d, "main")])
    return os.path.join(d, "main")


def run(mutation=None, flags=(), args=(), env=None):
    """-> CompletedProcess of the program, run directly as a stand-alone executable"""
    return subprocess.run([program(mutation, tuple(flags)), *args], capture_output=True, text=True, env=env, timeout=120)


@functools.lru_cache(maxsize=None)
def sanitizer_missing():
    """None when this g++ links and runs an address + undefined sanitizer build, else the reason"""
    d = tempfile.mkdtemp(prefix="mfas_devmem_san_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with open(os.path.join(d, "t.cpp"), "w") as f:
        f.write("int main() { return 0; }\n")
    res = subprocess.run(["g++", *SANITIZE, os.path.join(d, "t.cpp"), "-o", os.path.join(d, "t")], capture_output=True, text=True)
    if res.returncode:
        return "g++ has no sanitizer runtime: " + res.stderr.strip().splitlines()[-1]
    return None
