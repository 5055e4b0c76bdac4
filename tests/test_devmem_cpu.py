"""mfas_amd/csrc/devmem.hip.h on the CPU: DevBuf, the one owner of device memory on the host side, compiled with g++ alone against a
stand-in runtime (tests/devmem_header.py) that keeps the books.  The program checks, in this order:

* reserve within the capacity makes no runtime call; growth frees the old block exactly once;
* a failed growth leaves (nullptr, 0), and a following SMALLER reserve allocates anew — the stale capacity train_begin used to keep;
* alloc(0) and upload of an empty vector leave a null pointer; upload copies;
* move construction, move assignment and std::swap — of two buffers and of two owners with a destructor of their own, like
  mfas_population — neither leak nor free twice;
* nothing is live when the program ends.

The stand-in aborts on a free of a pointer it never handed out; one mutation of the header's text — reserve keeps its old size when
the allocation fails — fails the program; the same program passes as an address + undefined sanitizer build, run directly."""
import os
import signal

import pytest

from tests import devmem_header as DH


def test_devbuf_keeps_every_promise():
    res = DH.run()
    assert res.returncode == 0 and "FAILED" not in res.stdout, (res.stdout, res.stderr)
    assert res.stdout.strip().startswith("live=0 ") and res.stdout.strip().endswith("bad=0"), res.stdout


def test_standin_aborts_on_a_pointer_it_never_handed_out():
    res = DH.run(args=("wild_free",))
    assert res.returncode == -signal.SIGABRT and "never handed out" in res.stderr, (res.returncode, res.stderr)


def test_reserve_that_keeps_its_size_after_a_failure_is_caught():
    """The bug this header removes: the pointer is gone, the capacity is not, and a later smaller request launches on a null pointer."""
    old = "{ return n <= n_ ? hipSuccess : alloc(n); }"
    new = "{ if (n <= n_) return hipSuccess; const size_t old_n = n_; const hipError_t e = alloc(n); if (e != hipSuccess) n_ = old_n; return e; }"
    res = DH.run(mutation=(old, new))
    assert res.returncode == 1, (res.stdout, res.stderr)
    assert "FAILED failed growth" in res.stdout and "FAILED smaller reserve after a failed growth" in res.stdout, res.stdout


def test_devbuf_under_address_and_undefined_sanitizers():
    """A stand-alone executable, run directly: no sanitizer runtime is preloaded into anything."""
    why = DH.sanitizer_missing()
    if why:
        pytest.skip(why)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    res = DH.run(flags=DH.SANITIZE, env=env)
    assert res.returncode == 0 and "bad=0" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr, (res.stdout, res.stderr)
