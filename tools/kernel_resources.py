#!/usr/bin/env python3
"""Per-kernel register / scratch / spill table of a BUILT library (no recompilation): carves the gfx950 code object out of the
.so's clang offload bundle and reads the kernel metadata notes.  usage: python tools/kernel_resources.py [lib.so] [name filter]
(tools/codeobj_diff.py compares two libraries kernel by kernel with the same pieces)"""
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
HEADER = f"{'kernel':72s} VGPR AGPR SGPR scratch sspill vspill  LDS"


def code_object(lib: str) -> bytes:
    """The gfx950 code object inside the library's clang offload bundle."""
    blob = open(lib, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    at = blob.find(magic)
    assert at >= 0, "no offload bundle"
    n = struct.unpack_from("<Q", blob, at + len(magic))[0]
    pos = at + len(magic) + 8
    co = None
    for _ in range(n):
        off, size, tl = struct.unpack_from("<QQQ", blob, pos)
        triple = blob[pos + 24:pos + 24 + tl].decode()
        pos += 24 + tl
        if "gfx950" in triple:
            co = blob[at + off:at + off + size]
    assert co, "no gfx950 code object"
    return co


def run_on(co: bytes, tool: str, *flags) -> str:
    """Output of an LLVM binutil on the code object."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        return subprocess.run([LLVM + tool, *flags, f.name], capture_output=True, text=True, check=True).stdout


def short_name(demangled: str) -> str:
    return re.sub(r"\(.*", "", demangled).replace("void ", "")


def resource_rows(co: bytes) -> dict:
    """{mangled kernel name: (short demangled name, table row)} in the code object's order."""
    txt = run_on(co, "llvm-readelf", "--notes")
    names, rows = [], []
    for blk in re.split(r"\n\s+- \.agpr_count:", txt)[1:]:
        def f(k):
            m = re.search(r"\." + k + r":\s+(\d+)", blk)
            return int(m.group(1)) if m else -1
        names.append(re.search(r"\.name:\s+(\S+)", blk).group(1))
        r = (f("vgpr_count"), int(re.match(r"\s*(\d+)", blk).group(1)), f("sgpr_count"), f("private_segment_fixed_size"),
             f("sgpr_spill_count"), f("vgpr_spill_count"), f("group_segment_fixed_size"))
        rows.append(f"{r[0]:4d} {r[1]:4d} {r[2]:4d} {r[3]:7d} {r[4]:6d} {r[5]:6d} {r[6]:5d}")
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.strip().split("\n")
    return {nm: (short_name(d), row) for nm, d, row in zip(names, dem, rows)}


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else "mfas_amd/csrc/libmfas_hip.so"
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    print(HEADER)
    for nm, row in resource_rows(code_object(lib)).values():
        if flt in nm:
            print(f"{nm[:72]:72s} {row}")
