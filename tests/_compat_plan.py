"""csrc/ntk_compat_plan.hpp compiled with g++ behind a C shim, for the CPU tests that ask the header itself: the constants of the batched
Sequence-trait calls and their chunk cut (tests/test_compat_plan.py, tests/test_compat_scale_inputs.py).  Test infrastructure."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT_PLAN_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_compat_plan.hpp")

SHIM = r"""
#include "ntk_compat_plan.hpp"
extern "C" {
uint64_t plan_default_chunk(void) { return kCompatChunkBytes; }
uint64_t plan_min_chunk(void) { return kCompatChunkMin; }
uint64_t plan_banks(void) { return kCompatBanks; }
uint64_t plan_long_record(void) { return kLongRecord; }
// the walk of run_banked: {r0, r1, bytes} of every chunk, at most `cap` of them; the number of chunks
uint64_t plan_walk(const uint64_t *offsets, uint64_t n_records, uint64_t chunk_bytes, uint64_t per_record, uint64_t *out, uint64_t cap)
{
    uint64_t n = 0;
    for (uint64_t r0 = 0; r0 < n_records; n++) {
        const CompatCut c = compat_cut(offsets, n_records, r0, chunk_bytes, per_record);
        if (n < cap) { out[3 * n] = c.r0; out[3 * n + 1] = c.r1; out[3 * n + 2] = c.bytes; }
        if (c.nrec() != c.r1 - c.r0) return ~(uint64_t)0;
        r0 = c.r1;
    }
    return n;
}
}
"""


def build(tmp_dir):
    """The shim as a ctypes library, compiled into tmp_dir."""
    src, so = os.path.join(str(tmp_dir), "shim.cpp"), os.path.join(str(tmp_dir), "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.dirname(COMPAT_PLAN_HPP), "-o", so, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(so)
    u64, p64 = C.c_uint64, C.POINTER(C.c_uint64)
    for name, argtypes in (("plan_default_chunk", []), ("plan_min_chunk", []), ("plan_banks", []), ("plan_long_record", []),
                           ("plan_walk", [p64, u64, u64, u64, p64, u64])):
        getattr(lib, name).argtypes = argtypes
        getattr(lib, name).restype = u64
    return lib


def walk(lib, offsets, chunk_bytes, per_record):
    """[(r0, r1, bytes)] of every chunk the header cuts out of the records that `offsets` (n + 1 of them) bounds."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offs) - 1
    out = np.zeros(3 * max(n, 1), dtype=np.uint64)
    p64 = C.POINTER(C.c_uint64)
    got = lib.plan_walk(offs.ctypes.data_as(p64), n, chunk_bytes, per_record, out.ctypes.data_as(p64), n)
    assert got <= n, "a chunk without a record, or nrec() is not r1 - r0"
    return [tuple(int(x) for x in out[3 * i: 3 * i + 3]) for i in range(got)]
