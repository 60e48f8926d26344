"""The windowed-minimizer scans at their tile seams, on the CPU: the inputs of tests/_seams.py min_seam_inputs - a break at every offset
around each seam of a three-tile input, a palindrome whose two tied k-mers slide across it - through the lock-step wave emulation of the
register-fused builds (emu_minimizers: lane_tile_sv2_min at the kernel's tile geometry) and of the generic kernel (emu_minimizers_generic:
minimizer_lane at its run-time geometry, both key forms, with a quality stream) against the literal minimizer of every window (oracle).  A
window that straddles a seam needs its k-mers imported from the previous tile, the invalid smear over its w window ends, and the leftmost
rule across the import; test_minimizer_seam_inputs.py shows that the palindromes tell leftmost from rightmost.  The emulator runs the
per-lane source only: the same inputs run on the device in test_gpu_minimizer_seams.py, and a mismatch there that does not show here is in
what the emulator leaves out (work pulls, launch plan, buffer bounds, LDS histogram).  Offsets further than k + w + 2 from their seam are
thinned to every fourth (thin_far); measured times are in profiles/seam_sweeps/README.md."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O

from _seams import FUSED_PAIRS, GENERIC_PAIRS, map_threads, min_seam_inputs, min_stride, thin_far

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CUTOFF = 53
RULES = ((1, 1), (0, 0))   # (tie_rc, accept_u): the byte path and the bit path

_EMU = None


@pytest.fixture(scope="module")
def emu():
    global _EMU
    if _EMU is None:
        so = os.path.join(EMU_DIR, "libntk_emu.so")
        src = os.path.join(EMU_DIR, "emu_scan.cpp")
        hdr = os.path.join(HERE, "..", "needletail_amd", "csrc", "ntk_tile.hpp")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.emu_minimizers.restype = C.c_int
        L.emu_minimizers.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.emu_minimizers_generic.restype = C.c_int
        L.emu_minimizers_generic.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.emu_minimizers_generic_quality.restype = C.c_int
        L.emu_minimizers_generic_quality.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int,
                                                     C.c_int, C.c_int, C.c_void_p]
        _EMU = L
    return _EMU


def _padded(buf: bytes, fill: bytes):
    n = len(buf)
    npad = (n + 15) // 16 * 16
    return np.frombuffer(buf + fill * (npad - n), dtype=np.uint8).copy(), n, npad


def _stats(out):
    return {"n_total": int(out[0]), "n_fwd": int(out[1]), "n_rc": int(out[0] - out[1]), "sum": int(out[2]), "xor": int(out[3]), "hist": out[4:].copy()}


def fused(L, buf, k, w, tie_rc, accept_u):
    arr, n, npad = _padded(buf, b"\xAA")   # garbage in the 16-byte padding
    out = np.zeros(4 + 4096, dtype=np.uint64)
    assert L.emu_minimizers(arr.ctypes.data, n, npad, k, w, tie_rc, accept_u, 1, out.ctypes.data) == 0, (k, w)   # 14-bit cells: the product's
    return _stats(out)


def generic(L, buf, k, w, tie_rc, accept_u, f64, qual: bytes = None):
    arr, n, npad = _padded(buf, b"\xAA")
    out = np.zeros(4 + 4096, dtype=np.uint64)
    if qual is None:
        rc = L.emu_minimizers_generic(arr.ctypes.data, n, npad, k, w, tie_rc, accept_u, f64, out.ctypes.data)
    else:
        q, _, _ = _padded(qual, b"\x7e")
        rc = L.emu_minimizers_generic_quality(arr.ctypes.data, q.ctypes.data, CUTOFF, n, npad, k, w, tie_rc, accept_u, f64, out.ctypes.data)
    assert rc == 0, (k, w, f64)
    return _stats(out)


def assert_stats_equal(a, b, ctx=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (ctx, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), ctx


def cases_and_wants(k, w, stride):
    cases = list(thin_far(min_seam_inputs(k, w, stride), k, w))
    wants = {rule: map_threads(lambda c: O.minimizers_reduce(c[1], k, w, accept_u=bool(rule[1]), tie_rc=bool(rule[0])), cases) for rule in RULES}
    return cases, wants


@pytest.mark.parametrize("k,w", FUSED_PAIRS)
def test_fused_builds_at_their_seams(emu, k, w):
    stride = min_stride(k, w, "fused")
    cases, wants = cases_and_wants(k, w, stride)
    for rule in RULES:
        for (tag, buf), want in zip(cases, wants[rule]):
            assert_stats_equal(fused(emu, buf, k, w, *rule), want, ("fused", k, w, stride, tag, rule))


@pytest.mark.parametrize("k,w", GENERIC_PAIRS + FUSED_PAIRS)
def test_generic_kernel_at_its_seams(emu, k, w):
    stride = min_stride(k, w, "generic")
    cases, wants = cases_and_wants(k, w, stride)
    for rule in RULES:
        for (tag, buf), want in zip(cases, wants[rule]):
            for f64 in ((0, 1) if k <= 25 else (0,)):
                assert_stats_equal(generic(emu, buf, k, w, *rule, f64), want, ("generic", k, w, stride, tag, rule, "f64" if f64 else "general keys"))


@pytest.mark.parametrize("k,w", GENERIC_PAIRS)
def test_generic_kernel_at_its_seams_quality_masked(emu, k, w):
    """The quality tile is loaded with the sequence tile's geometry: one low quality at every swept offset, no N anywhere."""
    stride = min_stride(k, w, "generic")
    cases = list(thin_far(min_seam_inputs(k, w, stride), k, w))
    base = cases[0][1]
    quals = []
    for tag, _ in cases:
        if tag[0] == "break":
            q = np.full(len(base), 70, dtype=np.uint8)
            q[tag[2]] = CUTOFF - 1
            quals.append((tag, q.tobytes()))
    wants = map_threads(lambda c: O.minimizers_reduce(O.quality_mask(base, c[1], CUTOFF), k, w, accept_u=True, tie_rc=True), quals)
    for (tag, q), want in zip(quals, wants):
        assert_stats_equal(generic(emu, base, k, w, 1, 1, 1 if k <= 25 else 0, qual=q), want, ("generic, quality", k, w, stride, tag))
