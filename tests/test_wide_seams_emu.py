"""CanonicalKmers with k = 33..255 at the row, wave and tile seams of wide_canonical_reduce_kernel, on the CPU: the numpy restatement the
device sweep (test_gpu_wide_seams.py) compares with is pinned against the oracle's literal iterator; the inserts of the device sweep's tie
cases are shown to tie over 32 bases (and, with one base changed, not to); and the break sweep - one N at every offset of
[seam - k - 18, seam + 18] around 256, 1024, 4096, 4096 + 256, 4096 + 1024 and 8192 - runs through the per-slot functions of ntk_tile.hpp
(emu_wide_reduce: tile by tile, the block's max-scan of break positions as a running maximum; the DPP scan and its LDS fold are device
code and run in the device sweep only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O

from _seams import (WIDE_KS, WIDE_SEAMS, WIDE_TIE_KS, wide_break_offsets, wide_input, wide_reference, wide_tie_insert, wide_tie_starts)

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")

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
        L.emu_wide_reduce.restype = C.c_int
        L.emu_wide_reduce.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
        _EMU = L
    return _EMU


def emu_wide(L, buf: bytes, k, accept_u):
    n = len(buf)
    npad = (n + 15) // 16 * 16
    arr = np.frombuffer(buf + b"\xAA" * (npad - n), dtype=np.uint8).copy()   # garbage in the 16-byte padding: beyond n everything is a break
    out = np.zeros(4 + 4096, dtype=np.uint64)
    assert L.emu_wide_reduce(arr.ctypes.data, n, npad, k, int(accept_u), out.ctypes.data) == 0
    return {"n_total": int(out[0]), "n_fwd": int(out[1]), "ties": int(out[2]), "bit5": int(out[3]), "hist": out[4:].copy()}


def _wide_reference(recs, k, normalized):
    """CanonicalKmers with 33 <= k <= 255 per record through the oracle's literal iterator: counters + the histogram of the leading six bases
    of every emitted slice (as tests/test_gpu_parity.py holds it for the GPU)."""
    code = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i; code[ch | 0x20] = i
    st = {"n_total": 0, "n_fwd": 0, "hist": np.zeros(4096, dtype=np.uint64)}
    for r in recs:
        if normalized:
            r = O.normalize(r)[0]
        rc = O.reverse_complement(r)
        pos, flg = O.canonical_kmers_arrays(r, rc, k)
        for p, f in zip(pos.tolist(), flg.tolist()):
            sl = rc[len(rc) - p - k: len(rc) - p] if f else r[p: p + k]
            b = 0
            for ch in sl[:6]:
                b = b * 4 + int(code[ch])
            st["hist"][b] += 1
        st["n_total"] += len(pos); st["n_fwd"] += len(pos) - int(flg.sum())
    return st


def same(a, b):
    return (a["n_total"], a["n_fwd"]) == (b["n_total"], b["n_fwd"]) and np.array_equal(a["hist"], b["hist"])


@pytest.mark.parametrize("k", sorted(set(WIDE_KS + WIDE_TIE_KS)))
def test_numpy_reference_is_the_literal_iterator(k):
    """On the unbroken input, on one broken case per seam (the break k // 2 before it: the windows it removes lie on both sides), and on
    the tie insert across the first tile seam (a k-mer equal to its reverse complement over 32 bases, or all k of them)."""
    base = wide_input()
    inputs = [("none", base.tobytes())]
    for S in WIDE_SEAMS:
        a = base.copy()
        a[S - k // 2] = ord("N")
        inputs.append((("break", S), a.tobytes()))
    a = base.copy()
    a[4096 - k // 2: 4096 - k // 2 + k] = np.frombuffer(wide_tie_insert(k), dtype=np.uint8)
    inputs.append(("tie", a.tobytes()))
    for tag, buf in inputs:
        for normalized in (False, True):   # (upper-case ACGT and N: the two readings agree)
            assert same(wide_reference(buf, k), _wide_reference(buf.split(b"N"), k, normalized)), (k, tag, normalized)
    assert wide_reference(b"ACGT" * 5, k)["n_total"] == 0


@pytest.mark.parametrize("k", WIDE_TIE_KS)
def test_tie_inserts_tie_over_32_bases(emu, k):
    ins = np.frombuffer(wide_tie_insert(k), dtype=np.uint8)
    assert ins[:32].tobytes() == O.reverse_complement(ins[-32:].tobytes())
    base = wide_input()
    assert emu_wide(emu, base.tobytes(), k, True)["ties"] == 0
    changed = ins.copy()
    changed[5] = ord("C") if changed[5] != ord("C") else ord("G")
    for S, p in wide_tie_starts(k):
        a = base.copy()
        a[p: p + k] = ins
        got = emu_wide(emu, a.tobytes(), k, True)
        assert got["ties"] > 0, (k, S, p)
        a[p: p + k] = changed
        got = emu_wide(emu, a.tobytes(), k, True)
        assert got["ties"] == 0 and same(got, wide_reference(a.tobytes(), k)), (k, S, p)


@pytest.mark.parametrize("k", WIDE_KS)
def test_breaks_around_row_wave_and_tile_seams(emu, k):
    base = wide_input()
    assert same(emu_wide(emu, base.tobytes(), k, False), wide_reference(base.tobytes(), k))
    for S, off in wide_break_offsets(k):
        a = base.copy()
        a[off] = ord("N")
        buf = a.tobytes()
        want = wide_reference(buf, k)
        for accept_u in (False, True):
            got = emu_wide(emu, buf, k, accept_u)
            assert got["ties"] == 0 and got["bit5"] == 0 and same(got, want), (k, S, off, accept_u)
