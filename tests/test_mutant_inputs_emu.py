"""The inputs of tests/_mutant_inputs.py (and _seams.lower_tail_lengths) through the lock-step emulation of the per-lane source against the
oracle, on the CPU.  Each input was added for a small wrong edit of csrc/ntk_tile.hpp that the mutation audit (tools/mutation_audit.py) found
passing every earlier test; profiles/mutation_audit/README.md lists them.  Every test also shows that its input is not vacuous: the oracle's
own result changes under the reading the wrong edit would take.  The same inputs run on the device in test_gpu_minimizer_seams.py
(scan_kernel through the two-pass route, minimizer_scan_kernel), test_gpu_build_matrix.py (scan_kernel's own planes), test_gpu_wide_seams.py and
test_gpu_lower_watch.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O

from _mutant_inputs import SCAN_STRIDE, TAIL_FILL, WIDE_TILE, palindrome_kmer_inputs, tail_input, tail_plane_words
from _seams import lower_tail_lengths, min_stride, wide_input, wide_reference

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
        L.emu_scan.restype = C.c_int
        L.emu_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 4
        L.emu_minimizers_generic.restype = C.c_int
        L.emu_minimizers_generic.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.emu_wide_reduce.restype = C.c_int
        L.emu_wide_reduce.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
        _EMU = L
    return _EMU


def _padded(buf: bytes, fill: bytes):
    n = len(buf)
    npad = (n + 15) // 16 * 16
    return np.frombuffer(buf + fill * (npad - n), dtype=np.uint8).copy(), n, npad


def _stats(out):
    return {"n_total": int(out[0]), "n_fwd": int(out[1]), "n_rc": int(out[0] - out[1]), "sum": int(out[2]), "xor": int(out[3]), "hist": out[4:].copy()}


def scan(L, buf, k, canon, tie_rc, accept_u, fill):
    """scan_kernel's per-lane source (lane_tile), the plain build: tiles_per_wave = 2 selects neither the k-specialised nor the sv2 variants."""
    arr, n, npad = _padded(buf, fill)
    out = np.zeros(4 + 4096, dtype=np.uint64)
    assert L.emu_scan(arr.ctypes.data, n, npad, k, canon, tie_rc, accept_u, 2, out.ctypes.data, None, None, None) == 0
    return _stats(out)


def generic(L, buf, k, w, tie_rc, accept_u, f64, fill):
    arr, n, npad = _padded(buf, fill)
    out = np.zeros(4 + 4096, dtype=np.uint64)
    assert L.emu_minimizers_generic(arr.ctypes.data, n, npad, k, w, tie_rc, accept_u, f64, out.ctypes.data) == 0
    return _stats(out)


def wide(L, buf, k, accept_u, fill):
    arr, n, npad = _padded(buf, fill)
    out = np.zeros(4 + 4096, dtype=np.uint64)
    assert L.emu_wide_reduce(arr.ctypes.data, n, npad, k, int(accept_u), out.ctypes.data) == 0
    return {"n_total": int(out[0]), "n_fwd": int(out[1]), "ties": int(out[2]), "bit5": int(out[3]), "hist": out[4:].copy()}


def assert_stats_equal(a, b, ctx=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (ctx, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), ctx


# ---- a last line of 15 input bytes with a base behind them -----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 16, 22, 32])
def test_scan_ignores_a_base_in_the_padding(emu, k):
    buf = tail_input(SCAN_STRIDE)
    assert len(buf) % 16 == 15
    for canon, tie_rc, accept_u in ((1, 1, 1), (1, 0, 0), (0, 0, 0)):
        want = O.reduce_fused(buf, k, bool(canon), bool(tie_rc), bool(accept_u))
        assert O.reduce_fused(buf + TAIL_FILL, k, bool(canon), bool(tie_rc), bool(accept_u))["n_total"] == want["n_total"] + 1   # not vacuous
        assert_stats_equal(scan(emu, buf, k, canon, tie_rc, accept_u, TAIL_FILL), want, ("lane_tile", k, canon, tie_rc, accept_u))


@pytest.mark.parametrize("k", [5, 16, 21, 22, 32])
def test_scan_planes_ignore_a_base_in_the_padding(emu, k):
    """The same input into the materialising sink, whose valid16 word is ~inval as lane_tile leaves it, unclipped: the last word's bit 0 is
    position n, the padding byte.  A reduction over the planes reads positions below n only, so it cannot see that bit; the word itself can
    (the device twin is test_gpu_build_matrix.py::test_materialize_ignores_a_base_in_the_padding).  fix: k = 21 takes its own build."""
    buf = tail_input(SCAN_STRIDE)
    n = len(buf)
    arr, _, npad = _padded(buf, TAIL_FILL)
    assert n % 16 == 15 and npad == n + 1
    for canon, tie_rc, accept_u in ((1, 1, 1), (1, 0, 0), (0, 0, 0)):
        want_v, want_r = tail_plane_words(buf, k, bool(canon), bool(tie_rc))
        assert tail_plane_words(buf + TAIL_FILL, k, bool(canon), bool(tie_rc))[0][-1] == want_v[-1] | 1   # not vacuous: the reading that takes the byte
        out = np.zeros(4 + 4096, dtype=np.uint64)
        v16, r16 = np.full(npad // 16, 0x5A5A, dtype=np.uint16), np.full(npad // 16, 0x5A5A, dtype=np.uint16)
        assert emu.emu_scan(arr.ctypes.data, n, npad, k, canon, tie_rc, accept_u, 1, out.ctypes.data, None, v16.ctypes.data, r16.ctypes.data) == 0
        assert v16[-1] & 1 == 0, ("the window ending on the padding byte is marked valid", k, canon, tie_rc, hex(v16[-1]))
        assert np.array_equal(v16, want_v) and np.array_equal(r16, want_r), (k, canon, tie_rc, accept_u)


@pytest.mark.parametrize("k,w", [(21, 11), (24, 11), (26, 18), (11, 49)])
def test_generic_minimizers_ignore_a_base_in_the_padding(emu, k, w):
    """Both smear forms of minimizer_invalid16 (k + w - 1 <= 49 and beyond), both key forms."""
    buf = tail_input(min_stride(k, w, "generic"))
    assert len(buf) % 16 == 15
    for tie_rc, accept_u in ((1, 1), (0, 0)):
        want = O.minimizers_reduce(buf, k, w, accept_u=bool(accept_u), tie_rc=bool(tie_rc))
        assert O.minimizers_reduce(buf + TAIL_FILL, k, w, accept_u=bool(accept_u), tie_rc=bool(tie_rc))["n_total"] == want["n_total"] + 1
        for f64 in ((0, 1) if k <= 25 else (0,)):
            assert_stats_equal(generic(emu, buf, k, w, tie_rc, accept_u, f64, TAIL_FILL), want, ("minimizer_invalid16", k, w, tie_rc, f64))


@pytest.mark.parametrize("k", [33, 64, 255])
def test_wide_k_ignores_a_base_in_the_padding(emu, k):
    buf = tail_input(WIDE_TILE + 256)
    assert len(buf) % 16 == 15
    want = wide_reference(buf, k)
    assert wide_reference(buf + TAIL_FILL, k)["n_total"] == want["n_total"] + 1
    for accept_u in (False, True):
        got = wide(emu, buf, k, accept_u, TAIL_FILL)
        assert got["ties"] == 0 and got["bit5"] == 0, (k, accept_u)
        assert (got["n_total"], got["n_fwd"]) == (want["n_total"], want["n_fwd"]) and np.array_equal(got["hist"], want["hist"]), (k, accept_u)


# ---- a k-mer that is its own reverse complement ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [18, 22, 32, 4, 16])
def test_scan_reports_a_self_palindrome_by_the_paths_tie_rule(emu, k):
    """lane_tile's compare, one word (k <= 16) and two (k >= 17): the byte path reports the reverse complement on a tie, the bit path the
    forward strand.  The k-mer ends mid-tile, on both sides of the 992-byte seam and of a lane boundary."""
    for e, buf in palindrome_kmer_inputs(k):
        byte_path = O.reduce_fused(buf, k, True, True, True)
        bit_path = O.reduce_fused(buf, k, True, False, False)
        assert byte_path["n_rc"] > bit_path["n_rc"] and byte_path["n_total"] == bit_path["n_total"]   # the tie is there, and it shows
        assert_stats_equal(scan(emu, buf, k, 1, 1, 1, b"\xAA"), byte_path, ("lane_tile, byte path", k, e))
        assert_stats_equal(scan(emu, buf, k, 1, 0, 0, b"\xAA"), bit_path, ("lane_tile, bit path", k, e))


# ---- the last input byte at offsets 3, 4, 5, 14, 15, 16 of its line, lower case behind it ----------------------------------------------

@pytest.mark.parametrize("k", [33, 255])
def test_lower_case_padding_is_not_watched_and_the_last_byte_is(emu, k):
    """or_of_input_bytes through wk_stage_slot (the ACCEPT_U = false build watches bit 5): a dword that holds exactly its four input bytes,
    one more, a line with one byte of padding, a full line, one byte in a line of its own."""
    a = wide_input()
    for off, n in lower_tail_lengths(len(a)):
        head = a[:n].copy()
        assert (n - 1) % 16 == off % 16
        assert wide(emu, head.tobytes(), k, False, b"a")["bit5"] == 0, (k, off, "all upper case, lower case in the padding")
        head[n - 1] |= 0x20
        assert wide(emu, head.tobytes(), k, False, b"a")["bit5"] == 1, (k, off, "the last byte lower case")
