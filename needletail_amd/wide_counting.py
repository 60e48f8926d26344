"""Exact counting of canonical k-mers with k = 33..63 on the device: ctypes binding of libneedletail_amd_wide_count.so
(include/needletail_amd_wide_count.h).

WideKmerTable counts the canonical k-mers of the byte path (normalize -> canonical_kmers(k, &rc)) in a hash table in device memory and
answers with the sorted (k-mer, count) pairs, the abundance spectrum and point lookups.  A key is two u64 words [hi, lo]: hi = the first
k - 32 bases, lo = the last 32, in the 2-bit code (A 0, C 1, G 2, T 3, first base most significant).  There is no fallback: without a
gfx950 device every call raises."""
from __future__ import annotations

import os

import numpy as np

from . import _lib as L
from .counting import CALLS, CountTable

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_wide_count.so")
PREFIX = "ntk_wide_table_"

# every symbol include/needletail_amd_wide_count.h declares
SYMBOLS = [PREFIX + c for c in CALLS]

K_MIN, K_MAX = 33, 63


def lib():
    return L.load(LIB_PATH, PREFIX, CALLS)


_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c + 32] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3


def encode(kmers, k: int) -> np.ndarray:
    """k-mers given as str / bytes (ACGTU in either case) -> an (n, 2) uint64 array of [hi, lo] rows."""
    out = np.zeros((len(kmers), 2), dtype=np.uint64)
    for i, x in enumerate(kmers):
        if isinstance(x, str):
            x = x.encode()
        if len(x) != k:
            raise ValueError(f"k-mer of length {len(x)} in a k = {k} table")
        c = _CODE[np.frombuffer(bytes(x), dtype=np.uint8)]
        if (c == 255).any():
            raise ValueError(f"not a base in {bytes(x)!r}")
        hi = lo = 0
        for v in c[: k - 32]:
            hi = (hi << 2) | int(v)
        for v in c[k - 32:]:
            lo = (lo << 2) | int(v)
        out[i] = (hi, lo)
    return out


def decode(keys, k: int) -> list:
    """[hi, lo] rows -> k-mers as bytes."""
    out = []
    for hi, lo in np.asarray(keys, dtype=np.uint64).reshape(-1, 2):
        v = (int(hi) << 64) | int(lo)
        out.append(bytes(b"ACGT"[(v >> (2 * (k - 1 - j))) & 3] for j in range(k)))
    return out


class WideKmerTable(CountTable):
    """An exact count table of canonical k-mers, k = K_MIN..K_MAX (33..63), on PATH_BYTES_CANONICAL, sized for `capacity` distinct
    k-mers.

    The methods are KmerTable's; keys are (n, 2) uint64 arrays of [hi, lo] rows.  items() returns them ascending as 2k-bit values.
    lookup() takes k-mers as str / bytes (either strand) or as an (n, 2) array of [hi, lo] rows (canonicalised by the library); one
    k-mer given as str / bytes reads an int."""

    _lib, _prefix, _key_words = staticmethod(lib), PREFIX, 2

    def _queries(self, kmers):
        if isinstance(kmers, (bytes, bytearray, str)):
            return True, encode([kmers], self.k)
        if isinstance(kmers, np.ndarray) and kmers.dtype != object:
            return False, np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, 2)
        return False, encode(list(kmers), self.k)
