"""How alike are two samples?  ctypes binding of libneedletail_amd_minhash.so (include/needletail_amd_minhash.h).

KmerMinHash is a MinHash sketch of the keys a count table of the same k and path would insert, made from the same device batches:
bottom-s (`num`, mash / finch) or scaled (`scaled`, FracMinHash / sourmash), both with the exact abundance of every kept hash.
Sketches of several batches, GPUs or processes merge; two sketches compare by Jaccard, containment, cosine and Mash distance.  The
hash is this project's own (the k-mer sketch's), so sketches compare with each other, not with sourmash or mash files.  There is no
fallback: without a gfx950 device every call of the class raises; only compare(), which is host code on arrays that travelled, needs
none."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib as L
from .counting import upload_records
from .engine import Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_minhash.so")
PREFIX = "ntk_minhash_"

XOR = 0x9E3779B97F4A7C15      # NTK_MINHASH_XOR
MAX_NUM = 1 << 20             # NTK_MINHASH_MAX_NUM
BUFFER_DEFAULT = 1 << 22      # NTK_MINHASH_BUFFER_DEFAULT
BUFFER_MIN, BUFFER_MAX = 64, 1 << 28
ALL = (1 << 64) - 1


class Stats(C.Structure):
    _fields_ = [("n_windows", C.c_uint64), ("n_kept", C.c_uint64), ("threshold", C.c_uint64), ("num", C.c_uint64), ("scaled", C.c_uint64),
                ("buffer_entries", C.c_uint64), ("n_merges", C.c_uint64), ("n_redone", C.c_uint64), ("k", C.c_uint32), ("path", C.c_uint32)]


class Comparison(C.Structure):
    _fields_ = [("n_a", C.c_uint64), ("n_b", C.c_uint64), ("n_shared", C.c_uint64), ("n_union", C.c_uint64), ("dot", C.c_double),
                ("norm2_a", C.c_double), ("norm2_b", C.c_double)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the MinHash library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, _u32, _u64, _u64, _u64, C.POINTER(_vp)], "destroy": [_vp], "reset": [_vp],
    "add_device": [_vp, _vp, _vp, _u64, C.POINTER(L.Params)], "stats": [_vp, C.POINTER(Stats)],
    "read": [_vp, _vp, _vp, _u64, C.POINTER(_u64)], "merge": [_vp, _vp, _vp, _u64, _u64],
    "compare": [_vp, _vp, _u64, _vp, _vp, _u64, _u64, _u64, C.POINTER(Comparison)],
}

# every symbol include/needletail_amd_minhash.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The MinHash library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _u64_array(a, what: str):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint64 or a.ndim != 1:
        raise L.NtkError(2, f"{what} is a 1-d uint64 array, not {a.dtype}{list(a.shape)}")   # NTK_ERR_BAD_ARG
    return a


def _data(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def compare(a, ca, b, cb, num: int = 0, max_hash: int = ALL) -> dict:
    """ntk_minhash_compare on host arrays: strictly ascending uint64 hashes `a` and `b` with their counts `ca` and `cb` (None: every
    count 1).  Entries above max_hash are ignored; num = s takes the s smallest of the union (mash's rule).  Returns n_a, n_b,
    n_shared, n_union, dot, norm2_a, norm2_b; the ratios are the caller's (KmerMinHash.jaccard and the others)."""
    a, b, ca, cb = _u64_array(a, "a"), _u64_array(b, "b"), _u64_array(ca, "ca"), _u64_array(cb, "cb")
    if a is None or b is None or (ca is not None and ca.size != a.size) or (cb is not None and cb.size != b.size):
        raise L.NtkError(2, PREFIX + "compare")
    out = Comparison()
    L.check(lib().ntk_minhash_compare(_data(a), _data(ca), a.size, _data(b), _data(cb), b.size, num, max_hash, C.byref(out)),
            PREFIX + "compare")
    return {name: (float if t is C.c_double else int)(getattr(out, name)) for name, t in Comparison._fields_}


class KmerMinHash(L.Handle):
    """A MinHash sketch of the k-mers of `path` (a PATH_* constant): k = 1..32 on any path, k = 33..63 on PATH_BYTES_CANONICAL.
    Exactly one of `num` (bottom-s) and `scaled` (every hash <= (2^64 - 1) // scaled) is non-zero."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, k: int, path: int, num: int = 0, scaled: int = 0, ctx: Context = None, buffer_entries: int = 0):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path, self.num, self.scaled = k, path, num, scaled
        self.max_hash = ALL // scaled if scaled else ALL
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, k, path, num, scaled, buffer_entries, C.byref(self._h))

    def reset(self):
        self._check("reset", self._h)

    def add_device(self, d_seq, n_bytes: int, pre: int, d_qual=None, quality_cutoff: int = 0):
        """Add the k-mers of a device batch (the layout and rules of CountTable.count_device; may synchronise the context's stream)."""
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        self._check("add_device", self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.byref(p))

    def add_records(self, records, pre: int):
        """Pack the records with the batch packer (the route of CountTable.count_records), upload and add them."""
        up = upload_records(self.ctx, records, pre)
        if up is not None:
            self.add_device(up[0], up[1], pre)
            self.ctx.synchronize()

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def hashes(self):
        """(hashes, counts): the kept hashes, strictly ascending, and the number of k-mers behind each, as numpy uint64."""
        n = C.c_uint64(0)
        rc = lib().ntk_minhash_read(self._h, None, None, 0, C.byref(n))
        if rc not in (0, 5):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        h, c = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._check("read", self._h, h.ctypes.data, c.ctypes.data, n.value, C.byref(n))
        return h, c

    def merge(self, other, counts=None, n_windows: int = None):
        """Fold in another KmerMinHash of the same k and path, or bare (ascending) hashes with their counts (None: every count 1) and
        the exact number of k-mers behind them (`n_windows` is required then)."""
        if isinstance(other, KmerMinHash):
            if (other.k, other.path) != (self.k, self.path):
                raise L.NtkError(2, "merging sketches of different k or path")
            (hashes, counts), n_windows = other.hashes(), other.stats()["n_windows"]
        else:
            if n_windows is None:
                raise TypeError("merge(hashes, counts, n_windows): n_windows is required with bare arrays")
            if other is None:
                raise L.NtkError(2, PREFIX + "merge")
            hashes, counts = _u64_array(other, "hashes"), _u64_array(counts, "counts")
            if counts is not None and counts.size != hashes.size:
                raise L.NtkError(2, PREFIX + "merge")
        self._check("merge", self._h, _data(hashes), _data(counts), hashes.size, n_windows)

    def compare(self, other: "KmerMinHash") -> dict:
        """compare() of the two sketches: at the smaller of their max_hash, and by mash's rule when both are bottom-s sketches (num =
        the smaller of the two)."""
        if (other.k, other.path) != (self.k, self.path):
            raise L.NtkError(2, "comparing sketches of different k or path")
        if bool(self.num) != bool(other.num):
            raise L.NtkError(2, "comparing a bottom-s sketch with a scaled one")
        (a, ca), (b, cb) = self.hashes(), other.hashes()
        return compare(a, ca, b, cb, min(self.num, other.num), min(self.max_hash, other.max_hash))

    def jaccard(self, other: "KmerMinHash") -> float:
        c = self.compare(other)
        return c["n_shared"] / c["n_union"] if c["n_union"] else 0.0

    def containment(self, other: "KmerMinHash") -> float:
        """The share of this sketch's hashes that `other` holds too (meant for scaled sketches)."""
        c = self.compare(other)
        return c["n_shared"] / c["n_a"] if c["n_a"] else 0.0

    def cosine(self, other: "KmerMinHash") -> float:
        c = self.compare(other)
        d = math.sqrt(c["norm2_a"] * c["norm2_b"])
        return c["dot"] / d if d else 0.0

    def mash_distance(self, other: "KmerMinHash") -> float:
        j = self.jaccard(other)
        return 1.0 if j == 0 else max(0.0, -math.log(2.0 * j / (1.0 + j)) / self.k)
