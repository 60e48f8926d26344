"""Two exact count tables against each other.  ctypes binding of libneedletail_amd_kmer_sets.so (include/needletail_amd_kmer_sets.h).

KmerSet is a k-mer list resident on the device: strictly ascending keys with their counts, what a count table's extract writes.  Two
sets are joined on the GPU in one streaming pass: intersect / union / subtract / counters_subtract give a KmerSet again, compare gives
the joint spectrum (how many k-mers occur a times here and b times there) with exact integer totals, and the usual numbers are read
from those: Jaccard, containment, weighted Jaccard, Bray-Curtis, Merqury's QV and k-mer completeness.  The only floating-point step is
the last division, here in Python.  There is no fallback: without a gfx950 device every call of the class raises."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib as L
from .engine import Context, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_kmer_sets.so")
PREFIX = "ntk_kmer_sets_"

TILE_WORDS = 2048                                            # NTK_KSET_TILE_WORDS
MAX_BINS = 16384                                             # NTK_KSET_MAX_BINS
INTERSECT, UNION, SUBTRACT, COUNTERS_SUBTRACT = 1, 2, 3, 4   # NTK_KSET_* ops
MIN, MAX, SUM, LEFT, RIGHT = 1, 2, 3, 4, 5                   # NTK_KSET_* rules
RULES = {"min": MIN, "max": MAX, "sum": SUM, "left": LEFT, "right": RIGHT}
NTK_ERR_CAPACITY = 5


class Stats(C.Structure):
    _fields_ = [("key_words", C.c_uint64), ("device_bytes", C.c_uint64), ("n_launches", C.c_uint64), ("n_calls", C.c_uint64)]


class Totals(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("n_a", "n_b", "n_shared", "n_a_only", "n_b_only", "sum_a", "sum_b", "sum_a_shared",
                                                "sum_b_shared", "sum_a_only", "sum_b_only", "sum_min", "sum_max")]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, C.POINTER(_vp)], "destroy": [_vp], "release": [_vp], "stats": [_vp, C.POINTER(Stats)],
    "validate_device": [_vp, _vp, _u64, C.POINTER(_u64)],
    "compare_device": [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u32, _vp, C.POINTER(Totals)],
    "apply_device": [_vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64)],
}

# every symbol include/needletail_amd_kmer_sets.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _rule(rule) -> int:
    if isinstance(rule, str):
        if rule not in RULES:
            raise ValueError(f"rule {rule!r} not in {sorted(RULES)}")
        return RULES[rule]
    return int(rule)


def _ratio(num: int, den: int) -> float:
    return num / den if den else 0.0


class KmerSet(L.Handle):
    """A k-mer list on the device: `keys` (a torch int64 tensor holding the uint64 words, key_words per key) and `counts`, n entries,
    keys strictly ascending.  Make one with from_table or from_arrays; the operations return new sets and leave their inputs alone."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, keys, counts, n: int, k: int, path: int, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path, self.n = int(k), path, int(n)
        if not 1 <= self.k <= 63:
            raise L.NtkError(1, "a k-mer list holds k = 1..63")
        self.key_words = 1 if self.k <= 32 else 2
        self.keys, self.counts = keys, counts
        self._h = C.c_void_p()   # the native handle (the joins' scratch): made by the first call that needs one

    def _native(self):
        """The native handle, created on first use: a set that is only an operand or a result never allocates one."""
        if not self._h:
            self._check("create", self.ctx._h, self.key_words, C.byref(self._h))
        return self._h

    # -- making one ----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_table(cls, table, min_count: int = 1) -> "KmerSet":
        """The entries of a KmerTable or WideKmerTable with count >= min_count, extracted on the device and kept there."""
        import torch
        # counting.py offers items(), which copies to the host, and no device-resident read; so this goes to the table's extract_device
        # call through the CountTable internals (_fn, _h, _key_words, _prefix) and repeats items()'s size query
        n = C.c_uint64(0)
        extract = table._fn("extract_device")
        rc = extract(table._h, min_count, None, None, 0, C.byref(n))
        if rc not in (L.NTK_OK, NTK_ERR_CAPACITY) or (rc == NTK_ERR_CAPACITY and n.value == 0):
            L.check(rc, table._prefix + "extract_device")
        need, w = int(n.value), table._key_words
        dev = f"cuda:{table.ctx.device}"
        keys, counts = torch.empty(max(w * need, 1), dtype=torch.int64, device=dev), torch.empty(max(need, 1), dtype=torch.int64, device=dev)
        if need:
            table._check("extract_device", table._h, min_count, C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()), need, C.byref(n))
        return cls(keys, counts, need, table.k, table.path, table.ctx)

    @classmethod
    def from_arrays(cls, keys, counts, k: int, path: int = L.PATH_BYTES_CANONICAL, ctx: Context = None) -> "KmerSet":
        """From host arrays in any order: keys of shape (n,) for k <= 32 or (n, 2) [hi, lo] rows for k = 33..63, and their counts.  Sorted
        on the host, uploaded, and validated on the device: a key given twice is an error."""
        import torch
        ctx = ctx if ctx is not None else default_context()
        w = 1 if k <= 32 else 2
        keys, counts = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, w), np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        if keys.shape[0] != counts.size:
            raise L.NtkError(2, "from_arrays: one count per key")
        order = np.lexsort((keys[:, 1], keys[:, 0])) if w == 2 else np.argsort(keys[:, 0], kind="stable")
        dev = f"cuda:{ctx.device}"
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.int64).copy()).to(dev) if v.size else \
            torch.empty(1, dtype=torch.int64, device=dev)
        s = cls(up(keys[order]), up(counts[order]), counts.size, k, path, ctx)
        torch.cuda.synchronize(dev)
        if s.violations():
            raise L.NtkError(2, "from_arrays: a key is given twice")
        return s

    # -- reading -------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return self.n

    def items(self):
        """(keys, counts) as numpy uint64 arrays, keys ascending: values for k <= 32, [hi, lo] rows for k = 33..63."""
        w = self.key_words
        keys = self.keys[: w * self.n].cpu().numpy().view(np.uint64)
        return (keys if w == 1 else keys.reshape(-1, 2)), self.counts[: self.n].cpu().numpy().view(np.uint64)

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._native(), C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def release(self):
        """Free the scratch the joins of this set grew."""
        self._check("release", self._native())

    def _list(self):
        """(keys pointer, counts pointer, n) as the calls take a list: NULL arrays for an empty one."""
        if self.n == 0:
            return None, None, 0
        return C.c_void_p(self.keys.data_ptr()), C.c_void_p(self.counts.data_ptr()), self.n

    def violations(self) -> int:
        """Adjacent pairs of keys that do not ascend strictly: 0 on every set this module makes."""
        v = C.c_uint64(0)
        self._check("validate_device", self._native(), self._list()[0], self.n, C.byref(v))
        return v.value

    # -- two sets ------------------------------------------------------------------------------------------------------------
    def _admit(self, other: "KmerSet"):
        if not isinstance(other, KmerSet):
            raise TypeError("a KmerSet is joined with a KmerSet")
        if (other.k, other.path) != (self.k, self.path):
            raise L.NtkError(2, "joining k-mer sets of a different k or path")
        if other.ctx is not self.ctx:
            raise L.NtkError(2, "joining k-mer sets of two contexts")

    def _apply(self, op: int, rule: int, other: "KmerSet", bound: int) -> "KmerSet":
        import torch
        self._admit(other)
        dev, w = self.keys.device, self.key_words
        keys, counts = torch.empty(max(w * bound, 1), dtype=torch.int64, device=dev), torch.empty(max(bound, 1), dtype=torch.int64, device=dev)
        n = C.c_uint64(0)
        out = (C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr())) if bound else (None, None)
        torch.cuda.synchronize(dev)   # the inputs may have been written on torch's stream
        self._check("apply_device", self._native(), op, rule, *self._list(), *other._list(), *out, bound, C.byref(n))
        got = int(n.value)
        if 2 * got < bound:   # do not pin a buffer sized for the bound behind a small result
            keys, counts = keys[: max(w * got, 1)].clone(), counts[: max(got, 1)].clone()
        return KmerSet(keys, counts, got, self.k, self.path, self.ctx)

    def intersect(self, other: "KmerSet", rule="min") -> "KmerSet":
        """Keys in both, each with `rule` ("min", "max", "sum", "left", "right") of its two counts."""
        return self._apply(INTERSECT, _rule(rule), other, min(self.n, other.n))

    def union(self, other: "KmerSet", rule="sum") -> "KmerSet":
        """Keys in either; one in both gets `rule` of its two counts ("sum" saturates at 2^64 - 1), one in a single set keeps its count."""
        return self._apply(UNION, _rule(rule), other, self.n + other.n)

    def subtract(self, other: "KmerSet") -> "KmerSet":
        """Keys of this set that `other` lacks, with their counts."""
        return self._apply(SUBTRACT, 0, other, self.n)

    def counters_subtract(self, other: "KmerSet") -> "KmerSet":
        """Keys of this set whose count exceeds `other`'s (0 where it lacks the key), with the difference."""
        return self._apply(COUNTERS_SUBTRACT, 0, other, self.n)

    def compare(self, other: "KmerSet", bins_a: int = 256, bins_b: int = 8):
        """(hist, totals): hist[a, b] = distinct k-mers with min(count here, bins_a - 1) == a and min(count in `other`, bins_b - 1) == b
        (an absent k-mer counts 0; hist[0, 0] is 0), a uint64 array of shape (bins_a, bins_b); totals: a dict of exact integers (see
        struct ntk_kmer_sets_totals; sums are modulo 2^64)."""
        import torch
        self._admit(other)
        if bins_a < 2 or bins_b < 2 or bins_a * bins_b > MAX_BINS:
            raise L.NtkError(2, f"compare: bins_a and bins_b are each >= 2 and their product is at most {MAX_BINS}")
        hist, t = np.zeros((bins_a, bins_b), dtype=np.uint64), Totals()
        torch.cuda.synchronize(self.keys.device)
        self._check("compare_device", self._native(), *self._list(), *other._list(), bins_a, bins_b, hist.ctypes.data, C.byref(t))
        return hist, {name: int(getattr(t, name)) for name, _ in Totals._fields_}

    def totals(self, other: "KmerSet") -> dict:
        return self.compare(other, 2, 2)[1]

    # -- the numbers read from the totals ------------------------------------------------------------------------------------
    def jaccard(self, other: "KmerSet") -> float:
        return jaccard(self.totals(other))

    def containment(self, other: "KmerSet") -> float:
        """The share of this set's k-mers that `other` holds too."""
        return containment(self.totals(other))

    def weighted_jaccard(self, other: "KmerSet") -> float:
        return weighted_jaccard(self.totals(other))

    def bray_curtis(self, other: "KmerSet") -> float:
        return bray_curtis(self.totals(other))


def jaccard(t: dict) -> float:
    return _ratio(t["n_shared"], t["n_a"] + t["n_b"] - t["n_shared"])


def containment(t: dict) -> float:
    return _ratio(t["n_shared"], t["n_a"])


def weighted_jaccard(t: dict) -> float:
    return _ratio(t["sum_min"], t["sum_max"])


def bray_curtis(t: dict) -> float:
    """The Bray-Curtis dissimilarity 1 - 2 sum_min / (sum_a + sum_b); 0.0 for two empty sets."""
    den = t["sum_a"] + t["sum_b"]
    return 1.0 - 2.0 * t["sum_min"] / den if den else 0.0


def merqury_qv(reads: KmerSet, assembly: KmerSet, k: int = None) -> float:
    """Merqury's consensus quality value: e = the share of the assembly's k-mer instances that the reads lack,
    p = (1 - e)^(1/k), QV = -10 log10(1 - p); inf for e = 0."""
    t = reads.totals(assembly)
    k = reads.k if k is None else k
    if t["sum_b_only"] == 0:
        return math.inf
    p = (1.0 - t["sum_b_only"] / t["sum_b"]) ** (1.0 / k)
    return -10.0 * math.log10(1.0 - p)


def completeness(reads_solid: KmerSet, assembly: KmerSet) -> float:
    """Merqury's k-mer completeness: the share of the reads' solid k-mers found in the assembly."""
    t = reads_solid.totals(assembly)
    return _ratio(t["n_shared"], t["n_a"])
