"""Screen reads against many references: ctypes binding of libneedletail_amd_colors.so (include/needletail_amd_colors.h).

KmerColors is a coloured k-mer index on the device: every k-mer maps to the set of references ("colours", at most 64) that hold it.
add() puts a KmerSet (or a KmerTable) in under one colour; run_device() goes over a device batch once and returns, per record, how
many of its k-mers every colour holds (hits), how many it holds alone (single), and a row with n_kmers, n_hit, n_single, best and
second.  Everything is exact integers and stays on the device; classify() is the host helper that turns rows into a colour per record.
There is no fallback: without a gfx950 device every call raises.  k = 33..63 is not served."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .counting import KmerTable, upload_records_with_offsets
from .engine import Context, _ptr, default_context
from .kmer_sets import KmerSet
from .wide_counting import WideKmerTable

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_colors.so")
PREFIX = "ntk_kmer_colors_"

COLORS_MAX = 64                  # NTK_COLORS_MAX
NONE = (1 << 64) - 1             # NTK_COLORS_NONE
# the words of a row (struct ntk_kmer_colors_row), in order
COLUMNS = ("n_kmers", "n_hit", "n_single", "best", "second")


class Stats(C.Structure):
    _fields_ = [("n_keys", C.c_uint64), ("n_dropped", C.c_uint64), ("n_masked_bits", C.c_uint64), ("slots", C.c_uint64),
                ("device_bytes", C.c_uint64), ("n_launches", C.c_uint64), ("per_color", C.c_uint64 * 64),
                ("n_colors", C.c_uint32), ("k", C.c_uint32), ("path", C.c_uint32), ("reserved", C.c_uint32)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, _u32, _u32, _u64, C.POINTER(_vp)], "destroy": [_vp], "reset": [_vp],
    "add_device": [_vp, _vp, _vp, _u64, _u64], "stats": [_vp, C.POINTER(Stats)], "lookup_device": [_vp, _vp, _u64, _vp],
    "run_device": [_vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(L.Params), _vp, _vp, _vp], "release": [_vp],
}

# every symbol include/needletail_amd_colors.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _u64_tensor(values, device):
    import torch
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    if v.size == 0:
        return torch.empty(1, dtype=torch.int64, device=device)
    return torch.from_numpy(v.view(np.int64).copy()).to(device)


class KmerColors(L.Handle):
    """A coloured k-mer index of k-mers (k = 1..32) on `path` for `n_colors` (1..64) references, sized for `capacity` distinct k-mers."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, k: int, path: int, n_colors: int, capacity: int, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path, self.n_colors = int(k), path, int(n_colors)
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, self.k, path, self.n_colors, capacity, C.byref(self._h))

    @property
    def _device(self) -> str:
        return f"cuda:{self.ctx.device}"

    # -- building --------------------------------------------------------------------------------------------------------------
    def add(self, source, color: int, min_count: int = 1):
        """Add the k-mers of `source` under `color`: a KmerSet, or a KmerTable (its entries with count >= min_count).  Returns when they
        are in: the list may go at once."""
        import torch
        if isinstance(source, WideKmerTable):
            raise L.NtkError(1, "a coloured index holds k = 1..32")
        if isinstance(source, KmerTable):
            source = KmerSet.from_table(source, min_count)
        if not isinstance(source, KmerSet):
            raise TypeError(f"KmerColors.add takes a KmerSet or a KmerTable, not {type(source).__name__}")
        if source.k > 32 or source.key_words != 1:
            raise L.NtkError(1, "a coloured index holds k = 1..32")
        if (source.k, source.path) != (self.k, self.path):
            raise L.NtkError(2, "adding a k-mer set of a different k or path")
        if not 0 <= color < self.n_colors:
            raise L.NtkError(2, f"colour {color} in an index of {self.n_colors}")
        if source.n == 0:
            return
        torch.cuda.synchronize(source.keys.device)   # the list may have been written on torch's stream
        self._check("add_device", self._h, C.c_void_p(source.keys.data_ptr()), None, 1 << color, source.n)
        self.ctx.synchronize()

    def add_masks(self, keys, masks):
        """OR masks[i] into the entry of keys[i]: device int64 tensors holding the uint64 words, or host arrays (uploaded)."""
        import torch
        n = int(keys.numel()) if hasattr(keys, "numel") else int(np.size(keys))
        if n != (int(masks.numel()) if hasattr(masks, "numel") else int(np.size(masks))):
            raise L.NtkError(2, "add_masks: one mask per key")
        if n == 0:
            return
        if not hasattr(keys, "data_ptr"):
            keys = _u64_tensor(keys, self._device)
        if not hasattr(masks, "data_ptr"):
            masks = _u64_tensor(masks, self._device)
        torch.cuda.synchronize(keys.device)
        self._check("add_device", self._h, C.c_void_p(keys.data_ptr()), C.c_void_p(masks.data_ptr()), 0, n)
        self.ctx.synchronize()   # the tensors may go once this returns

    @classmethod
    def from_sets(cls, sets, ctx: Context = None) -> "KmerColors":
        """An index with one colour per KmerSet of `sets`, in their order; its capacity is the sum of their lengths."""
        sets = list(sets)
        if not sets or not all(isinstance(s, KmerSet) for s in sets):
            raise TypeError("from_sets takes a non-empty list of KmerSet")
        if any(s.k > 32 for s in sets):
            raise L.NtkError(1, "a coloured index holds k = 1..32")
        if any((s.k, s.path) != (sets[0].k, sets[0].path) for s in sets):
            raise L.NtkError(2, "k-mer sets of a different k or path in one index")
        kc = cls(sets[0].k, sets[0].path, len(sets), max(sum(s.n for s in sets), 1), ctx if ctx is not None else sets[0].ctx)
        for color, s in enumerate(sets):
            kc.add(s, color)
        return kc

    def reset(self):
        self._check("reset", self._h)

    def release(self):
        """Free the scratch run_device grew; the index stays."""
        self._check("release", self._h)

    # -- reading ---------------------------------------------------------------------------------------------------------------
    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        out = {name: int(getattr(s, name)) for name, _ in Stats._fields_ if name not in ("per_color", "reserved")}
        out["per_color"] = [int(v) for v in s.per_color][: self.n_colors]
        return out

    def lookup(self, keys) -> np.ndarray:
        """The masks of packed k-mer values (taken as given), 0 where absent: a numpy uint64 array."""
        import torch
        v = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        dq = _u64_tensor(v, self._device)
        dm = torch.empty(max(v.size, 1), dtype=torch.int64, device=self._device)
        torch.cuda.synchronize(dq.device)
        self._check("lookup_device", self._h, C.c_void_p(dq.data_ptr()), v.size, C.c_void_p(dm.data_ptr()))
        return dm[: v.size].cpu().numpy().view(np.uint64)

    # -- the screen ------------------------------------------------------------------------------------------------------------
    def run_device(self, d_seq, n_bytes: int, d_offsets, n_records: int, pre: int, d_qual=None, quality_cutoff: int = 0,
                   single: bool = True):
        """Screen a device batch (the layout of KmerTable.count_device) whose n_records + 1 record offsets are on the device: returns
        (rows (n_records, 5) int64 with columns COLUMNS, hits (n_records, n_colors) int64, single likewise or None) as device
        tensors holding the uint64 words.  Returns when they are written."""
        import torch
        dev = self._device
        rows = torch.empty((n_records, len(COLUMNS)), dtype=torch.int64, device=dev)
        hits = torch.empty((n_records, self.n_colors), dtype=torch.int64, device=dev)
        alone = torch.empty((n_records, self.n_colors), dtype=torch.int64, device=dev) if single else None
        torch.cuda.synchronize(rows.device)
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        self._check("run_device", self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.c_void_p(_ptr(d_offsets)), n_records, C.byref(p),
                    C.c_void_p(rows.data_ptr()), C.c_void_p(hits.data_ptr()), None if alone is None else C.c_void_p(alone.data_ptr()))
        return rows, hits, alone

    def run_records(self, records, pre: int):
        """Pack the records with the batch packer, upload them and their offsets, and return (rows, hits, single) as numpy uint64
        arrays."""
        up = upload_records_with_offsets(self.ctx, records, pre)
        if up is None:
            z = lambda w: np.zeros((0, w), dtype=np.uint64)   # noqa: E731
            return z(len(COLUMNS)), z(self.n_colors), z(self.n_colors)
        return tuple(t.cpu().numpy().view(np.uint64) for t in self.run_device(up[0], up[1], up[2], up[3], pre))


def classify(rows, hits, min_hits: int = 1, min_fraction=0.0) -> np.ndarray:
    """The colour of every record, or -1: `best`, provided hits[best] >= min_hits and hits[best] >= min_fraction * n_kmers.
    min_fraction is a rational (num, den), an int or a float (taken as its exact ratio); the comparison is made in integers by
    cross-multiplying."""
    from fractions import Fraction
    f = Fraction(*min_fraction) if isinstance(min_fraction, tuple) else Fraction(min_fraction)
    num, den = f.numerator, f.denominator
    rows = np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows).view(np.uint64).reshape(-1, len(COLUMNS))
    hits = np.asarray(hits.cpu() if hasattr(hits, "cpu") else hits).view(np.uint64).reshape(rows.shape[0], -1)
    out = np.full(rows.shape[0], -1, dtype=np.int64)
    for r in range(rows.shape[0]):
        best = int(rows[r, 3])
        if best == NONE:
            continue
        h = int(hits[r, best])
        if h >= min_hits and h * den >= num * int(rows[r, 0]):
            out[r] = best
    return out
