"""Exact k-mer counting on the device: ctypes binding of libneedletail_amd_count.so (include/needletail_amd_count.h).

KmerTable counts canonical (or forward) k-mers, k <= 32, in a hash table in device memory and answers with the sorted
(k-mer, count) pairs, the abundance spectrum and point lookups.  There is no fallback: without a gfx950 device every call raises.
CountTable and CALLS are what it shares with wide_counting.WideKmerTable (k = 33..63), whose library has the same eight calls under
its own symbol prefix."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .engine import Batch, Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_count.so")
PREFIX = "ntk_kmer_table_"

NTK_ERR_CAPACITY = 5


class TableStats(C.Structure):
    _fields_ = [("n_distinct", C.c_uint64), ("n_total", C.c_uint64), ("n_dropped", C.c_uint64), ("slots", C.c_uint64),
                ("k", C.c_uint32), ("path", C.c_uint32)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the eight calls of a count table library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, _u32, _u64, C.POINTER(_vp)], "destroy": [_vp], "reset": [_vp],
    "count_device": [_vp, _vp, _vp, _u64, C.POINTER(L.Params)], "stats": [_vp, C.POINTER(TableStats)],
    "extract_device": [_vp, _u64, _vp, _vp, _u64, C.POINTER(_u64)], "spectrum": [_vp, _vp, _u32], "lookup_device": [_vp, _vp, _u64, _vp],
}

# every symbol include/needletail_amd_count.h declares
SYMBOLS = [PREFIX + c for c in CALLS]

def lib() -> C.CDLL:
    """The count library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _device_u64(n: int, device: int):
    import torch
    return torch.empty(max(n, 1), dtype=torch.int64, device=f"cuda:{device}")


def _upload(ctx: Context, records, pre: int, with_offsets: bool):
    """Pack the records with the batch packer (ntk_batch_append: the pre-step's deleted bytes out, one break byte after each) and upload
    them: (device tensor in the batch layout, n_bytes, the packer's record offsets as a device int64 tensor if asked for, n_records),
    or None for no records."""
    import torch
    records = list(records)
    if not records:
        return None
    b = Batch(ctx, sum(len(r) for r in records) + len(records), len(records))
    try:
        for r in records:
            if not b.append(bytes(r), pre):
                raise RuntimeError("batch sized for the records is full")
        seq, off = b.buffers()
        n = int(seq.size)
        dev = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        dev[:n] = torch.from_numpy(np.array(seq, copy=True)).to(dev.device)
        d_off = torch.from_numpy(np.array(off, copy=True).view(np.int64)).to(dev.device) if with_offsets else None
        torch.cuda.synchronize(dev.device)
    finally:
        b.release()
    return dev, n, d_off, len(records)


def upload_records(ctx: Context, records, pre: int):
    """The records packed and uploaded (_upload): (device batch, n_bytes), or None for no records."""
    up = _upload(ctx, records, pre, False)
    return up and up[:2]


def upload_records_with_offsets(ctx: Context, records, pre: int):
    """upload_records with the packer's record offsets: (device batch, n_bytes, device int64 offsets, n_records), or None."""
    return _upload(ctx, records, pre, True)


class CountTable(L.Handle):
    """What the count tables share: a table in device memory behind one library's eight calls.  A subclass names the library
    (_lib, _prefix), the u64 words of a key (_key_words) and turns lookup's argument into queries (_queries)."""

    _key_words: int

    def __init__(self, k: int, path: int, capacity: int, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path = k, path
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, k, path, capacity, C.byref(self._h))

    def reset(self):
        self._check("reset", self._h)

    # -- counting ----------------------------------------------------------------------------------------------------------
    def count_device(self, d_seq, n_bytes: int, pre: int, d_qual=None, quality_cutoff: int = 0):
        """Count a device batch (the layout of Context.reduce_device; async on the context's stream)."""
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        self._check("count_device", self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.byref(p))

    def count_records(self, records, pre: int):
        """Pack the records with the batch packer (upload_records), upload and count them.  Returns when the table has counted them."""
        up = upload_records(self.ctx, records, pre)
        if up is not None:
            self.count_device(up[0], up[1], pre)
            self.ctx.synchronize()

    # -- reading -----------------------------------------------------------------------------------------------------------
    def stats(self) -> dict:
        s = TableStats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in TableStats._fields_}

    def _keys(self, words: np.ndarray) -> np.ndarray:
        return words if self._key_words == 1 else words.reshape(-1, self._key_words)

    def items(self, min_count: int = 1):
        """(keys, counts): numpy uint64 arrays, keys ascending, every key with count >= min_count (the subclass says what a key is)."""
        n = C.c_uint64(0)
        rc = self._fn("extract_device")(self._h, min_count, None, None, 0, C.byref(n))
        if rc not in (L.NTK_OK, NTK_ERR_CAPACITY) or (rc == NTK_ERR_CAPACITY and n.value == 0):
            L.check(rc, self._prefix + "extract_device")
        need, w = int(n.value), self._key_words
        if need == 0:
            return self._keys(np.zeros(0, np.uint64)), np.zeros(0, np.uint64)
        keys, counts = _device_u64(w * need, self.ctx.device), _device_u64(need, self.ctx.device)
        self._check("extract_device", self._h, min_count, C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()), need, C.byref(n))
        return self._keys(keys[: w * need].cpu().numpy().view(np.uint64)), counts[:need].cpu().numpy().view(np.uint64)

    def spectrum(self, n_bins: int = 256) -> np.ndarray:
        """hist[c] = distinct k-mers seen c times (the last bin: n_bins - 1 times or more)."""
        h = np.zeros(n_bins, dtype=np.uint64)
        self._check("spectrum", self._h, h.ctypes.data, n_bins)
        return h

    def _queries(self, kmers):
        """(single, queries): whether one k-mer was given, and the uint64 keys to look up (one value or row each)."""
        raise NotImplementedError

    def lookup(self, kmers):
        """Counts of the k-mers (the subclass says in which forms): an int for one k-mer, otherwise a numpy uint64 array."""
        import torch
        single, v = self._queries(kmers)
        n = v.shape[0]
        dq = torch.from_numpy(v.reshape(-1).view(np.int64).copy()).to(f"cuda:{self.ctx.device}")
        dc = _device_u64(n, self.ctx.device)
        torch.cuda.synchronize(dq.device)
        self._check("lookup_device", self._h, C.c_void_p(dq.data_ptr()), n, C.c_void_p(dc.data_ptr()))
        out = dc[:n].cpu().numpy().view(np.uint64)
        return int(out[0]) if single else out


class KmerTable(CountTable):
    """An exact count table of k-mers (k = 1..32) on `path` (a PATH_* constant), sized for `capacity` distinct k-mers.

    The key is the value the path emits: canonical on PATH_BYTES_CANONICAL / PATH_BITS_CANONICAL, forward on PATH_BITS.  items()
    returns keys as a uint64 array of values.  lookup() takes k-mers as bytes / str or packed values (canonicalised here for a
    canonical table); one k-mer given as bytes / str or an int reads an int."""

    _lib, _prefix, _key_words = staticmethod(lib), PREFIX, 1

    def _values(self, kmers) -> np.ndarray:
        if isinstance(kmers, (bytes, bytearray, str)):
            kmers = [kmers]
        if isinstance(kmers, np.ndarray) and kmers.dtype != object:
            return np.ascontiguousarray(kmers, dtype=np.uint64)
        out = np.empty(len(kmers), dtype=np.uint64)
        code = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
        for i, x in enumerate(kmers):
            if isinstance(x, str):
                x = x.encode()
            if isinstance(x, (bytes, bytearray)):
                if len(x) != self.k:
                    raise ValueError(f"k-mer of length {len(x)} in a k = {self.k} table")
                v = 0
                for ch in x:
                    if ch not in code:
                        raise ValueError(f"not a base: {chr(ch)!r}")
                    v = (v << 2) | code[ch]
                out[i] = v
            else:
                out[i] = int(x)
        return out

    def _queries(self, kmers):
        single = isinstance(kmers, (bytes, bytearray, str, int, np.integer))
        v = self._values([kmers] if isinstance(kmers, (int, np.integer)) else kmers)
        if self.path != L.PATH_BITS and v.size:
            from .sequence import bit_canonical
            v, _ = bit_canonical(v, self.k, self.ctx)
        return single, v
