"""Exact k-mer counting on the device: ctypes binding of libneedletail_amd_count.so (include/needletail_amd_count.h).

KmerTable counts canonical (or forward) k-mers, k <= 32, in a hash table in device memory and answers with the sorted
(k-mer, count) pairs, the abundance spectrum and point lookups.  There is no fallback: without a gfx950 device every call raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .engine import Batch, Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_count.so")

# every symbol include/needletail_amd_count.h declares
SYMBOLS = [
    "ntk_kmer_table_create", "ntk_kmer_table_destroy", "ntk_kmer_table_reset", "ntk_kmer_table_count_device", "ntk_kmer_table_stats",
    "ntk_kmer_table_extract_device", "ntk_kmer_table_spectrum", "ntk_kmer_table_lookup_device",
]

NTK_ERR_CAPACITY = 5


class TableStats(C.Structure):
    _fields_ = [("n_distinct", C.c_uint64), ("n_total", C.c_uint64), ("n_dropped", C.c_uint64), ("slots", C.c_uint64),
                ("k", C.c_uint32), ("path", C.c_uint32)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    L.lib()   # the core library first: the count library links against it
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP extensions first (python -c 'import __graft_entry__ as g; g.build()')")
    X = C.CDLL(LIB_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    X.ntk_kmer_table_create.argtypes = [vp, u32, u32, u64, C.POINTER(vp)]
    X.ntk_kmer_table_destroy.restype = None
    X.ntk_kmer_table_destroy.argtypes = [vp]
    X.ntk_kmer_table_reset.argtypes = [vp]
    X.ntk_kmer_table_count_device.argtypes = [vp, vp, vp, u64, C.POINTER(L.Params)]
    X.ntk_kmer_table_stats.argtypes = [vp, C.POINTER(TableStats)]
    X.ntk_kmer_table_extract_device.argtypes = [vp, u64, vp, vp, u64, C.POINTER(u64)]
    X.ntk_kmer_table_spectrum.argtypes = [vp, vp, u32]
    X.ntk_kmer_table_lookup_device.argtypes = [vp, vp, u64, vp]
    _lib = X
    return X


def _device_u64(n: int, device: int):
    import torch
    return torch.empty(max(n, 1), dtype=torch.int64, device=f"cuda:{device}")


class KmerTable:
    """An exact count table of k-mers (k = 1..32) on `path` (a PATH_* constant), sized for `capacity` distinct k-mers.

    The key is the value the path emits: canonical on PATH_BYTES_CANONICAL / PATH_BITS_CANONICAL, forward on PATH_BITS."""

    def __init__(self, k: int, path: int, capacity: int, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path = k, path
        self._h = C.c_void_p()
        L.check(lib().ntk_kmer_table_create(self.ctx._h, k, path, capacity, C.byref(self._h)), "ntk_kmer_table_create")

    def close(self):
        if self._h:
            lib().ntk_kmer_table_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        L.check(lib().ntk_kmer_table_reset(self._h), "ntk_kmer_table_reset")

    # -- counting ----------------------------------------------------------------------------------------------------------
    def count_device(self, d_seq, n_bytes: int, pre: int, d_qual=None, quality_cutoff: int = 0):
        """Count a device batch (the layout of Context.reduce_device; async on the context's stream)."""
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        L.check(lib().ntk_kmer_table_count_device(self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.byref(p)),
                "ntk_kmer_table_count_device")

    def count_records(self, records, pre: int):
        """Pack the records with the batch packer (ntk_batch_append: the pre-step's deleted bytes out, one break byte after each),
        upload and count them.  Returns when the table has counted them."""
        import torch
        records = list(records)
        if not records:
            return
        b = Batch(self.ctx, sum(len(r) for r in records) + len(records), len(records))
        try:
            for r in records:
                if not b.append(bytes(r), pre):
                    raise RuntimeError("batch sized for the records is full")
            seq, _ = b.buffers()
            n = int(seq.size)
            dev = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            dev[:n] = torch.from_numpy(np.array(seq, copy=True)).to(dev.device)
            torch.cuda.synchronize(dev.device)
            self.count_device(dev, n, pre)
            self.ctx.synchronize()
        finally:
            b.release()

    # -- reading -----------------------------------------------------------------------------------------------------------
    def stats(self) -> dict:
        s = TableStats()
        L.check(lib().ntk_kmer_table_stats(self._h, C.byref(s)), "ntk_kmer_table_stats")
        return {name: int(getattr(s, name)) for name, _ in TableStats._fields_}

    def items(self, min_count: int = 1):
        """(keys, counts): numpy uint64 arrays, keys ascending, every key with count >= min_count."""
        n = C.c_uint64(0)
        rc = lib().ntk_kmer_table_extract_device(self._h, min_count, None, None, 0, C.byref(n))
        if rc not in (L.NTK_OK, NTK_ERR_CAPACITY) or (rc == NTK_ERR_CAPACITY and n.value == 0):
            L.check(rc, "ntk_kmer_table_extract_device")
        need = int(n.value)
        if need == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        keys, counts = _device_u64(need, self.ctx.device), _device_u64(need, self.ctx.device)
        L.check(lib().ntk_kmer_table_extract_device(self._h, min_count, C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                   need, C.byref(n)), "ntk_kmer_table_extract_device")
        return keys[:need].cpu().numpy().view(np.uint64), counts[:need].cpu().numpy().view(np.uint64)

    def spectrum(self, n_bins: int = 256) -> np.ndarray:
        """hist[c] = distinct k-mers seen c times (the last bin: n_bins - 1 times or more)."""
        h = np.zeros(n_bins, dtype=np.uint64)
        L.check(lib().ntk_kmer_table_spectrum(self._h, h.ctypes.data, n_bins), "ntk_kmer_table_spectrum")
        return h

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

    def lookup(self, kmers):
        """Counts of k-mers given as bytes / str or packed values (canonicalised here for a canonical table).  One k-mer given as
        bytes / str or an int: an int; otherwise a numpy uint64 array."""
        import torch
        single = isinstance(kmers, (bytes, bytearray, str, int, np.integer))
        v = self._values([kmers] if isinstance(kmers, (int, np.integer)) else kmers)
        if self.path != L.PATH_BITS and v.size:
            from .sequence import bit_canonical
            v, _ = bit_canonical(v, self.k, self.ctx)
        dq = torch.from_numpy(v.view(np.int64).copy()).to(f"cuda:{self.ctx.device}")
        dc = _device_u64(v.size, self.ctx.device)
        torch.cuda.synchronize(dq.device)
        L.check(lib().ntk_kmer_table_lookup_device(self._h, C.c_void_p(dq.data_ptr()), v.size, C.c_void_p(dc.data_ptr())),
                "ntk_kmer_table_lookup_device")
        out = dc[: v.size].cpu().numpy().view(np.uint64)
        return int(out[0]) if single else out
