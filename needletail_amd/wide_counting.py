"""Exact counting of canonical k-mers with k = 33..63 on the device: ctypes binding of libneedletail_amd_wide_count.so
(include/needletail_amd_wide_count.h).

WideKmerTable counts the canonical k-mers of the byte path (normalize -> canonical_kmers(k, &rc)) in a hash table in device memory and
answers with the sorted (k-mer, count) pairs, the abundance spectrum and point lookups.  A key is two u64 words [hi, lo]: hi = the first
k - 32 bases, lo = the last 32, in the 2-bit code (A 0, C 1, G 2, T 3, first base most significant).  There is no fallback: without a
gfx950 device every call raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .counting import NTK_ERR_CAPACITY, TableStats, _device_u64
from .engine import Batch, Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_wide_count.so")

# every symbol include/needletail_amd_wide_count.h declares
SYMBOLS = [
    "ntk_wide_table_create", "ntk_wide_table_destroy", "ntk_wide_table_reset", "ntk_wide_table_count_device", "ntk_wide_table_stats",
    "ntk_wide_table_extract_device", "ntk_wide_table_spectrum", "ntk_wide_table_lookup_device",
]

K_MIN, K_MAX = 33, 63

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    L.lib()   # the core library first: the wide count library links against it
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP extensions first (python -c 'import __graft_entry__ as g; g.build()')")
    X = C.CDLL(LIB_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    X.ntk_wide_table_create.argtypes = [vp, u32, u32, u64, C.POINTER(vp)]
    X.ntk_wide_table_destroy.restype = None
    X.ntk_wide_table_destroy.argtypes = [vp]
    X.ntk_wide_table_reset.argtypes = [vp]
    X.ntk_wide_table_count_device.argtypes = [vp, vp, vp, u64, C.POINTER(L.Params)]
    X.ntk_wide_table_stats.argtypes = [vp, C.POINTER(TableStats)]
    X.ntk_wide_table_extract_device.argtypes = [vp, u64, vp, vp, u64, C.POINTER(u64)]
    X.ntk_wide_table_spectrum.argtypes = [vp, vp, u32]
    X.ntk_wide_table_lookup_device.argtypes = [vp, vp, u64, vp]
    _lib = X
    return X


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


class WideKmerTable:
    """An exact count table of canonical k-mers, k = 33..63, on PATH_BYTES_CANONICAL, sized for `capacity` distinct k-mers.

    The methods are KmerTable's; keys are (n, 2) uint64 arrays of [hi, lo] rows."""

    def __init__(self, k: int, path: int, capacity: int, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path = k, path
        self._h = C.c_void_p()
        L.check(lib().ntk_wide_table_create(self.ctx._h, k, path, capacity, C.byref(self._h)), "ntk_wide_table_create")

    def close(self):
        if self._h:
            lib().ntk_wide_table_destroy(self._h)
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
        L.check(lib().ntk_wide_table_reset(self._h), "ntk_wide_table_reset")

    # -- counting ----------------------------------------------------------------------------------------------------------
    def count_device(self, d_seq, n_bytes: int, pre: int, d_qual=None, quality_cutoff: int = 0):
        """Count a device batch (the layout of Context.reduce_device; async on the context's stream)."""
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        L.check(lib().ntk_wide_table_count_device(self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.byref(p)),
                "ntk_wide_table_count_device")

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
        L.check(lib().ntk_wide_table_stats(self._h, C.byref(s)), "ntk_wide_table_stats")
        return {name: int(getattr(s, name)) for name, _ in TableStats._fields_}

    def items(self, min_count: int = 1):
        """(keys, counts): an (n, 2) uint64 array of [hi, lo] rows, ascending as 2k-bit values, and a uint64 array of counts; every
        key with count >= min_count."""
        n = C.c_uint64(0)
        rc = lib().ntk_wide_table_extract_device(self._h, min_count, None, None, 0, C.byref(n))
        if rc not in (L.NTK_OK, NTK_ERR_CAPACITY) or (rc == NTK_ERR_CAPACITY and n.value == 0):
            L.check(rc, "ntk_wide_table_extract_device")
        need = int(n.value)
        if need == 0:
            return np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64)
        keys, counts = _device_u64(2 * need, self.ctx.device), _device_u64(need, self.ctx.device)
        L.check(lib().ntk_wide_table_extract_device(self._h, min_count, C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                   need, C.byref(n)), "ntk_wide_table_extract_device")
        return keys[: 2 * need].cpu().numpy().view(np.uint64).reshape(need, 2), counts[:need].cpu().numpy().view(np.uint64)

    def spectrum(self, n_bins: int = 256) -> np.ndarray:
        """hist[c] = distinct k-mers seen c times (the last bin: n_bins - 1 times or more)."""
        h = np.zeros(n_bins, dtype=np.uint64)
        L.check(lib().ntk_wide_table_spectrum(self._h, h.ctypes.data, n_bins), "ntk_wide_table_spectrum")
        return h

    def lookup(self, kmers):
        """Counts of k-mers given as str / bytes (either strand) or as an (n, 2) array of [hi, lo] rows (canonicalised by the library).
        One k-mer given as str / bytes: an int; otherwise a numpy uint64 array."""
        import torch
        single = isinstance(kmers, (bytes, bytearray, str))
        if single:
            v = encode([kmers], self.k)
        elif isinstance(kmers, np.ndarray) and kmers.dtype != object:
            v = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, 2)
        else:
            v = encode(list(kmers), self.k)
        n = v.shape[0]
        dq = torch.from_numpy(v.reshape(-1).view(np.int64).copy()).to(f"cuda:{self.ctx.device}")
        dc = _device_u64(n, self.ctx.device)
        torch.cuda.synchronize(dq.device)
        L.check(lib().ntk_wide_table_lookup_device(self._h, C.c_void_p(dq.data_ptr()), n, C.c_void_p(dc.data_ptr())),
                "ntk_wide_table_lookup_device")
        out = dc[:n].cpu().numpy().view(np.uint64)
        return int(out[0]) if single else out
