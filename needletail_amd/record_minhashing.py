"""One sketch per record, all in one call.  ctypes binding of libneedletail_amd_record_minhash.so
(include/needletail_amd_record_minhash.h).

RecordMinHash makes a MinHash sketch of every record of a device batch - a multi-FASTA of genomes, a set of contigs, long reads - in one
pass: record r's sketch is exactly what a KmerMinHash of the same k, path and kind holds after that record alone (the same hash, the
exact count behind every kept hash).  The result is a CSR on the host, and MinHashSet.add_record_sketches takes it whole.  k = 1..32.
There is no fallback: without a gfx950 device every call of the class raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from . import counting
from .engine import Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_record_minhash.so")
PREFIX = "ntk_record_minhash_"

XOR = 0x9E3779B97F4A7C15      # NTK_RECORD_MINHASH_XOR
MAX_NUM = 1 << 20             # NTK_RECORD_MINHASH_MAX_NUM
ALLPASS = 4                   # NTK_RECORD_MINHASH_ALLPASS
BUFFER_DEFAULT = 1 << 24      # NTK_RECORD_MINHASH_BUFFER_DEFAULT
BUFFER_MIN, BUFFER_MAX = 256, 1 << 30
ALL = (1 << 64) - 1


class Stats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_entries", C.c_uint64), ("n_windows", C.c_uint64), ("num", C.c_uint64),
                ("scaled", C.c_uint64), ("buffer_entries", C.c_uint64), ("n_rounds", C.c_uint64), ("n_retried_records", C.c_uint64),
                ("n_redone", C.c_uint64), ("device_bytes", C.c_uint64), ("k", C.c_uint32), ("path", C.c_uint32)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, _u32, _u64, _u64, _u64, C.POINTER(_vp)], "destroy": [_vp],
    "run_device": [_vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(L.Params)],
    "read": [_vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)], "stats": [_vp, C.POINTER(Stats)], "trim": [_vp],
}

# every symbol include/needletail_amd_record_minhash.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


class RecordMinHash(L.Handle):
    """Per-record MinHash sketches of the k-mers of `path` (a PATH_* constant), k = 1..32.  Exactly one of `num` (bottom-s) and
    `scaled` (every hash <= (2^64 - 1) // scaled) is non-zero; buffer_entries is a memory knob (12 B per candidate pair; 0: the
    default)."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, k: int, path: int, num: int = 0, scaled: int = 0, ctx: Context = None, buffer_entries: int = 0):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path, self.num, self.scaled = k, path, num, scaled
        self.max_hash = ALL // scaled if scaled else ALL
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, k, path, num, scaled, buffer_entries, C.byref(self._h))

    def trim(self):
        """Free every device array, the held result included."""
        self._check("trim", self._h)

    def run_device(self, d_seq, n_bytes: int, d_offsets, n_records: int, pre: int, d_qual=None, quality_cutoff: int = 0):
        """Sketch every record of a device batch (the layout of KmerTable.count_device) whose n_records + 1 record offsets are on the
        device (int64 / uint64, as Batch.buffers() returns them).  Returns when the result is held; it replaces the one before."""
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        o = None if d_offsets is None else C.c_void_p(_ptr(d_offsets))
        d = None if d_seq is None else C.c_void_p(_ptr(d_seq))
        self._check("run_device", self._h, d, q, n_bytes, o, n_records, C.byref(p))

    def run_records(self, records, pre: int):
        """Pack the records with the batch packer (the route of KmerTable.count_records), upload them with the packer's offsets and
        sketch them."""
        up = counting._upload(self.ctx, records, pre, True)
        if up is None:
            p = L.Params(self.k, self.path, pre, 0)
            self._check("run_device", self._h, None, None, 0, None, 0, C.byref(p))
        else:
            self.run_device(up[0], up[1], up[2], up[3], pre)

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def sketches(self):
        """(offsets, n_windows, hashes, counts) as numpy uint64: record r's kept hashes, strictly ascending, are
        hashes[offsets[r]:offsets[r + 1]], the number of k-mers behind each is counts[...], and n_windows[r] k-mers is what the record
        emits."""
        st = self.stats()
        n = C.c_uint64(0)
        rc = lib().ntk_record_minhash_read(self._h, None, None, None, None, 0, C.byref(n))
        if rc not in (0, 5):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        offsets, windows = np.zeros(st["n_records"] + 1, dtype=np.uint64), np.zeros(st["n_records"], dtype=np.uint64)
        h, c = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        data = lambda a: a.ctypes.data if a.size else None
        self._check("read", self._h, offsets.ctypes.data, data(windows), data(h), data(c), n.value, C.byref(n))
        return offsets, windows, h, c
