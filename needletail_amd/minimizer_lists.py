"""The windowed minimizers of a batch as lists.  ctypes binding of libneedletail_amd_minimizer_list.so
(include/needletail_amd/minimizer_list.h).

MinimizerList lists the (w, k) minimizers of every record of a device batch: per record the positions, values and strands of its
minimizers, each with the number of consecutive windows it won (its span).  The minimizer of a window of w k-mers is the leftmost one
whose key is smallest - the value itself (LEX) or the MinHash libraries' hash of it (HASH).  The result is a CSR that stays on the device
(device_arrays) and can be read back (read).  k = 1..32, w = 1..256.  There is no fallback: without a gfx950 device every call of the
class raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from . import counting
from .engine import Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_minimizer_list.so")
PREFIX = "ntk_minimizer_list_"

LEX, HASH = 0, 1              # NTK_MINIMIZER_LIST_LEX, NTK_MINIMIZER_LIST_HASH
W_MAX = 256                   # NTK_MINIMIZER_LIST_W_MAX
XOR = 0x9E3779B97F4A7C15      # NTK_MINIMIZER_LIST_XOR


class Stats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_entries", C.c_uint64), ("n_windows", C.c_uint64), ("n_chunks", C.c_uint64),
                ("device_bytes", C.c_uint64), ("k", C.c_uint32), ("path", C.c_uint32), ("w", C.c_uint32), ("order", C.c_uint32)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
_pp = C.POINTER(C.c_void_p)
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, _u32, _u32, _u32, _pp], "destroy": [_vp],
    "run_device": [_vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(L.Params)],
    "read": [_vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)],
    "result_device": [_vp, _pp, _pp, _pp, _pp, C.POINTER(_u64)],
    "stats": [_vp, C.POINTER(Stats)], "trim": [_vp],
}

# every symbol include/needletail_amd/minimizer_list.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


class MinimizerList(L.Handle):
    """The (w, k) minimizers of the k-mers of `path` (a PATH_* constant) under `order` (LEX or HASH), k = 1..32, w = 1..256."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, k: int, path: int, w: int, order: int = LEX, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path, self.w, self.order = k, path, w, order
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, k, path, w, order, C.byref(self._h))

    def trim(self):
        """Free every device array, the held result included."""
        self._check("trim", self._h)

    def run_device(self, d_seq, n_bytes: int, d_offsets, n_records: int, pre: int, d_qual=None, quality_cutoff: int = 0):
        """List the minimizers of every record of a device batch (the layout of KmerTable.count_device) whose n_records + 1 record
        offsets are on the device (int64 / uint64, as Batch.buffers() returns them).  Returns when the result is held; it replaces the
        one before."""
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        o = None if d_offsets is None else C.c_void_p(_ptr(d_offsets))
        d = None if d_seq is None else C.c_void_p(_ptr(d_seq))
        self._check("run_device", self._h, d, q, n_bytes, o, n_records, C.byref(p))

    def run_records(self, records, pre: int, quals=None, cutoff: int = 0):
        """Pack the records with the batch packer (the route of KmerTable.count_records), upload them with the packer's offsets and list
        their minimizers.  quals: one quality string per record (the pre-step must not delete a byte of such a record); a base whose
        quality byte is below `cutoff` is masked."""
        import torch
        records = [bytes(r) for r in records]
        up = counting._upload(self.ctx, records, pre, True)
        if up is None:
            p = L.Params(self.k, self.path, pre, 0)
            self._check("run_device", self._h, None, None, 0, None, 0, C.byref(p))
            return
        dev, n, d_off, n_records = up
        d_qual = None
        if quals is not None:
            off = d_off.cpu().numpy()
            qual = np.full(int(dev.numel()), 0xFF, dtype=np.uint8)
            for i, q in enumerate(quals):
                if len(q) != int(off[i + 1] - off[i]) - 1:
                    raise ValueError(f"record {i}: {len(q)} quality bytes for {int(off[i + 1] - off[i]) - 1} packed bases")
                qual[int(off[i]): int(off[i]) + len(q)] = np.frombuffer(bytes(q), dtype=np.uint8)
            d_qual = torch.from_numpy(qual).to(dev.device)
        self.run_device(dev, n, d_off, n_records, pre, d_qual, cutoff if quals is not None else 0)

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def read(self):
        """(offsets, pos, values, strand, span) as numpy arrays: record r's entries are [offsets[r], offsets[r + 1]); pos is the start
        of the k-mer in its record, values the k-mer as materialised, strand its flag (uint8) and span the number of consecutive
        windows it won (uint32)."""
        st = self.stats()
        n = C.c_uint64(0)
        rc = self._fn("read")(self._h, None, None, None, None, 0, C.byref(n))
        if rc not in (0, 5):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        offsets = np.zeros(st["n_records"] + 1, dtype=np.uint64)
        pos, values, info = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint32)
        data = lambda a: a.ctypes.data if a.size else None   # noqa: E731
        self._check("read", self._h, offsets.ctypes.data, data(pos), data(values), data(info), n.value, C.byref(n))
        return offsets, pos, values, (info & 1).astype(np.uint8), info >> 1

    def device_arrays(self):
        """(d_offsets, d_pos, d_values, d_info, n): the held result where it lies on the device, as addresses (0 where nothing is
        held) and the number of entries.  Host-side only; the addresses stay valid until the next run_device, trim or close."""
        ptrs = [C.c_void_p() for _ in range(4)]
        n = C.c_uint64(0)
        self._check("result_device", self._h, *(C.byref(p) for p in ptrs), C.byref(n))
        return tuple(p.value or 0 for p in ptrs) + (n.value,)
