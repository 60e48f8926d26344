"""Per-read k-mer abundance against a count table: ctypes binding of libneedletail_amd_abundance.so
(include/needletail_amd_abundance.h).

ReadAbundance goes back over the reads after counting: for every record of a device batch, the number of k-mers it emits, how many of
them the table holds at least `min_count` times, and the minimum, median (upper), maximum and sum of their table counts - the
quantities behind coverage filters, abundance normalisation and contamination screens.  The rows stay on the device.  There is no
fallback: without a gfx950 device every call raises.  k = 33..63 (WideKmerTable) is not served."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from . import counting
from .counting import KmerTable, upload_records_with_offsets
from .engine import _ptr
from .wide_counting import WideKmerTable

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_abundance.so")
PREFIX = "ntk_read_abundance_"

# the words of a row (struct ntk_read_abundance_row), in order
COLUMNS = ("n_kmers", "n_present", "min", "median", "max", "sum")

_vp, _u64 = C.c_void_p, C.c_uint64
# the calls of the abundance library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _vp, C.POINTER(_vp)], "destroy": [_vp],
    "run_device": [_vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(L.Params), _u64, _vp], "trim": [_vp],
}

# every symbol include/needletail_amd_abundance.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The abundance library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS, needs=(counting.lib,))


class ReadAbundance(L.Handle):
    """Per-record abundance rows against `table`, a KmerTable (k <= 32), which it borrows: keep the table open while this is."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, table: KmerTable):
        if isinstance(table, WideKmerTable):
            raise TypeError("ReadAbundance serves k <= 32 (a KmerTable); the wide table (k = 33..63) is not supported")
        if not isinstance(table, KmerTable):
            raise TypeError(f"ReadAbundance takes a KmerTable, not {type(table).__name__}")
        self.table, self.ctx = table, table.ctx
        self.k, self.path = table.k, table.path
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, table._h, C.byref(self._h))

    def trim(self):
        """Free the scratch kept between calls."""
        self._check("trim", self._h)

    def run_device(self, d_seq, n_bytes: int, d_offsets, n_records: int, pre: int, d_qual=None, quality_cutoff: int = 0,
                   min_count: int = 1):
        """The rows of a device batch (the layout of KmerTable.count_device) whose n_records + 1 record offsets are on the device
        (int64 / uint64, as Batch.buffers() returns them): a device torch.int64 tensor of shape (n_records, 6), columns COLUMNS (view
        it as uint64 on the host for counts of 2^63 and above).  Returns when the rows are written."""
        import torch
        rows = torch.empty((n_records, len(COLUMNS)), dtype=torch.int64, device=f"cuda:{self.ctx.device}")
        torch.cuda.synchronize(rows.device)
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        self._check("run_device", self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.c_void_p(_ptr(d_offsets)), n_records, C.byref(p),
                    min_count, C.c_void_p(rows.data_ptr()))
        return rows

    def run_records(self, records, pre: int, min_count: int = 1) -> np.ndarray:
        """Pack the records with the batch packer (the route of KmerTable.count_records), upload them and their offsets, and return
        the rows as a numpy uint64 array of shape (n_records, 6)."""
        up = upload_records_with_offsets(self.ctx, records, pre)
        if up is None:
            return np.zeros((0, len(COLUMNS)), dtype=np.uint64)
        rows = self.run_device(up[0], up[1], up[2], up[3], pre, min_count=min_count)
        return rows.cpu().numpy().view(np.uint64)
