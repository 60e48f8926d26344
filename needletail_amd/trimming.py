"""Trimming reads by k-mer abundance and writing the kept reads out as a batch: ctypes binding of libneedletail_amd_trim.so
(include/needletail_amd_trim.h).

ReadTrimmer is the step after counting and per-read abundance: for every record of a device batch the interval to keep - the read up
to its first low-abundance k-mer (khmer's rule), or its longest run of solid k-mers - and then the kept reads as a new device batch,
which count_device, ReadAbundance.run_device and the trimmer itself take as it is.  Nothing leaves the device.  There is no fallback:
without a gfx950 device every call raises.  k = 33..63 (WideKmerTable) is not served."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from . import counting
from .counting import KmerTable, upload_records_with_offsets
from .engine import _ptr
from .wide_counting import WideKmerTable

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_trim.so")
PREFIX = "ntk_read_trim_"

TRIM_PREFIX, TRIM_LONGEST = 0, 1   # NTK_TRIM_PREFIX, NTK_TRIM_LONGEST
MODES = {"prefix": TRIM_PREFIX, "longest": TRIM_LONGEST}

# the words of a row (struct ntk_read_trim_row), in order
COLUMNS = ("start", "length", "n_kmers", "n_solid")

_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the trim library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _vp, C.POINTER(_vp)], "destroy": [_vp], "release": [_vp],
    "run_device": [_vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(L.Params), _u64, _u32, _u64, _vp],
    "compact_device": [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)],
}

# every symbol include/needletail_amd_trim.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The trim library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS, needs=(counting.lib,))


def _mode(mode) -> int:
    return MODES[mode] if isinstance(mode, str) else int(mode)


class ReadTrimmer(L.Handle):
    """Per-record kept intervals against `table`, a KmerTable (k <= 32), which it borrows (keep the table open while this is), and
    the kept reads as a device batch."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, table: KmerTable):
        if isinstance(table, WideKmerTable):
            raise TypeError("ReadTrimmer serves k <= 32 (a KmerTable); the wide table (k = 33..63) is not supported")
        if not isinstance(table, KmerTable):
            raise TypeError(f"ReadTrimmer takes a KmerTable, not {type(table).__name__}")
        self.table, self.ctx = table, table.ctx
        self.k, self.path = table.k, table.path
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, table._h, C.byref(self._h))

    def release(self):
        """Free the scratch kept between calls."""
        self._check("release", self._h)

    def run_device(self, d_seq, n_bytes: int, d_offsets, n_records: int, pre: int, d_qual=None, quality_cutoff: int = 0,
                   min_count: int = 1, mode=TRIM_PREFIX, min_length: int = 0):
        """The rows of a device batch (the layout of ReadAbundance.run_device): a device torch.int64 tensor of shape (n_records, 4),
        columns COLUMNS - the kept interval in bytes relative to the record (0, 0: nothing kept), the windows the record emits and
        how many of them the table holds at least `min_count` times.  mode: TRIM_PREFIX / "prefix" or TRIM_LONGEST / "longest".
        Returns when the rows are written."""
        import torch
        rows = torch.empty((n_records, len(COLUMNS)), dtype=torch.int64, device=f"cuda:{self.ctx.device}")
        torch.cuda.synchronize(rows.device)
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        self._check("run_device", self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.c_void_p(_ptr(d_offsets)), n_records, C.byref(p),
                    min_count, _mode(mode), min_length, C.c_void_p(rows.data_ptr()))
        return rows

    def compact_device(self, d_seq, n_bytes: int, d_offsets, n_records: int, rows, d_aux=None):
        """The records with length > 0 as a new device batch, in input order: (out_seq, out_n_bytes, out_offsets, out_source) and,
        with a parallel stream d_aux (the quality bytes), out_aux as a fifth item.  out_seq (and out_aux) are uint8 tensors padded
        with break bytes to a multiple of 16 and 64 more, out_offsets the n_out + 1 int64 offsets, out_source the input index of
        every output record; all on the device.  The output is sized for the worst case (the input's size) and cut to what was
        written."""
        import torch
        device = f"cuda:{self.ctx.device}"
        cap_bytes = (n_bytes + 15) // 16 * 16
        out_seq = torch.full((cap_bytes + 64,), ord("\n"), dtype=torch.uint8, device=device)
        out_aux = None if d_aux is None else torch.full((cap_bytes + 64,), ord("\n"), dtype=torch.uint8, device=device)
        out_offsets = torch.zeros(n_records + 1, dtype=torch.int64, device=device)
        out_source = torch.zeros(max(n_records, 1), dtype=torch.int64, device=device)
        torch.cuda.synchronize(out_seq.device)
        nb, nr = _u64(0), _u64(0)
        vp = lambda x: None if x is None else C.c_void_p(_ptr(x))   # noqa: E731
        self._check("compact_device", self._h, vp(d_seq), vp(d_aux), n_bytes, vp(d_offsets), n_records, vp(rows), vp(out_seq),
                    vp(out_aux), cap_bytes, vp(out_offsets), vp(out_source), n_records, C.byref(nb), C.byref(nr))
        keep = (nb.value + 15) // 16 * 16 + 64
        out = (out_seq[:keep], nb.value, out_offsets[: nr.value + 1], out_source[: nr.value])
        return out if d_aux is None else out + (out_aux[:keep],)

    def trim_records(self, records, pre: int, mode=TRIM_PREFIX, min_count: int = 1, min_length: int = 0, quals=None):
        """Pack the records with the batch packer, upload them, trim and compact on the device, and return the kept reads as a list
        of (source_index, bytes), or (source_index, bytes, qual_bytes) with `quals` (one quality string per record, cut alike; the
        pre-step must not delete a byte of such a record)."""
        import torch
        records = [bytes(r) for r in records]
        up = upload_records_with_offsets(self.ctx, records, pre)
        if up is None:
            return []
        dev, n, d_off, n_records = up
        d_aux = None
        if quals is not None:
            off = d_off.cpu().numpy()
            aux = np.full(int(dev.numel()), ord("\n"), dtype=np.uint8)
            for i, q in enumerate(quals):
                if len(q) != int(off[i + 1] - off[i]) - 1:
                    raise ValueError(f"record {i}: {len(q)} quality bytes for {int(off[i + 1] - off[i]) - 1} packed bases")
                aux[int(off[i]): int(off[i]) + len(q)] = np.frombuffer(bytes(q), dtype=np.uint8)
            d_aux = torch.from_numpy(aux).to(dev.device)
        rows = self.run_device(dev, n, d_off, n_records, pre, min_count=min_count, mode=mode, min_length=min_length)
        out = self.compact_device(dev, n, d_off, n_records, rows, d_aux)
        seq, off, src = out[0].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()
        aux = out[4].cpu().numpy() if quals is not None else None
        kept = []
        for i in range(len(src)):
            lo, hi = int(off[i]), int(off[i + 1]) - 1
            item = (int(src[i]), seq[lo:hi].tobytes())
            kept.append(item if aux is None else item + (aux[lo:hi].tobytes(),))
        return kept
