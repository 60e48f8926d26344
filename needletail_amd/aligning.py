"""Base-level alignment of reported chains.  ctypes binding of libneedletail_amd_align.so (include_pending/needletail_amd/align.h).

ChainAlignments fills the gaps between the anchors of selected chains by banded affine dynamic programming on the device: the chains
an AnchorChains holds, the anchors a SeedIndex holds, the selection a ChainMappings reports - each taken zero-copy - and the two
sequence batches where they lie.  The result is, per selected chain, a canonical CIGAR (=, X, I, D) with its counts and score; it stays
on the device (device_arrays) and can be read back (read).  Integer arithmetic only: exact and deterministic.  There is no fallback:
without a gfx950 device every call of the class raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .engine import Context, _ptr, default_context
from .mapping import _anchor_args, _chain_args

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_align.so")
PREFIX = "ntk_align_"

SEG_MAX = 4095                # ALN_SEG_MAX of csrc/ntk_align_rule.hpp: the largest band_pad and max_seg
SPAN_MAX = 1 << 28            # ALN_SPAN_MAX: a chain spanning this much of its reference or read is refused
ERR_CAPACITY = 5              # NTK_ERR_CAPACITY
ROW = ("flags", "n_cigar", "n_eq", "n_x", "n_ins", "n_del", "n_gaps", "zero")
ALIGNED, TOO_LONG = 1, 2      # the flags of a row
OPS = {1: "I", 2: "D", 7: "=", 8: "X"}   # BAM's codes of the four ops of a CIGAR word, len << 4 | op


class Params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("q", C.c_uint32), ("e", C.c_uint32), ("band_pad", C.c_uint32),
                ("max_seg", C.c_uint32), ("work_mib", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("n_sel", C.c_uint64), ("n_aligned", C.c_uint64), ("n_too_long", C.c_uint64), ("n_segments", C.c_uint64),
                ("n_dp_segments", C.c_uint64), ("dp_cells", C.c_uint64), ("n_cigar", C.c_uint64), ("n_groups", C.c_uint64),
                ("device_bytes", C.c_uint64)]


_vp, _u64 = C.c_void_p, C.c_uint64
_pp, _pu64 = C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _pp], "destroy": [_vp],
    "run_device": [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp, _u64, C.POINTER(Params)],
    "read": [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _pu64, _pu64],
    "result_device": [_vp, _pp, _pp, _pp, _pp, _pu64, _pu64],
    "stats": [_vp, C.POINTER(Stats)], "trim": [_vp],
}

# every symbol include_pending/needletail_amd/align.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def cigar_string(words) -> str:
    """A CIGAR's words (len << 4 | op) as text: 12=1X3D ..."""
    return "".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in words)


def _batch_args(batch):
    """(d_seq, n_bytes, d_offsets, n_records) of a device batch (dev, n_bytes, offsets, n_records): the bytes and the n_records + 1
    record starts (8-byte words) as device tensors."""
    dev, n_bytes, offsets, n_records = batch
    if offsets is None or offsets.element_size() != 8 or offsets.numel() < n_records + 1:
        raise ValueError("the offsets of a batch are n_records + 1 8-byte words on the device")
    return (_ptr(dev) if n_bytes else 0), int(n_bytes), _ptr(offsets), int(n_records)


def _sel_args(sel):
    """(d_sel, n_sel) of a ChainMappings' reported chains, zero-copy, or of a device tensor of 4-byte words."""
    if hasattr(sel, "device_arrays"):
        _, _, _, d_out, _, _, n_out = sel.device_arrays()
        return d_out, n_out
    if sel.element_size() != 4:
        raise ValueError("the selection is a device tensor of 4-byte words")
    return (_ptr(sel) if sel.numel() else 0), int(sel.numel())


class ChainAlignments(L.Handle):
    """The base-level alignments of selected chains: per chain a canonical CIGAR, its counts and its score."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, C.byref(self._h))

    def trim(self):
        """Free the result and every work array."""
        self._check("trim", self._h)

    def run(self, refs, reads, chains, anchors, sel, k: int, a: int = 2, b: int = 4, q: int = 4, e: int = 2, band_pad: int = 64,
            max_seg: int = 2048, work_mib: int = 0):
        """Align the chains `sel` names - a ChainMappings, whose reported chains are used, or a device tensor of chain indices - of the
        chains an AnchorChains holds (or (c_offsets, chain_rows, m_offsets, members) as device tensors) over the anchors a SeedIndex
        holds (or (rpos, qpos)).  refs and reads are the device batches the lists were made from, each (dev, n_bytes, offsets,
        n_records); k is the seed length of the lists; a, b, q, e score a match, a mismatch and a gap of length L (q + L * e); the band
        is the two diagonals of a between part padded by band_pad; a chain with a between part longer than max_seg is flagged TOO_LONG;
        work_mib bounds the direction workspace of one group (0: 256).  Returns when the result is held; it replaces the one before.
        Parameters out of range and arrays that fail the verification raise NtkError with status 2 (NTK_ERR_BAD_ARG) and leave the held
        result as it was."""
        values = (k, a, b, q, e, band_pad, max_seg, work_mib)
        if not all(0 <= v < 1 << 32 for v in values):
            raise ValueError("the parameters are 32-bit words")
        params = Params(*values)
        d_ref, ref_bytes, d_ref_off, n_refs = _batch_args(refs)
        d_seq, seq_bytes, d_seq_off, n_reads = _batch_args(reads)
        c_ptrs, n_chain_reads, n_chains, n_members = _chain_args(chains)
        if n_chain_reads != n_reads:
            raise ValueError("the chains are those of %d reads and the batch holds %d" % (n_chain_reads, n_reads))
        a_ptrs, n_anchors = _anchor_args(anchors)
        d_sel, n_sel = _sel_args(sel)
        vp = lambda p: C.c_void_p(p) if p else None   # noqa: E731
        self._check("run_device", self._h, vp(d_ref), ref_bytes, vp(d_ref_off), n_refs, vp(d_seq), seq_bytes, vp(d_seq_off), n_reads,
                    *(vp(p) for p in c_ptrs + a_ptrs), n_chains, n_members, n_anchors, vp(d_sel), n_sel, C.byref(params))

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def read(self):
        """(rows, scores, g_offsets, cigar) as numpy arrays, indexed by position in the selection: rows[s] is the entry's eight words,
        named by ROW; scores[s] its score (int64); its CIGAR is cigar[g_offsets[s]: g_offsets[s + 1]], words of len << 4 | op
        (cigar_string spells them)."""
        n_s, n_c = C.c_uint64(0), C.c_uint64(0)
        rc = self._fn("read")(self._h, None, None, None, None, 0, 0, C.byref(n_s), C.byref(n_c))
        if rc not in (0, ERR_CAPACITY):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        rows, scores = np.zeros((n_s.value, 8), dtype=np.uint32), np.zeros(n_s.value, dtype=np.int64)
        g_offsets, cigar = np.zeros(n_s.value + 1, dtype=np.uint64), np.zeros(n_c.value, dtype=np.uint32)
        data = lambda x: x.ctypes.data if x.size else None   # noqa: E731
        self._check("read", self._h, data(rows), data(scores), g_offsets.ctypes.data, data(cigar), n_s.value, n_c.value, C.byref(n_s), C.byref(n_c))
        return rows, scores, g_offsets, cigar

    def device_arrays(self):
        """(d_rows, d_scores, d_g_offsets, d_cigar, n_sel, n_cigar): the held result where it lies on the device, as addresses (0 where
        nothing is held) and the two sizes.  Host-side only; the addresses stay valid until the next run, trim or close."""
        ptrs = [C.c_void_p() for _ in range(4)]
        n_s, n_c = C.c_uint64(0), C.c_uint64(0)
        self._check("result_device", self._h, *(C.byref(p) for p in ptrs), C.byref(n_s), C.byref(n_c))
        return tuple(p.value or 0 for p in ptrs) + (n_s.value, n_c.value)
