"""Seeding reads against references.  ctypes binding of libneedletail_amd_seed_index.so
(include_staged/needletail_amd/seed_index.h).

SeedIndex holds a minimizer index of a reference batch on the device and matches the minimizer lists of a read batch against it.  Both
lists are what MinimizerList makes (same k, w, path and order, which belong to the lists: the index cannot know them).  A seed - an
entry of a read - whose value is a key of the index makes one anchor (ref, rev, rpos, qpos) per occurrence, unless the key occurs more
than max_occ times; the anchors of a read are held in ascending order of (ref << 1 | rev, rpos, qpos), as a CSR that stays on the device
(device_arrays) and can be read back (read).  There is no fallback: without a gfx950 device every call of the class raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .engine import Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_seed_index.so")
PREFIX = "ntk_seed_index_"

SORT_TILE = 2048              # SI_SORT_TILE of csrc/ntk_si_rule.hpp: a read with more anchors takes the segmented-sort route
ERR_CAPACITY = 5              # NTK_ERR_CAPACITY


class Stats(C.Structure):
    _fields_ = [("n_refs", C.c_uint64), ("n_entries", C.c_uint64), ("n_keys", C.c_uint64), ("max_occ", C.c_uint64),
                ("n_reads", C.c_uint64), ("n_seeds", C.c_uint64), ("n_anchors", C.c_uint64), ("device_bytes", C.c_uint64)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
_pp = C.POINTER(C.c_void_p)
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _pp], "destroy": [_vp],
    "build_device": [_vp, _vp, _vp, _vp, _vp, _u64, _u64],
    "spectrum": [_vp, _vp, _u32],
    "match_device": [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _u32, _u64],
    "read": [_vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)],
    "result_device": [_vp, _pp, _pp, _pp, _pp, _pp, C.POINTER(_u64)],
    "stats": [_vp, C.POINTER(Stats)], "trim": [_vp],
}

# every symbol include_staged/needletail_amd/seed_index.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _list_args(ml_or_arrays):
    """(d_offsets, d_pos, d_values, d_info, n_records, n_entries) of a MinimizerList's held result, zero-copy, or of a tuple of four
    device tensors (offsets of n_records + 1 words; pos, values and info of n_entries each)."""
    if hasattr(ml_or_arrays, "device_arrays"):
        d_offsets, d_pos, d_values, d_info, n = ml_or_arrays.device_arrays()
        ptrs, n_records = (d_offsets, d_pos, d_values, d_info), ml_or_arrays.stats()["n_records"]
    else:
        offsets, pos, values, info = ml_or_arrays
        if not (pos.numel() == values.numel() == info.numel()) or offsets.numel() < 1:
            raise ValueError("a list is offsets[n_records + 1] and pos, values, info of one length")
        if offsets.element_size() != 8 or pos.element_size() != 8 or values.element_size() != 8 or info.element_size() != 4:
            raise ValueError("offsets, pos and values are 8-byte words and info 4-byte words")
        n, n_records = int(pos.numel()), int(offsets.numel()) - 1
        ptrs = (_ptr(offsets),) + tuple(_ptr(t) if n else 0 for t in (pos, values, info))
    return tuple(C.c_void_p(p) if p else None for p in ptrs) + (n_records, n)


class SeedIndex(L.Handle):
    """A minimizer index of a reference batch and the anchors of a read batch against it."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, C.byref(self._h))

    def trim(self):
        """Free the match result and every work array; the index stays."""
        self._check("trim", self._h)

    def build(self, ml_or_arrays):
        """Index the minimizer list of a reference batch: a MinimizerList that holds it, or (offsets, pos, values, info) as device
        tensors.  Returns when the index is held; it replaces the one before and drops a held match."""
        self._check("build_device", self._h, *_list_args(ml_or_arrays))

    def match(self, ml_or_arrays, max_occ: int = 0, max_anchors: int = 0):
        """Match the minimizer list of a read batch against the index.  A seed whose key occurs more than max_occ times makes no anchor
        (0: no limit).  max_anchors != 0: a batch that makes more anchors raises NtkError with status 5 (NTK_ERR_CAPACITY); the rows
        and stats()["n_anchors"], the number needed, are valid then and no anchors are held."""
        if not 0 <= max_occ < 1 << 32 or not 0 <= max_anchors < 1 << 64:
            raise ValueError("max_occ is 0..2^32 - 1 and max_anchors 0..2^64 - 1")
        self._check("match_device", self._h, *_list_args(ml_or_arrays), max_occ, max_anchors)

    def spectrum(self, n_bins: int) -> np.ndarray:
        """hist[c] = the keys that occur c times; the last bin also takes every larger occ; hist[0] = 0."""
        hist = np.zeros(n_bins, dtype=np.uint64)
        self._check("spectrum", self._h, hist.ctypes.data if n_bins else None, n_bins)
        return hist

    def occ_cutoff(self, fraction_ppm: int) -> int:
        """The max_occ that cuts the most frequent fraction of the keys, in parts per million (minimap2's -f 0.0002 is 200): the
        smallest occ c such that at most fraction_ppm / 10^6 of the keys occur more than c times.  Integer arithmetic on the spectrum;
        never below 1.  An empty index gives 1."""
        if not 0 <= fraction_ppm <= 1_000_000:
            raise ValueError("fraction_ppm is 0..1000000")
        st = self.stats()
        n_keys, top = st["n_keys"], st["max_occ"]
        if n_keys == 0:
            return 1
        hist = self.spectrum(top + 2)
        above = 0                      # keys with occ > c
        c = top
        while c > 1 and (above + int(hist[c])) * 1_000_000 <= fraction_ppm * n_keys:
            above += int(hist[c])
            c -= 1
        return c

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def read(self):
        """(a_offsets, ref, rev, rpos, qpos, rows) as numpy arrays: read q's anchors are [a_offsets[q], a_offsets[q + 1]); ref is the
        reference record, rev 1 where the read matches its reverse strand (uint8), rpos and qpos the positions of the two k-mers in
        their records; rows[q] = (n_seeds, n_hit, n_repetitive, n_absent)."""
        st = self.stats()
        n = C.c_uint64(0)
        rc = self._fn("read")(self._h, None, None, None, None, None, 0, C.byref(n))
        if rc not in (0, ERR_CAPACITY):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        a_offsets = np.zeros(st["n_reads"] + 1, dtype=np.uint64)
        rows = np.zeros((st["n_reads"], 4), dtype=np.uint32)
        ref_rev, rpos, qpos = (np.zeros(n.value, dtype=np.uint32) for _ in range(3))
        data = lambda a: a.ctypes.data if a.size else None   # noqa: E731
        self._check("read", self._h, a_offsets.ctypes.data, data(ref_rev), data(rpos), data(qpos), data(rows), n.value, C.byref(n))
        return a_offsets, ref_rev >> 1, (ref_rev & 1).astype(np.uint8), rpos, qpos, rows

    def device_arrays(self):
        """(d_a_offsets, d_ref_rev, d_rpos, d_qpos, d_rows, n): the held result where it lies on the device, as addresses (0 where
        nothing is held) and the number of anchors; ref_rev = ref << 1 | rev.  Host-side only; the addresses stay valid until the next
        build, match, trim or close."""
        ptrs = [C.c_void_p() for _ in range(5)]
        n = C.c_uint64(0)
        self._check("result_device", self._h, *(C.byref(p) for p in ptrs), C.byref(n))
        return tuple(p.value or 0 for p in ptrs) + (n.value,)
