"""Chaining seed anchors.  ctypes binding of libneedletail_amd_chain.so (include_pending/needletail_amd/chain.h).

AnchorChains runs minimap2's chaining recurrence over a fixed predecessor window and its backtrack on the anchors of a read batch: what
SeedIndex holds after a match, taken zero-copy, or four device tensors of that shape.  The result is a per-read CSR of chains with
their member anchors that stays on the device (device_arrays) and can be read back (read): per chain a score, a reference and strand
and the first and last anchor.  Integer arithmetic only: exact and deterministic.  There is no fallback: without a gfx950 device every
call of the class raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .engine import Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_chain.so")
PREFIX = "ntk_chain_"

H_MAX = 512                   # CH_H_MAX of csrc/ntk_chain_rule.hpp: the ring of the recurrence kernel
NONE = 0xFFFFFFFF             # CH_NONE: p of an anchor without a predecessor
ERR_CAPACITY = 5              # NTK_ERR_CAPACITY


class Params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("max_dist", C.c_uint32), ("bw", C.c_uint32), ("h", C.c_uint32), ("min_score", C.c_uint32),
                ("min_cnt", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_anchors", C.c_uint64), ("n_runs", C.c_uint64), ("longest_run", C.c_uint64),
                ("n_chains", C.c_uint64), ("n_members", C.c_uint64), ("reserved", C.c_uint64), ("device_bytes", C.c_uint64)]


_vp, _u64 = C.c_void_p, C.c_uint64
_pp, _pu64 = C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _pp], "destroy": [_vp],
    "run_device": [_vp, _vp, _vp, _vp, _vp, _u64, _u64, C.POINTER(Params)],
    "read": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _pu64, _pu64],
    "result_device": [_vp, _pp, _pp, _pp, _pp, _pp, _pp, _pp, _pu64, _pu64],
    "stats": [_vp, C.POINTER(Stats)], "trim": [_vp],
}

# every symbol include_pending/needletail_amd/chain.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _anchor_args(si_or_arrays):
    """(d_a_offsets, d_ref_rev, d_rpos, d_qpos, n_reads, n_anchors) of a SeedIndex's held match, zero-copy, or of a tuple of four device
    tensors (offsets of n_reads + 1 8-byte words; ref_rev, rpos and qpos of n_anchors 4-byte words each)."""
    if hasattr(si_or_arrays, "device_arrays"):
        d_a_offsets, d_ref_rev, d_rpos, d_qpos, _, n = si_or_arrays.device_arrays()
        if not d_a_offsets:
            raise ValueError("the seed index holds no match")
        ptrs, n_reads = (d_a_offsets, d_ref_rev, d_rpos, d_qpos), si_or_arrays.stats()["n_reads"]
    else:
        offsets, ref_rev, rpos, qpos = si_or_arrays
        if not (ref_rev.numel() == rpos.numel() == qpos.numel()) or offsets.numel() < 1:
            raise ValueError("the anchors are offsets[n_reads + 1] and ref_rev, rpos, qpos of one length")
        if offsets.element_size() != 8 or ref_rev.element_size() != 4 or rpos.element_size() != 4 or qpos.element_size() != 4:
            raise ValueError("offsets are 8-byte words and ref_rev, rpos and qpos 4-byte words")
        n, n_reads = int(rpos.numel()), int(offsets.numel()) - 1
        ptrs = (_ptr(offsets),) + tuple(_ptr(t) if n else 0 for t in (ref_rev, rpos, qpos))
    return tuple(C.c_void_p(p) if p else None for p in ptrs) + (n_reads, n)


class AnchorChains(L.Handle):
    """The colinear chains of the anchors of a read batch."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, C.byref(self._h))

    def trim(self):
        """Free the result and every work array."""
        self._check("trim", self._h)

    def run(self, seed_index_or_arrays, k: int, max_dist: int = 5000, bw: int = 500, h: int = 64, min_score: int = 40, min_cnt: int = 3):
        """Chain the anchors a SeedIndex holds after a match, or (a_offsets, ref_rev, rpos, qpos) as device tensors.  k is the seed
        length of the lists the anchors came from; the other parameters are minimap2's, with its defaults.  Returns when the result is
        held; it replaces the one before.  Parameters out of range and arrays that are not a sorted anchor CSR raise NtkError with
        status 2 (NTK_ERR_BAD_ARG) and leave the held result as it was."""
        values = (k, max_dist, bw, h, min_score, min_cnt)
        if not all(0 <= v < 1 << 32 for v in values):
            raise ValueError("the parameters are 32-bit words")
        params = Params(*values)
        self._check("run_device", self._h, *_anchor_args(seed_index_or_arrays), C.byref(params))

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def read(self):
        """(c_offsets, chain_rows, m_offsets, members, f, p, read_rows) as numpy arrays: read q's chains are
        [c_offsets[q], c_offsets[q + 1]) in the order found; chain_rows[c] = (score, n_members, ref_rev, rpos and qpos of the first member,
        rpos and qpos of the last member, 0); chain c's members are members[m_offsets[c]: m_offsets[c + 1]], ascending indices into the
        batch's anchor arrays; f (int32) and p (NONE: no predecessor) per anchor; read_rows[q] = (n_anchors, n_chains, anchors in kept
        chains, best score)."""
        st = self.stats()
        n_c, n_m = C.c_uint64(0), C.c_uint64(0)
        rc = self._fn("read")(self._h, None, None, None, None, None, None, None, 0, 0, C.byref(n_c), C.byref(n_m))
        if rc not in (0, ERR_CAPACITY):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        c_offsets = np.zeros(st["n_reads"] + 1, dtype=np.uint64)
        chain_rows, m_offsets = np.zeros((n_c.value, 8), dtype=np.uint32), np.zeros(n_c.value + 1, dtype=np.uint64)
        members = np.zeros(n_m.value, dtype=np.uint32)
        f, p = np.zeros(st["n_anchors"], dtype=np.int32), np.zeros(st["n_anchors"], dtype=np.uint32)
        read_rows = np.zeros((st["n_reads"], 4), dtype=np.uint32)
        data = lambda a: a.ctypes.data if a.size else None   # noqa: E731
        self._check("read", self._h, c_offsets.ctypes.data, data(chain_rows), m_offsets.ctypes.data, data(members), data(f), data(p),
                    data(read_rows), n_c.value, n_m.value, C.byref(n_c), C.byref(n_m))
        return c_offsets, chain_rows, m_offsets, members, f, p, read_rows

    def device_arrays(self):
        """(d_c_offsets, d_chain_rows, d_m_offsets, d_members, d_f, d_p, d_read_rows, n_chains, n_members): the held result where it
        lies on the device, as addresses (0 where nothing is held) and the two sizes.  Host-side only; the addresses stay valid until
        the next run, trim or close."""
        ptrs = [C.c_void_p() for _ in range(7)]
        n_c, n_m = C.c_uint64(0), C.c_uint64(0)
        self._check("result_device", self._h, *(C.byref(p) for p in ptrs), C.byref(n_c), C.byref(n_m))
        return tuple(p.value or 0 for p in ptrs) + (n_c.value, n_m.value)
