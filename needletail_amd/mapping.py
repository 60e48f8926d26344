"""Primary and secondary chains and their mapping quality.  ctypes binding of libneedletail_amd_mapping.so
(include_pending/needletail_amd/mapping.h).

ChainMappings runs minimap2's mm_set_parent with a hard mask level, mm_select_sub and its chain-only mapping quality on the chains of a
read batch: what AnchorChains holds after a run, taken zero-copy with the anchors a SeedIndex holds, or device tensors of that shape.
The result is a row of sixteen words per chain - the columns of a PAF line - and per read the chains to report; it stays on the device
(device_arrays) and can be read back (read).  Integer arithmetic only: exact and deterministic.  ReadMapper composes the five stages
from sequences to reported mappings.  There is no fallback: without a gfx950 device every call of the classes raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .engine import Context, _ptr, default_context

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_mapping.so")
PREFIX = "ntk_mapping_"

LDS_CHAINS = 512              # MP_LDS_CHAINS of csrc/ntk_map_rule.hpp: a read with more chains takes the parent loop from global memory
READ_CHAINS = 1 << 16         # MP_READ_CHAINS: a read with this many chains or more is refused
ERR_CAPACITY = 5              # NTK_ERR_CAPACITY
ROW = ("qs", "qe", "rs", "re", "ref_rev", "score", "cnt", "mlen", "blen", "parent", "subsc", "n_sub", "mapq", "flags", "rank", "zero")
PRIMARY, SECONDARY = 1, 2     # the flags of a row


class Params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("mask_level_pm", C.c_uint32), ("pri_ratio_pm", C.c_uint32), ("best_n", C.c_uint32),
                ("min_chain_score", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_chains", C.c_uint64), ("n_primary", C.c_uint64), ("n_secondary", C.c_uint64),
                ("n_reported", C.c_uint64), ("most_chains", C.c_uint64), ("reserved", C.c_uint64), ("device_bytes", C.c_uint64)]


_vp, _u64 = C.c_void_p, C.c_uint64
_pp, _pu64 = C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _pp], "destroy": [_vp],
    "run_device": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(Params)],
    "read": [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _pu64, _pu64],
    "result_device": [_vp, _pp, _pp, _pp, _pp, _pp, _pu64, _pu64],
    "stats": [_vp, C.POINTER(Stats)], "trim": [_vp],
}

# every symbol include_pending/needletail_amd/mapping.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _chain_args(chains):
    """(d_c_offsets, d_chain_rows, d_m_offsets, d_members, n_reads, n_chains, n_members) of an AnchorChains' held result, zero-copy, or of
    a tuple of four device tensors (c_offsets of n_reads + 1 and m_offsets of n_chains + 1 8-byte words; chain_rows of 8 * n_chains and
    members of n_members 4-byte words)."""
    if hasattr(chains, "device_arrays"):
        d_c_offsets, d_chain_rows, d_m_offsets, d_members, _, _, _, n_chains, n_members = chains.device_arrays()
        if not d_c_offsets:
            raise ValueError("the chains hold no result")
        return (d_c_offsets, d_chain_rows, d_m_offsets, d_members), chains.stats()["n_reads"], n_chains, n_members
    c_offsets, chain_rows, m_offsets, members = chains
    if c_offsets.numel() < 1 or m_offsets.numel() < 1 or chain_rows.numel() != 8 * (m_offsets.numel() - 1):
        raise ValueError("the chains are c_offsets[n_reads + 1], chain_rows[8 * n_chains], m_offsets[n_chains + 1] and members")
    if c_offsets.element_size() != 8 or m_offsets.element_size() != 8 or chain_rows.element_size() != 4 or members.element_size() != 4:
        raise ValueError("c_offsets and m_offsets are 8-byte words and chain_rows and members 4-byte words")
    n_chains, n_members = int(m_offsets.numel()) - 1, int(members.numel())
    ptrs = (_ptr(c_offsets), _ptr(chain_rows) if n_chains else 0, _ptr(m_offsets), _ptr(members) if n_members else 0)
    return ptrs, int(c_offsets.numel()) - 1, n_chains, n_members


def _anchor_args(anchors):
    """(d_rpos, d_qpos, n_anchors) of a SeedIndex's held match, zero-copy, or of a tuple of two device tensors of 4-byte words."""
    if hasattr(anchors, "device_arrays"):
        _, _, d_rpos, d_qpos, _, n = anchors.device_arrays()
        return (d_rpos, d_qpos), n
    rpos, qpos = anchors
    if rpos.numel() != qpos.numel() or rpos.element_size() != 4 or qpos.element_size() != 4:
        raise ValueError("the anchors are rpos and qpos, 4-byte words of one length")
    n = int(rpos.numel())
    return (_ptr(rpos) if n else 0, _ptr(qpos) if n else 0), n


def per_mille(fraction: float) -> int:
    """A fraction as the library takes it."""
    return int(round(fraction * 1000))


class ChainMappings(L.Handle):
    """The primary and secondary chains of the reads of a batch, each with the columns of a PAF line and a mapping quality."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, C.byref(self._h))

    def trim(self):
        """Free the result and every work array."""
        self._check("trim", self._h)

    def run(self, chains, anchors, k: int, mask_level: float = 0.5, pri_ratio: float = 0.8, best_n: int = 5, min_chain_score: int = 40):
        """Mark the chains an AnchorChains holds after a run, or (c_offsets, chain_rows, m_offsets, members) as device tensors, over the
        anchors a SeedIndex holds after a match, or (rpos, qpos) as device tensors.  k is the seed length of the lists the anchors came
        from; the other parameters are minimap2's, with its defaults; the two fractions are rounded to per mille.  Returns when the
        result is held; it replaces the one before.  Parameters out of range and arrays that are not a chain CSR raise NtkError with
        status 2 (NTK_ERR_BAD_ARG) and leave the held result as it was."""
        values = (k, per_mille(mask_level), per_mille(pri_ratio), best_n, min_chain_score)
        if not all(0 <= v < 1 << 32 for v in values):
            raise ValueError("the parameters are 32-bit words")
        params = Params(*values)
        c_ptrs, n_reads, n_chains, n_members = _chain_args(chains)
        a_ptrs, n_anchors = _anchor_args(anchors)
        self._check("run_device", self._h, *(C.c_void_p(p) if p else None for p in c_ptrs + a_ptrs), n_reads, n_chains, n_members, n_anchors,
                    C.byref(params))

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def read(self):
        """(rows, order, out_offsets, out, read_rows) as numpy arrays: rows[c] is chain c's sixteen words, named by ROW; read q's chains
        by rank are order[c_offsets[q]: c_offsets[q + 1]] under the offsets of the chains; the chains to report for it, primaries and kept
        secondaries by rank, are out[out_offsets[q]: out_offsets[q + 1]]; read_rows[q] = (chains, primaries, kept secondaries, the mapq
        of the rank-0 chain)."""
        st = self.stats()
        n_c, n_o = C.c_uint64(0), C.c_uint64(0)
        rc = self._fn("read")(self._h, None, None, None, None, None, 0, 0, C.byref(n_c), C.byref(n_o))
        if rc not in (0, ERR_CAPACITY):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        rows, order = np.zeros((n_c.value, 16), dtype=np.uint32), np.zeros(n_c.value, dtype=np.uint32)
        out_offsets, out = np.zeros(st["n_reads"] + 1, dtype=np.uint64), np.zeros(n_o.value, dtype=np.uint32)
        read_rows = np.zeros((st["n_reads"], 4), dtype=np.uint32)
        data = lambda a: a.ctypes.data if a.size else None   # noqa: E731
        self._check("read", self._h, data(rows), data(order), out_offsets.ctypes.data, data(out), data(read_rows), n_c.value, n_o.value,
                    C.byref(n_c), C.byref(n_o))
        return rows, order, out_offsets, out, read_rows

    def device_arrays(self):
        """(d_rows, d_order, d_out_offsets, d_out, d_read_rows, n_chains, n_out): the held result where it lies on the device, as
        addresses (0 where nothing is held) and the two sizes.  Host-side only; the addresses stay valid until the next run, trim or
        close."""
        ptrs = [C.c_void_p() for _ in range(5)]
        n_c, n_o = C.c_uint64(0), C.c_uint64(0)
        self._check("result_device", self._h, *(C.byref(p) for p in ptrs), C.byref(n_c), C.byref(n_o))
        return tuple(p.value or 0 for p in ptrs) + (n_c.value, n_o.value)


class _DeviceWords:
    """n words at a device address, as torch takes them."""

    def __init__(self, address, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}


MAPPING = np.dtype([("read", np.uint32), ("qs", np.uint32), ("qe", np.uint32), ("strand", "S1"), ("ref", np.uint32), ("rs", np.uint32),
                    ("re", np.uint32), ("mlen", np.uint32), ("blen", np.uint32), ("mapq", np.uint8), ("primary", np.bool_), ("score", np.uint32),
                    ("cnt", np.uint32)])


class ReadMapper:
    """Reads mapped against references: two minimizer lists, a seed index, the chains and their marks, each stage's result taken by the
    next where it lies on the device.  The seeds are the (w, k) minimizers of the bit-canonical path under `order`."""

    def __init__(self, k: int = 15, w: int = 10, order: int = None, ctx: Context = None):
        from .chaining import AnchorChains
        from .minimizer_lists import HASH, MinimizerList
        from .seeding import SeedIndex
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.w = k, w
        order = HASH if order is None else order
        self.refs = MinimizerList(k, L.PATH_BITS_CANONICAL, w, order, self.ctx)
        self.reads = MinimizerList(k, L.PATH_BITS_CANONICAL, w, order, self.ctx)
        self.seeds, self.chains, self.mappings = SeedIndex(self.ctx), AnchorChains(self.ctx), ChainMappings(self.ctx)
        self.alignments = None    # a ChainAlignments, made by the first map_aligned
        self._ref_batch = None    # the reference batch index() was given

    def close(self):
        for h in (self.alignments, self.mappings, self.chains, self.seeds, self.reads, self.refs):
            if h is not None:
                h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def index(self, dev, n_bytes: int, offsets, n_records: int, pre: int = L.PRE_NORMALIZE):
        """List and index the references: a device batch and its n_records + 1 record offsets on the device.  The batch is remembered
        for map_aligned, which reads its bases: the caller keeps `dev` and `offsets` alive and unchanged until the last map_aligned."""
        self.refs.run_device(dev, n_bytes, offsets, n_records, pre)
        self.seeds.build(self.refs)
        self._ref_batch = (dev, n_bytes, offsets, n_records)

    def index_records(self, records, pre: int = L.PRE_NORMALIZE):
        """index() of host sequences, packed and uploaded by the batch packer."""
        self.refs.run_records(records, pre)
        self.seeds.build(self.refs)
        self._ref_batch = None    # (the packer's upload is not kept: map_aligned needs index())

    def map(self, dev, n_bytes: int, offsets, n_reads: int, pre: int = L.PRE_NORMALIZE, max_occ: int = 0, max_dist: int = 5000, bw: int = 500,
            h: int = 64, min_score: int = 40, min_cnt: int = 3, mask_level: float = 0.5, pri_ratio: float = 0.8, best_n: int = 5):
        """Map the reads of a device batch: one structured array (dtype MAPPING) of the reported mappings, primaries and kept
        secondaries, read by read and by rank within a read.  Only those rows leave the device."""
        self.reads.run_device(dev, n_bytes, offsets, n_reads, pre)
        return self._map(max_occ, max_dist, bw, h, min_score, min_cnt, mask_level, pri_ratio, best_n)

    def map_aligned(self, dev, n_bytes: int, offsets, n_reads: int, pre: int = L.PRE_NORMALIZE, max_occ: int = 0, max_dist: int = 5000,
                    bw: int = 500, h: int = 64, min_score: int = 40, min_cnt: int = 3, mask_level: float = 0.5, pri_ratio: float = 0.8,
                    best_n: int = 5, a: int = 2, b: int = 4, q: int = 4, e: int = 2, band_pad: int = 64, max_seg: int = 2048, work_mib: int = 0):
        """map(), then every reported chain aligned base by base (ChainAlignments): (mappings, rows, scores, g_offsets, cigar), the
        structured array of map() and, entry by entry in the order of its rows, what ChainAlignments.read returns.  The references must
        have been indexed by index(), whose batch is read here; after index_records this raises ValueError."""
        if self._ref_batch is None:
            raise ValueError("map_aligned reads the reference batch: index the references with index(), not index_records()")
        from .aligning import ChainAlignments
        got = self.map(dev, n_bytes, offsets, n_reads, pre, max_occ, max_dist, bw, h, min_score, min_cnt, mask_level, pri_ratio, best_n)
        if self.alignments is None:
            self.alignments = ChainAlignments(self.ctx)
        self.alignments.run(self._ref_batch, (dev, n_bytes, offsets, n_reads), self.chains, self.seeds, self.mappings, self.k, a, b, q, e, band_pad,
                            max_seg, work_mib)
        return (got,) + self.alignments.read()

    def map_records(self, records, pre: int = L.PRE_NORMALIZE, **kw):
        """map() of host sequences, packed and uploaded by the batch packer."""
        self.reads.run_records(records, pre)
        return self._map(**{**dict(max_occ=0, max_dist=5000, bw=500, h=64, min_score=40, min_cnt=3, mask_level=0.5, pri_ratio=0.8, best_n=5), **kw})

    def _map(self, max_occ, max_dist, bw, h, min_score, min_cnt, mask_level, pri_ratio, best_n):
        import torch
        self.seeds.match(self.reads, max_occ)
        self.chains.run(self.seeds, self.k, max_dist, bw, h, min_score, min_cnt)
        self.mappings.run(self.chains, self.seeds, self.k, mask_level, pri_ratio, best_n, min_score)
        d_rows, _, d_out_offsets, d_out, _, n_chains, n_out = self.mappings.device_arrays()
        n_reads = self.mappings.stats()["n_reads"]
        got = np.zeros(n_out, dtype=MAPPING)
        if not n_out:
            return got
        device = "cuda:%d" % self.ctx.device
        # (run returned when the result was complete, so any stream may read it)
        rows = torch.as_tensor(_DeviceWords(d_rows, 16 * n_chains, "<i4"), device=device).view(-1, 16)
        out = torch.as_tensor(_DeviceWords(d_out, n_out, "<i4"), device=device).to(torch.int64) & 0xFFFFFFFF
        sel = rows[out].cpu().numpy().view(np.uint32)
        offs = torch.as_tensor(_DeviceWords(d_out_offsets, n_reads + 1, "<i8"), device=device).cpu().numpy()
        got["read"] = np.repeat(np.arange(n_reads, dtype=np.uint32), np.diff(offs))
        for name, word in (("qs", 0), ("qe", 1), ("rs", 2), ("re", 3), ("score", 5), ("cnt", 6), ("mlen", 7), ("blen", 8), ("mapq", 12)):
            got[name] = sel[:, word]
        got["strand"] = np.where(sel[:, 4] & 1, b"-", b"+")
        got["ref"] = sel[:, 4] >> 1
        got["primary"] = (sel[:, 13] & PRIMARY) != 0
        return got

