"""The compacted de Bruijn graph of a k-mer set.  ctypes binding of libneedletail_amd_dbg.so (include/needletail_amd_dbg.h).

KmerGraph takes a KmerSet of canonical k-mers (odd k, 3..31), as a count table's extract or a set operation leaves it on the device,
and answers on the device: the edge byte of every k-mer with exact degree totals (tips, branch points, isolated k-mers), the unitigs
with their lengths and summed counts, and the unitigs spelled out as a device batch that the count tables, the sketches, MinHash and
the trimmer take as it is.  There is no fallback: without a gfx950 device every call raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .kmer_sets import KmerSet

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_dbg.so")
PREFIX = "ntk_dbg_"

K_MIN, K_MAX = 3, 31                       # NTK_DBG_K_MIN, NTK_DBG_K_MAX
N_MAX = 0x7FFFFFFF                         # NTK_DBG_N_MAX
UNITIG_BYTES_PER_KMER = 96                 # NTK_DBG_UNITIG_BYTES_PER_KMER
FLAG_CYCLE = 1                             # NTK_DBG_FLAG_CYCLE
NTK_ERR_BAD_K, NTK_ERR_CAPACITY, NTK_ERR_UNSUPPORTED = 1, 5, 6
# the words of a unitig row (struct ntk_dbg_unitig_row) and of a k-mer row (struct ntk_dbg_kmer_row), in order
UNITIG_COLUMNS = ("start_index", "n_kmers", "sum_counts", "flags")
KMER_COLUMNS = ("unitig", "pos_flip")


class Stats(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("k", "device_bytes", "n_launches", "n_calls", "n_rounds")]


class Totals(C.Structure):
    _fields_ = [("n_half_edges", C.c_uint64), ("deg_hist", C.c_uint64 * 5 * 5), ("n_isolated", C.c_uint64), ("n_tips", C.c_uint64),
                ("n_branching", C.c_uint64), ("n_self", C.c_uint64), ("n_links", C.c_uint64)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, C.POINTER(_vp)], "destroy": [_vp], "release": [_vp], "stats": [_vp, C.POINTER(Stats)],
    "adjacency_device": [_vp, _vp, _u64, _vp, C.POINTER(Totals)],
    "unitigs_device": [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)],
    "spell_device": [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)],
}

# every symbol include/needletail_amd_dbg.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


class Unitigs:
    """What KmerGraph.unitigs() returns.  kmer_rows: a device int32 tensor of shape (n, 2), columns KMER_COLUMNS (pos_flip = position
    << 1 | flipped); unitig_rows: a device int64 tensor of shape (n_unitigs, 4) holding the uint64 words UNITIG_COLUMNS; n_unitigs and
    n_bases: integers."""

    def __init__(self, kmer_rows, unitig_rows, n_unitigs: int, n_bases: int):
        self.kmer_rows, self.unitig_rows, self.n_unitigs, self.n_bases = kmer_rows, unitig_rows, n_unitigs, n_bases

    def __iter__(self):
        return iter((self.kmer_rows, self.unitig_rows, self.n_unitigs, self.n_bases))


class KmerGraph(L.Handle):
    """The de Bruijn graph of `kmer_set`, a KmerSet of canonical k-mers with odd k in 3..31, which it borrows (the set's tensors are
    read by every call)."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, kmer_set: KmerSet):
        if not isinstance(kmer_set, KmerSet):
            raise TypeError(f"KmerGraph takes a KmerSet, not {type(kmer_set).__name__}")
        if kmer_set.path == L.PATH_BITS:
            raise L.NtkError(NTK_ERR_UNSUPPORTED, "KmerGraph: the keys of a PATH_BITS set are not canonical")
        if not (K_MIN <= kmer_set.k <= K_MAX and kmer_set.k % 2 == 1):
            raise L.NtkError(NTK_ERR_BAD_K, f"KmerGraph: k is odd and {K_MIN}..{K_MAX}, not {kmer_set.k}")
        if kmer_set.n > N_MAX:
            raise L.NtkError(NTK_ERR_UNSUPPORTED, f"KmerGraph: at most {N_MAX} k-mers")
        self.set, self.ctx, self.k, self.n = kmer_set, kmer_set.ctx, kmer_set.k, kmer_set.n
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, self.k, C.byref(self._h))
        self._unitigs = None

    @property
    def _device(self):
        return self.set.keys.device

    def _sync(self):
        import torch
        torch.cuda.synchronize(self._device)   # the set, and the tensors made here, may have been written on torch's stream

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def release(self):
        """Free the scratch the calls of this graph grew."""
        self._check("release", self._h)

    def _adjacency(self, with_edges: bool):
        import torch
        edges = torch.zeros(max(self.n, 1), dtype=torch.uint8, device=self._device) if with_edges else None
        t = Totals()
        self._sync()
        self._check("adjacency_device", self._h, self.set._list()[0], self.n, None if edges is None else C.c_void_p(edges.data_ptr()),
                    C.byref(t))
        totals = {name: int(getattr(t, name)) for name, _ in Totals._fields_ if name != "deg_hist"}
        totals["deg_hist"] = np.array([[int(v) for v in row] for row in t.deg_hist], dtype=np.uint64)
        return (None if edges is None else edges[: self.n]), totals

    def edges(self):
        """The edge bytes: a device uint8 tensor, one per k-mer of the set, bit 4 * side + c set iff that neighbour is in the set."""
        return self._adjacency(True)[0]

    def totals(self) -> dict:
        """The exact totals of struct ntk_dbg_totals: integers, and deg_hist as a (5, 5) uint64 array."""
        return self._adjacency(False)[1]

    def unitigs(self) -> Unitigs:
        """The unitigs (computed once per graph): see Unitigs."""
        import torch
        if self._unitigs is not None:
            return self._unitigs
        n, dev = self.n, self._device
        kmer_rows = torch.zeros((max(n, 1), 2), dtype=torch.int32, device=dev)
        keys, counts, _ = self.set._list()
        nu, nb = _u64(0), _u64(0)
        # a first capacity that most lists fit (a quarter of the k-mers: 8 B per k-mer), so that the graph is ranked once; the call says
        # what is needed when it does not, and writes nothing then
        cap = min(n, max(1024, n // 4))
        unitig_rows = torch.zeros((max(cap, 1), 4), dtype=torch.int64, device=dev)
        if n:
            self._sync()
            rc = self._fn("unitigs_device")(self._h, keys, counts, n, C.c_void_p(kmer_rows.data_ptr()), C.c_void_p(unitig_rows.data_ptr()), cap,
                                            C.byref(nu), C.byref(nb))
            if rc == NTK_ERR_CAPACITY and nu.value > cap:
                cap = int(nu.value)
                unitig_rows = torch.zeros((cap, 4), dtype=torch.int64, device=dev)
                self._sync()
                rc = self._fn("unitigs_device")(self._h, keys, counts, n, C.c_void_p(kmer_rows.data_ptr()), C.c_void_p(unitig_rows.data_ptr()),
                                                cap, C.byref(nu), C.byref(nb))
            L.check(rc, PREFIX + "unitigs_device")
        cap = int(nu.value)
        if 2 * cap < unitig_rows.shape[0]:   # do not pin a buffer sized for the first capacity behind a small result
            unitig_rows = unitig_rows[: max(cap, 1)].clone()
        self._unitigs = Unitigs(kmer_rows[:n], unitig_rows[:cap], int(nu.value), int(nb.value))
        return self._unitigs

    def unitig_batch(self):
        """The unitigs spelled as a device batch: (seq, n_bytes, offsets, n_records).  seq: a uint8 tensor, every unitig's upper-case bases
        and one break byte, padded with break bytes to a multiple of 16 and 64 more; offsets: the n_records + 1 int64 record starts.
        KmerTable.count_device(seq, n_bytes, PRE_NORMALIZE) and the other batch calls take it as it is."""
        import torch
        u = self.unitigs()
        dev = self._device
        n_bytes = self.n + u.n_unitigs * self.k   # every k-mer's first base, and k - 1 bases and a break byte per unitig
        cap_bytes = (n_bytes + 15) // 16 * 16
        seq = torch.full((cap_bytes + 64,), ord("\n"), dtype=torch.uint8, device=dev)
        offsets = torch.zeros(u.n_unitigs + 1, dtype=torch.int64, device=dev)
        nb, nr = _u64(0), _u64(0)
        self._sync()
        self._check("spell_device", self._h, self.set._list()[0], self.n, C.c_void_p(u.kmer_rows.data_ptr()) if self.n else None,
                    C.c_void_p(u.unitig_rows.data_ptr()) if u.n_unitigs else None, u.n_unitigs, C.c_void_p(seq.data_ptr()), cap_bytes,
                    C.c_void_p(offsets.data_ptr()), u.n_unitigs, C.byref(nb), C.byref(nr))
        return seq, int(nb.value), offsets, int(nr.value)

    def unitig_sequences(self):
        """The spelled unitigs as a list of str, copied to the host."""
        seq, n_bytes, offsets, n_records = self.unitig_batch()
        text, off = seq[:n_bytes].cpu().numpy().tobytes(), offsets.cpu().numpy()
        return [text[int(off[i]): int(off[i + 1]) - 1].decode() for i in range(n_records)]
