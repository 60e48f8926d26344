"""Many samples against many.  ctypes binding of libneedletail_amd_minhash_set.so (include/needletail_amd_minhash_set.h).

MinHashSet keeps MinHash sketches (what KmerMinHash.hashes() returns: ascending hashes with their counts) on the device and compares a
block of rows with a block of columns, pair by pair, in one pass on the GPU; every pair's numbers are those of minhashing.compare for it.
On top of that: the Jaccard, containment, cosine and Mash-distance matrices, and search(), one query against the whole set.  There is
no fallback: without a gfx950 device every call of the class raises."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib as L
from .engine import Context, default_context
from .minhashing import ALL, KmerMinHash, _data, _u64_array

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_minhash_set.so")
PREFIX = "ntk_mhset_"

BLOCK_DEFAULT = 1 << 20                 # NTK_MHSET_BLOCK_DEFAULT
BLOCK_MIN, BLOCK_MAX = 1, 1 << 26       # NTK_MHSET_BLOCK_MIN, NTK_MHSET_BLOCK_MAX
STAGE = 2048                            # NTK_MHSET_STAGE
MATRICES = ("n_shared", "n_union", "dot", "norm2_a", "norm2_b")
_DTYPES = {"n_shared": np.uint32, "n_union": np.uint32, "dot": np.float64, "norm2_a": np.float64, "norm2_b": np.float64}


class Stats(C.Structure):
    _fields_ = [("n_sketches", C.c_uint64), ("n_entries", C.c_uint64), ("abundance", C.c_uint64), ("block_pairs", C.c_uint64),
                ("device_bytes", C.c_uint64), ("n_launches", C.c_uint64), ("n_uploads", C.c_uint64)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, _u64, C.POINTER(_vp)], "destroy": [_vp], "reset": [_vp],
    "add": [_vp, _vp, _vp, _u64, C.POINTER(_u64)], "read": [_vp, _u64, _vp, _vp, _u64, C.POINTER(_u64)],
    "stats": [_vp, C.POINTER(Stats)],
    "compare": [_vp, _u64, _u64, _vp, _u64, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}

# every symbol include/needletail_amd_minhash_set.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _range(r, n: int):
    """(first, count) of a range given as None (everything), an int (that one), a (first, end) pair, a range or a slice of step 1."""
    if r is None:
        return 0, n
    if isinstance(r, (int, np.integer)):
        return int(r), 1
    if isinstance(r, slice):
        r = range(*r.indices(n))
    if isinstance(r, range):
        if r.step != 1:
            raise L.NtkError(2, "a range of sketches has step 1")
        return r.start, max(0, r.stop - r.start)
    first, end = r
    return int(first), max(0, int(end) - int(first))


def _ratio(num, den):
    """num / den where den is non-zero, 0.0 elsewhere (the rule of KmerMinHash.jaccard and the others)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.zeros(np.broadcast(num, den).shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


class MinHashSet(L.Handle):
    """A set of sketches on the device.  abundance=False stores no counts (every count is 1); block_pairs is the number of pairs one
    launch covers (a memory knob: 32 B of result scratch per pair; 0 is BLOCK_DEFAULT)."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, abundance: bool = False, ctx: Context = None, block_pairs: int = 0):
        self.ctx = ctx if ctx is not None else default_context()
        self.abundance = bool(abundance)
        self.k = self.path = self.num = self.scaled = self.max_hash = None   # of the first KmerMinHash added
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, int(self.abundance), block_pairs, C.byref(self._h))

    def reset(self):
        self._check("reset", self._h)
        self.k = self.path = self.num = self.scaled = self.max_hash = None

    def _admit(self, mh: KmerMinHash):
        """The checks of KmerMinHash.compare, against what the first handle recorded."""
        if self.k is None:
            return
        if (mh.k, mh.path) != (self.k, self.path):
            raise L.NtkError(2, "adding a sketch of a different k or path")
        if bool(mh.num) != bool(self.num):
            raise L.NtkError(2, "adding a bottom-s sketch to scaled ones, or a scaled one to bottom-s sketches")

    def add(self, sketch) -> int:
        """Append a KmerMinHash, or a (hashes, counts) pair of ascending uint64 hashes and their counts (None: every count 1); returns
        its index.  The first KmerMinHash fixes k, path and the kind; compare() then defaults to the smallest num and max_hash added."""
        mh = sketch if isinstance(sketch, KmerMinHash) else None
        if mh is not None:
            self._admit(mh)
            hashes, counts = mh.hashes()
        else:
            hashes, counts = sketch
        hashes, counts = _u64_array(hashes, "hashes"), _u64_array(counts, "counts")
        if hashes is None or (counts is not None and counts.size != hashes.size):
            raise L.NtkError(2, PREFIX + "add")
        if not self.abundance and mh is not None:
            counts = None   # a flat set takes the hashes of a handle
        index = C.c_uint64(0)
        self._check("add", self._h, _data(hashes), _data(counts), hashes.size, C.byref(index))
        if mh is not None:
            if self.k is None:
                self.k, self.path, self.num, self.scaled, self.max_hash = mh.k, mh.path, mh.num, mh.scaled, mh.max_hash
            else:
                self.num, self.max_hash = min(self.num, mh.num), min(self.max_hash, mh.max_hash)
        return index.value

    def add_record_sketches(self, rmh) -> range:
        """Append every record's sketch of a RecordMinHash, in record order; returns the range of their indices.  The checks are those
        add() makes for a KmerMinHash of the handle's k, path and kind, made before anything is added, as is the check that every
        sketch ascends strictly.  Not atomic beyond that: if an add fails halfway (out of memory), the sketches added so far stay,
        and k, path and kind are recorded for them."""
        self._admit(rmh)
        offsets, _, hashes, counts = rmh.sketches()
        n = offsets.size - 1
        inner = np.ones(hashes.size, dtype=bool)
        inner[offsets[:-1][offsets[:-1] < hashes.size].astype(np.int64)] = False   # the first entry of every sketch
        if hashes.size > 1 and not (hashes[1:] > hashes[:-1])[inner[1:]].all():
            raise L.NtkError(2, PREFIX + "add: a record's hashes do not ascend")
        first, added = len(self), 0
        try:
            for r in range(n):
                h, c = hashes[int(offsets[r]):int(offsets[r + 1])], counts[int(offsets[r]):int(offsets[r + 1])]
                self._check("add", self._h, _data(h), _data(c) if self.abundance else None, h.size, None)
                added += 1
        finally:
            if added and self.k is None:
                self.k, self.path, self.num, self.scaled, self.max_hash = rmh.k, rmh.path, rmh.num, rmh.scaled, rmh.max_hash
            elif added:
                self.num, self.max_hash = min(self.num, rmh.num), min(self.max_hash, rmh.max_hash)
        return range(first, first + n)

    def __len__(self) -> int:
        return self.stats()["n_sketches"]

    def stats(self) -> dict:
        s = Stats()
        self._check("stats", self._h, C.byref(s))
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def sketch(self, i: int):
        """(hashes, counts) of sketch i, read back from the device."""
        n = C.c_uint64(0)
        rc = lib().ntk_mhset_read(self._h, i, None, None, 0, C.byref(n))
        if rc not in (0, 5):   # NTK_ERR_CAPACITY answers the size query
            L.check(rc, PREFIX + "read")
        h, c = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._check("read", self._h, i, h.ctypes.data, c.ctypes.data, n.value, C.byref(n))
        return h, c

    def compare(self, rows=None, cols=None, other: "MinHashSet" = None, num: int = None, max_hash: int = None, want=MATRICES) -> dict:
        """Rows `rows` of this set against columns `cols` of `other` (this set when None): a dict of numpy arrays shaped (n_rows,
        n_cols) for every name in `want` (of MATRICES), plus the vectors n_a (per row) and n_b (per column).  num and max_hash default to
        what the handles added so far recorded (0 and everything on a set of bare arrays)."""
        cols_set = self if other is None else other
        r0, nr = _range(rows, len(self))
        c0, nc = _range(cols, len(cols_set))
        if num is None:
            num = min(s.num or 0 for s in (self, cols_set))
        if max_hash is None:
            max_hash = min(ALL if s.max_hash is None else s.max_hash for s in (self, cols_set))
        unknown = set(want) - set(MATRICES)
        if unknown:
            raise ValueError(f"want: {sorted(unknown)} not in {MATRICES}")
        out = {name: np.zeros((nr, nc), dtype=_DTYPES[name]) for name in MATRICES if name in want}
        out["n_a"], out["n_b"] = np.zeros(nr, dtype=np.uint64), np.zeros(nc, dtype=np.uint64)
        ptr = lambda name: out[name].ctypes.data if name in out and out[name].size else None
        self._check("compare", self._h, r0, nr, cols_set._h, c0, nc, num, max_hash, *(ptr(m) for m in MATRICES), ptr("n_a"), ptr("n_b"))
        return out

    def _square(self, want, num=None, max_hash=None, tile: int = 1024) -> dict:
        """The square matrix of the set from the blocks with c >= r, mirrored (norm2_a and norm2_b swap under the mirror)."""
        n = len(self)
        out = {name: np.zeros((n, n), dtype=_DTYPES[name]) for name in want}
        out["n_a"] = np.zeros(n, dtype=np.uint64)   # of one set: also its n_b
        mirror = {"norm2_a": "norm2_b", "norm2_b": "norm2_a"}
        for r in range(0, n, tile):
            for c in range(r, n, tile):
                blk = self.compare((r, min(n, r + tile)), (c, min(n, c + tile)), num=num, max_hash=max_hash, want=want)
                for name in want:
                    out[name][r:r + tile, c:c + tile] = blk[name]
                    if c > r:
                        out[mirror.get(name, name)][c:c + tile, r:r + tile] = blk[name].T
                out["n_a"][r:r + tile] = blk["n_a"]
                out["n_a"][c:c + tile] = blk["n_b"]
        return out

    def jaccard_matrix(self, num: int = None, max_hash: int = None) -> np.ndarray:
        m = self._square(("n_shared", "n_union"), num, max_hash)
        return _ratio(m["n_shared"], m["n_union"])

    def containment_matrix(self, num: int = None, max_hash: int = None) -> np.ndarray:
        """Entry (r, c): the share of sketch r's hashes that sketch c holds too."""
        m = self._square(("n_shared",), num, max_hash)
        return _ratio(m["n_shared"], m["n_a"][:, None])

    def cosine_matrix(self, num: int = None, max_hash: int = None) -> np.ndarray:
        m = self._square(("dot", "norm2_a", "norm2_b"), num, max_hash)
        return _ratio(m["dot"], np.sqrt(m["norm2_a"] * m["norm2_b"]))

    def mash_distance_matrix(self, k: int = None, num: int = None, max_hash: int = None) -> np.ndarray:
        k = self.k if k is None else k
        if not k:
            raise L.NtkError(2, "mash_distance_matrix(k): a set of bare arrays does not know its k")
        j = self.jaccard_matrix(num, max_hash)
        # KmerMinHash.mash_distance on every distinct Jaccard value: math.log, so that the two agree to the last bit
        u, inv = np.unique(j, return_inverse=True)
        d = np.array([1.0 if v == 0 else max(0.0, -math.log(2.0 * v / (1.0 + v)) / k) for v in u.tolist()], dtype=np.float64)
        return d[inv].reshape(j.shape)

    def search(self, query, top: int = 10, containment: bool = False):
        """One query (a KmerMinHash or a (hashes, counts) pair) against the whole set: [(index, score)] of the `top` best, best first;
        the score is the Jaccard similarity, or with containment=True the share of the query's hashes the sketch holds."""
        with MinHashSet(self.abundance, self.ctx) as q:
            if isinstance(query, KmerMinHash):
                self._admit(query)
            q.add(query)
            num = min(self.num or 0, q.num or 0) if isinstance(query, KmerMinHash) else (self.num or 0)
            max_hash = min(ALL if s.max_hash is None else s.max_hash for s in (self, q))
            m = q.compare(other=self, num=num, max_hash=max_hash, want=("n_shared", "n_union"))
        score = _ratio(m["n_shared"][0], m["n_a"][0] if containment else m["n_union"][0])
        order = np.argsort(-score, kind="stable")[:top]
        return [(int(i), float(score[i])) for i in order]
