"""A host model of the minimizer-list library (include/needletail_amd/minimizer_list.h), written from the header's text: the keys are
the k-mers the oracle's iterators emit on the packed batch (tests/_count_helpers.oracle_values' way of laying the runs side by side, here
with their window ends and strand flags kept), a window is w consecutive emitted window ends, its minimizer the leftmost smallest key,
and consecutive windows with the same pick are one entry with a span.  numpy-vectorised; independent of needletail_amd/minimizer_lists.py;
nothing here calls the library under test."""
import numpy as np

import oracle as O  # the checker
from _count_helpers import _CODE, _window_values, quality_masked

PATH_BYTES_CANONICAL, PATH_BITS, PATH_BITS_CANONICAL = 0, 1, 2
PRE_NONE, PRE_STRIP_RETURNS, PRE_NORMALIZE, PRE_NORMALIZE_IUPAC = 0, 1, 2, 3
LEX, HASH = 0, 1
W_MAX = 256
XOR = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
HIST_BINS = 4096
CHUNK = 64 << 20          # bases materialised per pass (csrc/ntk_chunks.hpp kChunkBases)
TILE = 1024               # window ends a block of ml_select_kernel takes at a time (csrc/ntk_ml_rule.hpp ML_TILE)
BLOCKS_PER_CU = 8         # ML_BLOCKS_PER_CU: the grid cap of the two tile kernels
STATS = ("n_records", "n_entries", "n_windows", "n_chunks", "device_bytes", "k", "path", "w", "order")


def fmix64(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33); x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33); x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def keys_of(values, order):
    values = np.asarray(values, dtype=np.uint64)
    return fmix64(values ^ np.uint64(XOR)) if order == HASH else values


def planes(buf: bytes, k: int, path: int, pre: int, qual=None, cutoff: int = 0):
    """(values, valid, strand) per window END byte of a packed batch: what the materialise face emits.  qual: one quality byte per
    batch byte (a base below `cutoff` is an N first)."""
    if qual is not None and cutoff:
        buf = quality_masked(bytes(buf), np.asarray(qual, dtype=np.uint8), cutoff)
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    n = a.size
    values, valid, strand = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.uint8)
    if n < k:
        return values, valid, strand
    accept_u = pre >= PRE_NORMALIZE
    base = _CODE[a] != 255
    isu = (a == ord("U")) | (a == ord("u"))
    if accept_u:
        base |= isu
    runs = np.where(base, a, ord("N")).astype(np.uint8)
    if accept_u:
        runs[isu] = ord("T")
    if path != PATH_BYTES_CANONICAL:
        pos, val, flg = O.bit_kmers_arrays(runs.tobytes(), k, path == PATH_BITS_CANONICAL)
    else:
        norm = O.normalize(runs.tobytes())[0]
        assert len(norm) == n
        rc = O.reverse_complement(norm)
        pos, flg = O.canonical_kmers_arrays(norm, rc, k)
        p = pos.astype(np.int64)
        fw, rv = _CODE[np.frombuffer(norm, dtype=np.uint8)], _CODE[np.frombuffer(rc, dtype=np.uint8)]
        val = np.where(flg == 1, _window_values(rv, np.where(flg == 1, n - p - k, 0), k), _window_values(fw, np.where(flg == 1, 0, p), k))
    end = pos.astype(np.int64) + k - 1
    values[end], valid[end], strand[end] = val, True, flg
    return values, valid, strand


class Entries:
    """The entries of a batch in ascending order of first window end: end (the first window end), picked (the minimizer's window
    end), value, strand, span."""

    def __init__(self, end, picked, value, strand, span):
        self.end, self.picked = np.asarray(end, dtype=np.int64), np.asarray(picked, dtype=np.int64)
        self.value, self.strand = np.asarray(value, dtype=np.uint64), np.asarray(strand, dtype=np.uint8)
        self.span = np.asarray(span, dtype=np.uint32)

    def __len__(self):
        return self.end.size

    def shifted(self, by):
        return Entries(self.end + by, self.picked + by, self.value, self.strand, self.span)


def concat(parts):
    parts = list(parts)
    return Entries(*(np.concatenate([getattr(p, f) for p in parts]) if parts else [] for f in ("end", "picked", "value", "strand", "span")))


def windows(values, valid, w, order):
    """(whole, picked) per window end: the window of w ends is whole, and the end it picks (the leftmost smallest key)."""
    n = values.size
    key = keys_of(values, order)
    bad = np.concatenate([[0], np.cumsum(~valid)])
    e = np.arange(n, dtype=np.int64)
    first = e - (w - 1)
    whole = (first >= 0) & ((bad[e + 1] - bad[np.maximum(first, 0)]) == 0)
    at = np.maximum(first, 0)
    best, picked = key[at].copy(), at.copy()
    for j in range(w - 2, -1, -1):    # from the left: only a strictly smaller key replaces the pick
        at = np.maximum(e - j, 0)
        take = key[at] < best
        best[take], picked[take] = key[at][take], at[take]
    return whole, picked


def entries_of(buf: bytes, k: int, w: int, path: int, pre: int, order: int = LEX, qual=None, cutoff: int = 0) -> Entries:
    values, valid, strand = planes(buf, k, path, pre, qual, cutoff)
    n = values.size
    if n == 0:
        return Entries([], [], [], [], [])
    whole, picked = windows(values, valid, w, order)
    before_whole = np.concatenate([[False], whole[:-1]])
    before_pick = np.concatenate([[-1], picked[:-1]])
    opens = whole & ~(before_whole & (before_pick == picked))
    e = np.flatnonzero(opens)
    stop = np.flatnonzero(~(whole & ~opens))           # the ends that do not continue an entry
    stop = np.append(stop, n)
    span = stop[np.searchsorted(stop, e, side="right")] - e
    a = picked[e]
    return Entries(e, a, values[a], strand[a], span)


def starts(offsets, n_bytes):
    return np.minimum(np.asarray(offsets, dtype=np.uint64), np.uint64(n_bytes)).astype(np.int64)


def csr(entries: Entries, offsets, n_bytes: int, k: int):
    """(offsets_out, pos, values, strand, span) as MinimizerList.read() returns them."""
    s = starts(offsets, n_bytes)
    out = np.searchsorted(entries.end, s, side="left").astype(np.uint64)
    j = np.searchsorted(s, entries.end, side="right")            # record starts at or before the first window end
    rec_start = np.where(j > 0, s[np.maximum(j - 1, 0)], 0)
    pos = (entries.picked - (k - 1) - rec_start).astype(np.uint64)
    return out, pos, entries.value, entries.strand, entries.span


def lists(records, k, w, path, pre, order=LEX, quals=None, cutoff=0):
    """The CSR of records the packer copies unchanged."""
    buf = b"".join(bytes(r) + b"\n" for r in records)
    off = packed_offsets(records)
    qual = None
    if quals is not None:
        qual = np.frombuffer(b"".join(bytes(q) + b"\xff" for q in quals), dtype=np.uint8)
    return csr(entries_of(buf, k, w, path, pre, order, qual, cutoff), off, len(buf), k)


def packed_offsets(records) -> np.ndarray:
    """The packer's offsets of records it copies unchanged: record r = [off[r], off[r + 1]), the last byte its break byte."""
    return np.concatenate([[0], np.cumsum([len(r) + 1 for r in records])]).astype(np.uint64)


def hist_shift(k):
    return 2 * (k - min(k, 6))


def digest(values, strand, span, k):
    """What ntk_minimizers_reduce_device folds, from the entries: every window counts its minimizer once."""
    values, span = np.asarray(values, dtype=np.uint64), np.asarray(span, dtype=np.uint64)
    strand = np.asarray(strand)
    hist = np.zeros(HIST_BINS, dtype=np.uint64)
    np.add.at(hist, (values >> np.uint64(hist_shift(k))).astype(np.int64), span)
    with np.errstate(over="ignore"):
        total = int((span * values).sum(dtype=np.uint64)) if values.size else 0
    odd = values[(span & np.uint64(1)) == 1]
    n_total, n_fwd = int(span.sum()), int(span[strand == 0].sum())
    return {"n_total": n_total, "n_fwd": n_fwd, "n_rc": n_total - n_fwd, "sum": total & M64,
            "xor": int(np.bitwise_xor.reduce(odd)) if odd.size else 0, "hist": hist}


def same_digest(a, b):
    return all(a[key] == b[key] for key in ("n_total", "n_fwd", "n_rc", "sum", "xor")) and np.array_equal(a["hist"], b["hist"])


# ---- the header's memory statement --------------------------------------------------------------------------------------------------

def halo(k, w):
    return (k + w - 1 + 15) & ~15


def grow_half_again(need):
    return need + need // 2 + 64


def device_bytes(n_bytes, n_records, k, w, entries_per_chunk):
    """stats.device_bytes after ONE run on a fresh (or trimmed) handle: entries_per_chunk = the entries each chunk added, in order."""
    if n_bytes == 0 or n_records == 0:
        return grow_half_again(n_records + 1) * 8
    many = n_bytes > CHUNK
    bases = min(n_bytes, CHUNK) + (halo(k, w) + w - 1 if many else 0)
    bases16 = (bases + 15) & ~15
    tiles = (min(n_bytes, CHUNK) + w - 1 + TILE - 1) // TILE
    total = bases16 * 8 + 2 * (bases16 // 16) * 2        # the materialise scratch: 8.25 B per base
    total += bases16 * 2                                  # the window ends' words
    total += 2 * (tiles + 1) * 4                          # the tiles' counts and their scan
    total += 2 * 8                                        # the counter words
    total += grow_half_again(n_records + 1) * 8           # the record ranges
    cap = held = 0
    for fresh in entries_per_chunk:
        if fresh and held + fresh > cap:
            cap = grow_half_again(held + fresh)
        held += fresh
    return total + cap * (20 + 8)            # the held list and the first window ends
