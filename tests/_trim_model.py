"""The expected rows and output batch of the read trimmer (include/needletail_amd_trim.h), from the oracle alone.

A record's windows come from the oracle's literal iterators with their POSITIONS (`O.canonical_kmers_arrays` / `O.bit_kmers_arrays`):
`record_windows` returns the end position and the value of every k-mer the record emits.  The window ending at record position j
(k - 1 <= j < L) is solid when it was emitted and its value's count in the table items (`_abundance_model.lookup`, absent = 0) is
>= min_count (0 counts as 1); every other window is weak.  `interval` is the header's rule in plain Python, written in the record
positions j the header uses.  Nothing here calls the library under test."""
import numpy as np

import oracle as O  # the checker
from _abundance_model import lookup, offsets  # noqa: F401  (offsets: re-exported for the tests)
from _count_helpers import _CODE, _window_values, quality_masked

COLUMNS = ("start", "length", "n_kmers", "n_solid")
PREFIX, LONGEST = 0, 1
PATH_BYTES_CANONICAL, PATH_BITS, PATH_BITS_CANONICAL = 0, 1, 2
PRE_NORMALIZE = 2


def windows_of(buf: bytes, k: int, path: int, pre: int):
    """(end positions, values) of every k-mer a packed buffer emits: `_count_helpers.oracle_values` with the iterators' positions
    kept.  Each maximal run of base bytes of the mode is a sequence of its own; the runs are laid side by side with an N where the
    other bytes were, so one iterator call covers them all and a position in it is a position in the buffer."""
    a = np.frombuffer(buf, dtype=np.uint8)
    accept_u = pre >= PRE_NORMALIZE
    base = _CODE[a] != 255
    isu = (a == ord("U")) | (a == ord("u"))
    if accept_u:
        base |= isu
    runs = np.where(base, a, ord("N")).astype(np.uint8)
    if accept_u:
        runs[isu] = ord("T")
    if path != PATH_BYTES_CANONICAL:
        pos, val, _ = O.bit_kmers_arrays(runs.tobytes(), k, path == PATH_BITS_CANONICAL)
        return pos.astype(np.int64) + (k - 1), val
    norm = O.normalize(runs.tobytes())[0]
    n = len(norm)
    rc = O.reverse_complement(norm)
    pos, flg = O.canonical_kmers_arrays(norm, rc, k)
    pos = pos.astype(np.int64)
    fw, rv = _CODE[np.frombuffer(norm, dtype=np.uint8)], _CODE[np.frombuffer(rc, dtype=np.uint8)]
    val = np.where(flg == 1, _window_values(rv, np.where(flg == 1, n - pos - k, 0), k), _window_values(fw, np.where(flg == 1, 0, pos), k))
    return pos + (k - 1), val


def record_windows(record: bytes, k, path, pre, qual=None, cutoff=None):
    """(end positions in the record, values) of the k-mers record r emits.  qual: its quality bytes (masked at `cutoff` first)."""
    buf = bytes(record) + b"\n"
    if qual is not None:
        q = np.append(np.asarray(qual, dtype=np.uint8), 0xFF)
        buf = quality_masked(buf, q) if cutoff is None else quality_masked(buf, q, cutoff)
    return windows_of(buf, k, path, pre)


def solid_windows(L: int, k: int, ends, counts, min_count) -> np.ndarray:
    """solid[i] for the window that ends at record position k - 1 + i, i = 0 .. L - k (empty when L < k)."""
    solid = np.zeros(max(L - k + 1, 0), dtype=bool)
    mc = max(int(min_count), 1)
    ends, counts = np.asarray(ends, dtype=np.int64), np.asarray(counts, dtype=np.uint64)
    solid[ends[counts >= np.uint64(mc)] - (k - 1)] = True
    return solid


def runs(bits):
    """(length, leading ones, trailing ones, longest run of ones, position of its first bit: the leftmost of equals; 0, 0 for none)."""
    bits = [bool(x) for x in bits]
    n = len(bits)
    lead = next((i for i, b in enumerate(bits) if not b), n)
    trail = next((i for i, b in enumerate(reversed(bits)) if not b), n)
    best, pos, i = 0, 0, 0
    while i < n:
        if not bits[i]:
            i += 1
            continue
        e = i
        while e < n and bits[e]:
            e += 1
        if e - i > best:
            best, pos = e - i, i
        i = e
    return n, lead, trail, best, pos


def interval(solid, k: int, mode: int, min_length: int = 0):
    """(start, length) of the kept interval; (0, 0) when nothing is kept."""
    solid = [bool(x) for x in solid]
    L = len(solid) + k - 1 if solid else 0   # only used when there is a window
    if mode == PREFIX:
        j_star = L
        for i, s in enumerate(solid):
            if not s:
                j_star = k - 1 + i
                break
        kept = (0, j_star) if solid and j_star > k - 1 else None
    elif mode == LONGEST:
        kept, best, i = None, 0, 0
        while i < len(solid):
            if not solid[i]:
                i += 1
                continue
            e = i
            while e + 1 < len(solid) and solid[e + 1]:
                e += 1
            if e - i + 1 > best:   # strictly longer: the leftmost run wins a tie
                best = e - i + 1
                j0, j1 = k - 1 + i, k - 1 + e
                kept = (j0 - k + 1, j1 + 1)
            i = e + 1
    else:
        raise ValueError(mode)
    if kept is None or kept[1] - kept[0] < (min_length if min_length else k):
        return 0, 0
    return kept[0], kept[1] - kept[0]


def row(L, k, ends, counts, mode, min_count=1, min_length=0) -> np.ndarray:
    solid = solid_windows(L, k, ends, counts, min_count)
    start, length = interval(solid, k, mode, min_length)
    return np.array([start, length, len(ends), int(solid.sum())], dtype=np.uint64)


def rows_from_windows(records, windows, items, k, mode, min_count=1, min_length=0) -> np.ndarray:
    """The (n_records, 4) uint64 rows from the records' windows (record_windows), for several settings on one walk of the oracle."""
    out = np.zeros((len(records), 4), dtype=np.uint64)
    for i, (r, (ends, vals)) in enumerate(zip(records, windows)):
        out[i] = row(len(r), k, ends, lookup(vals, items), mode, min_count, min_length)
    return out


def rows(records, items, k, path, pre, mode, min_count=1, min_length=0, quals=None, cutoff=None) -> np.ndarray:
    wins = [record_windows(r, k, path, pre, None if quals is None else quals[i], cutoff) for i, r in enumerate(records)]
    return rows_from_windows(records, wins, items, k, mode, min_count, min_length)


def clamp(L, start, length):
    """A row that reaches beyond the record: start to L, then length to L - start."""
    start = min(int(start), L)
    return start, min(int(length), L - start)


def compact(records, rows_, auxs=None, aux_breaks=None):
    """The output batch of the records under the rows: (seq bytes padded with break bytes to a multiple of 16, n_bytes, offsets,
    sources[, aux bytes padded alike]).  aux_breaks[i]: the byte under record i's break byte in the aux stream."""
    seq, aux, offs, src = bytearray(), bytearray(), [0], []
    for i, r in enumerate(records):
        s, n = clamp(len(r), rows_[i][0], rows_[i][1])
        if n == 0:
            continue
        seq += r[s:s + n] + b"\n"
        if auxs is not None:
            aux += bytes(auxs[i][s:s + n]) + bytes([aux_breaks[i]])
        offs.append(len(seq))
        src.append(i)
    n_bytes = len(seq)
    pad = b"\n" * (-n_bytes % 16)
    out = (bytes(seq) + pad, n_bytes, np.array(offs, dtype=np.uint64), np.array(src, dtype=np.uint64))
    return out if auxs is None else out + (bytes(aux) + pad,)


def cli_text(names, records, rows_, quals=None) -> str:
    """What trim_reads prints: the kept records in input order, FASTQ with qualities and FASTA without."""
    out = []
    for i, (name, r) in enumerate(zip(names, records)):
        s, n = int(rows_[i][0]), int(rows_[i][1])
        if n == 0:
            continue
        if quals is None:
            out.append(f">{name}\n{r[s:s + n].decode()}\n")
        else:
            out.append(f"@{name}\n{r[s:s + n].decode()}\n+\n{bytes(quals[i][s:s + n]).decode()}\n")
    return "".join(out)
