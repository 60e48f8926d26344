"""The expected rows of the per-read abundance call (include/needletail_amd_abundance.h), from the oracle alone.

The table is `_count_helpers.oracle_items(table_batch, k, path, pre)`; the k-mers of record r are
`_count_helpers.oracle_values(record + b"\\n", k, path, pre)` (after `quality_masked` when a quality stream is used); each value is
looked up in the items (absent = 0), and the row is len, (c >= min_count).sum(), sort(c)[0], sort(c)[n // 2], sort(c)[-1],
sum mod 2^64.  min_count 0 counts as 1.  Nothing here calls the library under test."""
import numpy as np

from _count_helpers import oracle_values, quality_masked

COLUMNS = ("n_kmers", "n_present", "min", "median", "max", "sum")
M64 = (1 << 64) - 1


def row(counts, min_count=1) -> np.ndarray:
    """The row of one record from the table counts of its k-mers (any order)."""
    c = np.asarray(counts, dtype=np.uint64)
    n = int(c.size)
    if n == 0:
        return np.zeros(6, dtype=np.uint64)
    mc = np.uint64(max(int(min_count), 1))
    s = np.sort(c)
    total = int(c.sum(dtype=np.uint64))   # numpy's uint64 sum wraps mod 2^64 (tests/test_abundance_abi.py holds it to Python integers)
    return np.array([n, int((c >= mc).sum()), int(s[0]), int(s[n // 2]), int(s[-1]), total], dtype=np.uint64)


def weighted_row(counts, weights, min_count=1) -> np.ndarray:
    """row() of the multiset in which counts[i] occurs weights[i] times, without writing it out (a periodic record of any length)."""
    c, w = np.asarray(counts, dtype=np.uint64), np.asarray(weights, dtype=np.int64)
    c, w = c[w > 0], w[w > 0]
    n = int(w.sum())
    if n == 0:
        return np.zeros(6, dtype=np.uint64)
    mc = np.uint64(max(int(min_count), 1))
    order = np.argsort(c, kind="stable")
    cs, ws = c[order], w[order]
    median = int(cs[np.searchsorted(np.cumsum(ws), n // 2, side="right")])   # the first value whose cumulative weight exceeds n // 2
    total = sum(int(x) * int(y) for x, y in zip(c, w)) & M64
    return np.array([n, int(w[c >= mc].sum()), int(cs[0]), median, int(cs[-1]), total], dtype=np.uint64)


def lookup(values, items) -> np.ndarray:
    """Table counts of the values: items = (keys ascending, counts); absent = 0."""
    keys, counts = items
    values = np.asarray(values, dtype=np.uint64)
    if keys.size == 0:
        return np.zeros(values.size, dtype=np.uint64)
    at = np.minimum(np.searchsorted(keys, values), keys.size - 1)
    return np.where(keys[at] == values, counts[at].astype(np.uint64), np.uint64(0))


def record_values(record: bytes, k, path, pre, qual=None, cutoff=None):
    """The k-mers record r emits.  qual: its quality bytes (masked at `cutoff` first)."""
    buf = bytes(record) + b"\n"
    if qual is not None:
        q = np.append(np.asarray(qual, dtype=np.uint8), 0xFF)
        buf = quality_masked(buf, q) if cutoff is None else quality_masked(buf, q, cutoff)
    return oracle_values(buf, k, path, pre)


def rows(records, items, k, path, pre, min_count=1, quals=None, cutoff=None) -> np.ndarray:
    """The (n_records, 6) uint64 array of rows of `records` against the table `items`."""
    return rows_from_values([record_values(r, k, path, pre, None if quals is None else quals[i], cutoff) for i, r in enumerate(records)],
                            items, min_count)


def rows_from_values(values_per_record, items, min_count=1) -> np.ndarray:
    """rows() from the records' k-mers, for several min_count on one walk of the oracle."""
    out = np.zeros((len(values_per_record), 6), dtype=np.uint64)
    for i, v in enumerate(values_per_record):
        out[i] = row(lookup(v, items), min_count)
    return out


def offsets(records) -> np.ndarray:
    """The packer's offsets of records it copies unchanged: record r = [off[r], off[r + 1]), the last byte its break byte."""
    return np.concatenate([[0], np.cumsum([len(r) + 1 for r in records])]).astype(np.uint64)


def mean_text(row_) -> str:
    """sum / n_kmers with 3 decimals, halves rounded up, in integers; 0.000 for no k-mers."""
    n, s = int(row_[0]), int(row_[5])
    if n == 0:
        return "0.000"
    whole, milli = s // n, ((s % n) * 1000 + n // 2) // n
    if milli == 1000:
        whole, milli = whole + 1, 0
    return f"{whole}.{milli:03d}"


def cli_line(name: str, row_) -> str:
    return "\t".join([name] + [str(int(x)) for x in row_[:5]] + [mean_text(row_)])
