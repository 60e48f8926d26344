"""The expected answers of the coloured k-mer index and its read screen (include/needletail_amd_colors.h), by definition.

The index is a Python dict built by OR: key -> mask, bits at or above n_colors cleared first, a key whose mask is then 0 left out.
The k-mers of record r are `_count_helpers.oracle_values(record + b"\\n", k, path, pre)` (after `quality_masked` when a quality stream
is used), as tests/_abundance_model.py takes them.  hits[c] counts the record's k-mers whose mask has bit c, single[c] those whose
mask is exactly 1 << c; the row is n_kmers, n_hit (mask != 0), n_single (one bit), best, second.  best = the colour with the most
hits, ties to the smallest colour, NONE without a hit; second = the same over the other colours.  Nothing here calls the library under
test."""
import numpy as np

from _abundance_model import offsets, record_values  # noqa: F401  (the tests take both from here)

COLUMNS = ("n_kmers", "n_hit", "n_single", "best", "second")
STATS = ("n_keys", "n_dropped", "n_masked_bits", "slots", "device_bytes", "n_launches", "per_color", "n_colors", "k", "path", "reserved")
M64 = (1 << 64) - 1
NONE = M64
COLORS_MAX = 64
LONG_RECORD = 16384   # ntk_colors.hip kLongRecord (tests/test_colors_abi.py ties them)


def color_bits(n_colors: int) -> int:
    return (1 << n_colors) - 1


class Index:
    """key -> mask (the dict `masks`), with the statistics the library reports that do not depend on its slots."""

    def __init__(self, n_colors: int):
        assert 1 <= n_colors <= COLORS_MAX
        self.n_colors, self.masks, self.n_masked_bits = n_colors, {}, 0
        self._sorted = None

    def add(self, keys, masks):
        """masks: one per key, or one int for all."""
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
        masks = np.full(keys.size, int(masks), dtype=np.uint64) if np.ndim(masks) == 0 else np.asarray(masks, dtype=np.uint64).reshape(-1)
        assert keys.size == masks.size
        bits = np.uint64(color_bits(self.n_colors))
        beyond, times = np.unique(masks & ~bits, return_counts=True)
        self.n_masked_bits += sum(bin(int(m)).count("1") * int(t) for m, t in zip(beyond, times))
        masks = masks & bits
        for key, m in zip(keys[masks != 0].tolist(), masks[masks != 0].tolist()):
            self.masks[key] = self.masks.get(key, 0) | m
        self._sorted = None

    def lookup(self, values) -> np.ndarray:
        values = np.asarray(values, dtype=np.uint64).reshape(-1)
        if not self.masks or values.size == 0:
            return np.zeros(values.size, dtype=np.uint64)
        if self._sorted is None:
            keys = np.fromiter(self.masks.keys(), dtype=np.uint64, count=len(self.masks))
            order = np.argsort(keys)
            self._sorted = keys[order], np.fromiter(self.masks.values(), dtype=np.uint64, count=len(self.masks))[order]
        keys, masks = self._sorted
        at = np.minimum(np.searchsorted(keys, values), keys.size - 1)
        return np.where(keys[at] == values, masks[at], np.uint64(0))

    @property
    def n_keys(self) -> int:
        return len(self.masks)

    def per_color(self):
        return [sum(m >> c & 1 for m in self.masks.values()) for c in range(self.n_colors)]


def device_bytes(slots: int, longest_batch: int, k: int) -> int:
    """The header's memory statement: what stats.device_bytes reads after run_device calls whose longest batch had `longest_batch` bytes
    (0: none yet, or released)."""
    from _count_model import CHUNK
    total = 16 * slots + 68 * 8
    if longest_batch:
        halo = (k - 1 + 15) // 16 * 16 if longest_batch > CHUNK else 0
        bases = (min(longest_batch, CHUNK) + halo + 15) // 16 * 16
        total += bases * 8 + 2 * (bases // 16) * 2 + (longest_batch // LONG_RECORD + 2) * 8
    return total


def best_second(hits):
    """(best, second) of one row of the matrix."""
    order = sorted((c for c, h in enumerate(hits) if int(h) > 0), key=lambda c: (-int(hits[c]), c))
    return (order[0] if order else NONE), (order[1] if len(order) > 1 else NONE)


def screen_masks(masks, n_colors: int):
    """(row, hits, single) of one record from the masks of its k-mers."""
    m = np.asarray(masks, dtype=np.uint64).reshape(-1)
    colours = np.arange(n_colors, dtype=np.uint64)
    hits = ((m[:, None] >> colours[None, :]) & np.uint64(1)).sum(axis=0, dtype=np.uint64)
    single = (m[:, None] == (np.uint64(1) << colours)[None, :]).sum(axis=0, dtype=np.uint64)
    b, s = best_second(hits)
    return np.array([m.size, int((m != 0).sum()), int(single.sum()), b, s], dtype=np.uint64), hits, single


def screen_values(values_per_record, index: Index):
    """(rows (n, 5), hits (n, C), single (n, C)) uint64 from the records' k-mers."""
    n, c = len(values_per_record), index.n_colors
    rows, hits, single = np.zeros((n, 5), dtype=np.uint64), np.zeros((n, c), dtype=np.uint64), np.zeros((n, c), dtype=np.uint64)
    for i, v in enumerate(values_per_record):
        rows[i], hits[i], single[i] = screen_masks(index.lookup(v), c)
    return rows, hits, single


def screen(records, index: Index, k, path, pre, quals=None, cutoff=None):
    return screen_values([record_values(r, k, path, pre, None if quals is None else quals[i], cutoff) for i, r in enumerate(records)], index)


def classify(rows, hits, min_hits=1, num=0, den=1) -> np.ndarray:
    """best where hits[best] >= min_hits and hits[best] * den >= num * n_kmers, else -1."""
    out = np.full(len(rows), -1, dtype=np.int64)
    for r in range(len(rows)):
        b = int(rows[r][3])
        if b != NONE and int(hits[r][b]) >= min_hits and int(hits[r][b]) * den >= num * int(rows[r][0]):
            out[r] = b
    return out


def colour_text(c) -> str:
    return "-" if int(c) == NONE else str(int(c))


def cli_line(name: str, row, hits) -> str:
    return "\t".join([name] + [str(int(x)) for x in row[:3]] + [colour_text(row[3]), colour_text(row[4])] + [str(int(h)) for h in hits])


def cli_summary(rows, hits, min_hits=1) -> str:
    n_colors = hits.shape[1]
    per, unassigned, ambiguous = [0] * n_colors, 0, 0
    for row, h in zip(rows, hits):
        b, s = int(row[3]), int(row[4])
        if b == NONE or int(h[b]) < min_hits:
            unassigned += 1
            continue
        per[b] += 1
        ambiguous += s != NONE and int(h[s]) == int(h[b])
    return "".join(f"#best\t{c}\t{n}\n" for c, n in enumerate(per)) + f"#unassigned\t{unassigned}\n#ambiguous\t{ambiguous}\n"
