"""The model of the exact k-mer set algebra (include/needletail_amd_kmer_sets.h): plain dicts and numpy, no tiles, no merge.

A list is (keys, counts): keys a uint64 array of shape (n,) for narrow keys or (n, 2) for wide ones ({hi, lo} rows), counts uint64 of
shape (n,).  A key of the model is a Python int: the value, or hi << 64 | lo."""
import numpy as np

M64 = (1 << 64) - 1
INTERSECT, UNION, SUBTRACT, COUNTERS_SUBTRACT = 1, 2, 3, 4          # NTK_KSET_*
MIN, MAX, SUM, LEFT, RIGHT = 1, 2, 3, 4, 5
OPS = tuple((op, rule) for op in (INTERSECT, UNION) for rule in (MIN, MAX, SUM, LEFT, RIGHT)) + ((SUBTRACT, 0), (COUNTERS_SUBTRACT, 0))
TILE_WORDS = 2048                                                    # NTK_KSET_TILE_WORDS: a tile is 2048 narrow or 1024 wide keys
MAX_BINS = 16384                                                     # NTK_KSET_MAX_BINS
TOTALS = ("n_a", "n_b", "n_shared", "n_a_only", "n_b_only", "sum_a", "sum_b", "sum_a_shared", "sum_b_shared", "sum_a_only", "sum_b_only",
          "sum_min", "sum_max")


def as_dict(keys, counts) -> dict:
    keys, counts = np.asarray(keys, dtype=np.uint64), np.asarray(counts, dtype=np.uint64)
    if keys.ndim == 2:
        ints = [(int(hi) << 64) | int(lo) for hi, lo in keys.tolist()]
    else:
        ints = [int(v) for v in keys.tolist()]
    d = dict(zip(ints, (int(c) for c in counts.tolist())))
    assert len(d) == len(ints), "a list holds every key once"
    return d


def as_list(d: dict, key_words: int):
    """The dict as a list: keys ascending, in the layout of the given key width."""
    ks = sorted(d)
    counts = np.array([d[k] for k in ks], dtype=np.uint64)
    if key_words == 2:
        keys = np.array([[k >> 64, k & M64] for k in ks], dtype=np.uint64).reshape(-1, 2)
    else:
        keys = np.array(ks, dtype=np.uint64)
    return keys, counts


def rule_of(rule: int, a: int, b: int) -> int:
    return {MIN: min(a, b), MAX: max(a, b), SUM: min(a + b, M64), LEFT: a, RIGHT: b}[rule]


def apply(op: int, rule: int, a: dict, b: dict) -> dict:
    if op == INTERSECT:
        return {k: rule_of(rule, a[k], b[k]) for k in a if k in b}
    if op == UNION:
        return {k: rule_of(rule, a[k], b[k]) if k in a and k in b else a.get(k, b.get(k)) for k in set(a) | set(b)}
    if op == SUBTRACT:
        return {k: c for k, c in a.items() if k not in b}
    assert op == COUNTERS_SUBTRACT
    return {k: c - b.get(k, 0) for k, c in a.items() if c > b.get(k, 0)}


def compare(a: dict, b: dict, bins_a: int, bins_b: int):
    """(hist of bins_a * bins_b uint64 values, totals as a dict of Python ints modulo 2^64)."""
    bins = []
    t = dict.fromkeys(TOTALS, 0)
    t["n_a"], t["n_b"] = len(a), len(b)
    for k in set(a) | set(b):
        ca, cb = a.get(k, 0), b.get(k, 0)
        bins.append(min(ca, bins_a - 1) * bins_b + min(cb, bins_b - 1))
        t["sum_a"] += ca
        t["sum_b"] += cb
        t["sum_max"] += max(ca, cb)
        if k in a and k in b:
            t["n_shared"] += 1
            t["sum_a_shared"] += ca
            t["sum_b_shared"] += cb
            t["sum_min"] += min(ca, cb)
        elif k in a:
            t["n_a_only"] += 1
            t["sum_a_only"] += ca
        else:
            t["n_b_only"] += 1
            t["sum_b_only"] += cb
    hist = np.bincount(np.array(bins, dtype=np.int64), minlength=bins_a * bins_b).astype(np.uint64)
    return hist, {name: v & M64 for name, v in t.items()}


def qv(sum_b_only: int, sum_b: int, k: int) -> float:
    """Merqury's consensus quality from the assembly's k-mer instances that the reads lack."""
    import math
    if sum_b_only == 0:
        return math.inf
    p = (1.0 - sum_b_only / sum_b) ** (1.0 / k)
    return -10.0 * math.log10(1.0 - p)
