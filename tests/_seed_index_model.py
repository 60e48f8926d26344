"""The host model of the seed-index library (include_staged/needletail_amd/seed_index.h): the rule in numpy, and the device memory the
header states.  A list is (offsets, pos, values, info) as numpy arrays, the shape MinimizerList hands out on the device.

tests/test_seed_index_model.py holds it to a brute-force restatement of the definition; the GPU tests hold the library to it.  The
`mutant` arguments restate four wrong libraries (tests/test_seed_index_inputs.py shows that the GPU cases tell each of them from the
right one)."""
import numpy as np

OK, ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 0, 2, 5, 6
SORT_TILE = 2048          # SI_SORT_TILE of csrc/ntk_si_rule.hpp
BLOCKS_PER_CU = 8         # SI_BLOCKS_PER_CU
THREADS = 256             # SI_THREADS
STATS = ("n_refs", "n_entries", "n_keys", "max_occ", "n_reads", "n_seeds", "n_anchors", "device_bytes")
FIELDS = ("a_offsets", "ref", "rev", "rpos", "qpos", "rows")
MUTANTS = ("rightmost", "max_occ_ge", "unstable_tie", "last_read")
U64, U32 = np.uint64, np.uint32


def as_list(offsets, pos, values, info):
    return (np.asarray(offsets, dtype=U64), np.asarray(pos, dtype=U64), np.asarray(values, dtype=U64), np.asarray(info, dtype=U32))


def verify(lst):
    """The status of the list's verification: what build_device and match_device refuse."""
    off, pos, values, info = lst
    n, n_records = pos.size, off.size - 1
    if n >= 1 << 32 or n_records >= 1 << 31:
        return ERR_BAD_ARG
    if np.any(off[1:] < off[:-1]) or int(off[-1]) > n:
        return ERR_BAD_ARG
    if np.any(pos[int(off[0]): int(off[-1])] >> U64(32)):
        return ERR_UNSUPPORTED
    return OK


def _owners(off, lo, hi):
    """The record of every entry [lo, hi): the last one that starts at or before it."""
    return (np.searchsorted(off, np.arange(lo, hi, dtype=U64), side="right") - 1).astype(np.int64)


class Index:
    """keys ascending, start[key] .. start[key + 1] its occurrences, ref = r << 1 | strand and rpos per occurrence."""

    def __init__(self, lst):
        assert verify(lst) == OK
        off, pos, values, info = lst
        lo, hi = int(off[0]), int(off[-1])
        order = np.argsort(values[lo:hi], kind="stable")   # entry order already is (record, pos) order
        self.keys, first, self.occ = np.unique(values[lo:hi][order], return_index=True, return_counts=True)
        self.start = np.concatenate([first, [hi - lo]]).astype(np.int64)
        self.ref = ((_owners(off, lo, hi)[order] << 1) | (info[lo:hi][order] & 1).astype(np.int64)).astype(U32)
        self.rpos = pos[lo:hi][order].astype(U32)
        self.n_refs, self.n_entries, self.n_keys = off.size - 1, hi - lo, self.keys.size
        self.max_occ = int(self.occ.max()) if self.n_keys else 0

    def spectrum(self, n_bins):
        hist = np.zeros(n_bins, dtype=U64)
        np.add.at(hist, np.minimum(self.occ, n_bins - 1), 1)
        return hist

    def occ_cutoff(self, fraction_ppm):
        """The smallest c >= 1 such that at most fraction_ppm / 10^6 of the keys occur more than c times (1 for an empty index)."""
        c = 1
        while self.n_keys and int((self.occ > c).sum()) * 1_000_000 > fraction_ppm * self.n_keys:
            c += 1
        return c


def classify(index, values, max_occ, mutant=None):
    """Per seed: its key index (-1: ABSENT), its occ, and whether it is a HIT."""
    side = "right" if mutant == "rightmost" else "left"
    at = np.searchsorted(index.keys, values, side=side).astype(np.int64)
    present = at < index.n_keys
    present[present] = index.keys[at[present]] == values[present]
    occ = np.where(present, index.occ[np.minimum(at, max(index.n_keys - 1, 0))] if index.n_keys else 0, 0).astype(np.int64)
    repetitive = present & (max_occ != 0) & ((occ >= max_occ) if mutant == "max_occ_ge" else (occ > max_occ))
    return np.where(present, at, -1), occ, present & ~repetitive


def match(index, lst, max_occ=0, max_anchors=0, mutant=None):
    """(status, (a_offsets, ref, rev, rpos, qpos, rows), n_anchors): after NTK_ERR_CAPACITY the rows and n_anchors are valid, no
    anchor is held and every range is empty."""
    assert verify(lst) == OK
    off, pos, values, info = lst
    lo, hi, n_reads = int(off[0]), int(off[-1]), off.size - 1
    at, occ, hit = classify(index, values[lo:hi], max_occ, mutant)
    read_of_seed = _owners(off, lo, hi)
    rows = np.zeros((n_reads, 4), dtype=U32)
    for col, mask in ((0, np.ones(hi - lo, dtype=bool)), (1, hit), (2, (at >= 0) & ~hit), (3, at < 0)):
        rows[:, col] = np.bincount(read_of_seed[mask], minlength=n_reads)[:n_reads] if n_reads else 0
    count = np.where(hit, occ, 0)
    base = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    total = int(base[-1])
    empty = (np.zeros(n_reads + 1, dtype=U64), np.zeros(0, U32), np.zeros(0, np.uint8), np.zeros(0, U32), np.zeros(0, U32), rows)
    if (max_anchors and total > max_anchors) or total >= 1 << 32:
        return ERR_CAPACITY, empty, total
    seed = np.repeat(np.arange(hi - lo, dtype=np.int64), count)
    o = index.start[at[seed]] + (np.arange(total, dtype=np.int64) - base[seed])
    ref_rev = index.ref[o].astype(np.int64) ^ (info[lo:hi][seed] & 1).astype(np.int64)
    rpos, qpos, read = index.rpos[o].astype(np.int64), pos[lo:hi][seed].astype(np.int64), read_of_seed[seed]
    a_offsets = base[np.asarray(off, dtype=np.int64) - lo].astype(U64)
    if mutant == "unstable_tie":   # equal (ref_rev, rpos) in descending order of qpos
        order = np.lexsort((-qpos, rpos, ref_rev, read))
    else:
        order = np.lexsort((qpos, rpos, ref_rev, read))
    if mutant == "last_read" and n_reads:   # the last read is left as the fill made it
        keep = int(a_offsets[n_reads - 1])
        order = np.concatenate([order[:keep], np.arange(keep, total)])
    ref_rev, rpos, qpos = ref_rev[order], rpos[order], qpos[order]
    return OK, (a_offsets, (ref_rev >> 1).astype(U32), (ref_rev & 1).astype(np.uint8), rpos.astype(U32), qpos.astype(U32), rows), total


def stats(index, lst=None, n_anchors=0):
    """The stats without device_bytes: of the index, and of a match of `lst` that makes n_anchors."""
    out = {"n_refs": index.n_refs, "n_entries": index.n_entries, "n_keys": index.n_keys, "max_occ": index.max_occ,
           "n_reads": 0, "n_seeds": 0, "n_anchors": 0}
    if lst is not None:
        out.update(n_reads=lst[0].size - 1, n_seeds=int(lst[0][-1]) - int(lst[0][0]), n_anchors=n_anchors)
    return out


def half_again(n):
    return n + n // 2 + 64 if n else 0


def index_bytes(n_keys, n_entries):
    """The header's index: 12 B per key and 4 more, 8 B per occurrence."""
    return 12 * n_keys + 4 + 8 * n_entries


def device_bytes(n_keys, n_entries, n_reads=None, n_seeds=0, n_anchors=0, long_anchors=0, n_bins=0, build_work=True):
    """stats.device_bytes of a handle whose arrays were grown by one build of n_entries (build_work: since the last trim), at most one
    match of n_reads reads and one spectrum of n_bins, term by term as the header states them: the index; 4 counter words; the build's
    work, 28 B per entry; the match's work, 16 B per seed and 12 more and 16 B per read; the result, 12 B per anchor grown by half
    again and 64 and 8 + 16 B per read and 8 more; 24 B per anchor of the reads with more than SORT_TILE; the bins.  rocPRIM's
    temporary storage is held inside a call only: no term."""
    total = index_bytes(n_keys, n_entries) + 4 * 8 + (28 * n_entries if build_work else 0) + 8 * n_bins
    if n_reads is not None:
        total += 16 * n_seeds + 12 + 16 * n_reads + 12 * half_again(n_anchors) + 24 * n_reads + 8 + 24 * long_anchors
    return total


def long_anchors(a_offsets):
    """The anchors of the reads that have more than SORT_TILE of them."""
    n = np.diff(np.asarray(a_offsets, dtype=np.int64))
    return int(n[n > SORT_TILE].sum())
