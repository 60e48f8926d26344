"""The inputs of the seed-index tests (tests/test_gpu_seed_index.py), fabricated as lists - (offsets, pos, values, info) in numpy - or cut
from random sequences.  tests/test_seed_index_inputs.py shows on the CPU, with counts from the model, that they are not vacuous."""
import functools

import numpy as np

import _seed_index_model as M

U64, U32 = np.uint64, np.uint32
TOP = (1 << 64) - 1
# the values of the small case: A[c] occurs c times in the references; Z are in no reference (below, between and above the keys)
A = {1: 0x1111, 2: 0x2222_0000_0000, 3: 0x3333, 4: 0xF000_0000_0000_4444, 5: TOP - 5}
Z = (0, 0x2000, TOP)
GARBAGE = (1 << 32, 0x5A5A, 1)   # an entry outside every record: a pos the library would refuse if it looked at it


def make_list(records, front=0, back=0):
    """records: per record a list of (pos, value, strand) -> a list, with `front` / `back` entries outside every record."""
    flat = [e for r in records for e in r]
    pad = lambda n: [GARBAGE] * n   # noqa: E731
    entries = pad(front) + flat + pad(back)
    offsets = front + np.concatenate([[0], np.cumsum([len(r) for r in records])])
    # the span (bits 31:1 of info) is ignored: any will do
    return M.as_list(offsets, [e[0] for e in entries], [e[1] for e in entries], [e[2] | (i % 7 + 1) << 1 for i, e in enumerate(entries)])


def small_refs():
    """3 references of at most 12 entries: A[c] c times, strands mixed, A[2] on both strands of reference 0; fillers that occur once."""
    return [
        [(5, A[1], 0), (20, A[2], 0), (40, A[2], 1), (60, A[3], 1), (70, A[5], 0), (80, 0x7001, 0), (81, 0x7002, 1)],
        [(7, A[3], 0), (30, A[4], 0), (50, A[4], 1), (70, A[5], 0), (90, A[5], 1), (91, 0x7003, 0)],
        [(9, A[3], 0), (31, A[4], 0), (33, A[4], 1), (70, A[5], 0), (95, A[5], 1), (96, 0x7004, 1), (97, 0x7005, 0)],
    ]


def small_reads():
    """8 reads of at most 12 entries: one without seeds, one whose seeds are all absent, values twice in one read (equal ref_rev and
    rpos, two qpos), both strands, qpos not in list order, and a last read whose anchors come out of the fill unsorted."""
    return [
        [],
        [(1, Z[0], 0), (2, Z[1], 1), (3, Z[2], 0)],
        [(0, A[1], 0), (4, A[2], 0), (9, A[3], 1), (11, Z[1], 0)],
        [(3, A[1], 0), (9, A[1], 0), (12, A[5], 1), (15, A[5], 1), (20, Z[2], 0)],
        [(2, A[2], 1), (6, A[3], 0), (8, A[4], 1), (30, A[4], 0)],
        [(40, A[5], 0), (35, A[4], 0), (30, A[3], 0), (25, A[2], 0), (20, A[1], 0), (15, Z[0], 1), (10, A[1], 1), (5, A[2], 1), (4, A[3], 1),
         (3, A[4], 1), (2, A[5], 1), (1, 0x7003, 0)],
        [(17, A[4], 0)],
        [(1, 0x7005, 0), (2, A[3], 1), (3, A[2], 0), (4, A[1], 1)],
    ]


def small_case(front=0, back=0):
    return make_list(small_refs(), front, back), make_list(small_reads(), front, back)


def empty_list(n_records=0):
    return M.as_list(np.zeros(n_records + 1), [], [], [])


def refused_lists():
    """(what, list, status): each refusal of the on-device verification, on the small reads."""
    off, pos, values, info = make_list(small_reads())
    down = off.copy()
    down[3], down[4] = off[4], off[3]
    beyond = off.copy()
    beyond[-1] += 1
    far = pos.copy()
    far[5] = 1 << 32
    both = far.copy()
    return [("offsets decreasing", (down, pos, values, info), M.ERR_BAD_ARG), ("offsets[n] > n", (beyond, pos, values, info), M.ERR_BAD_ARG),
            ("a pos of 2^32", (off, far, values, info), M.ERR_UNSUPPORTED), ("both", (down, both, values, info), M.ERR_BAD_ARG)]


# ---- the two sort routes -------------------------------------------------------------------------------------------------------------------

V, W = 0xABCDEF, 0xABCDF0


def sort_route_case(n_anchors):
    """One read with exactly n_anchors anchors, short reads before and behind it.  The reference holds V on alternating strands (the
    fill's order, ascending rpos, is not the sorted one) and W once or twice; the read holds V twice, the later qpos first, so every
    (ref_rev, rpos) of V is there twice, and W."""
    w_occ = 1 if n_anchors % 2 else 2
    a = (n_anchors - w_occ) // 2
    ref0 = [(3 * i, V, i & 1) for i in range(a)] + [(3 * a + 5 * j, W, j) for j in range(w_occ)]
    refs = [[(4, 0x77, 0), (9, 0x78, 1)], ref0, [(1, 0x79, 0)]]
    short = [[(1, 0x77, 0), (2, 0x79, 0)], [], [(5, 0x78, 0)]]
    reads = short + [[(50, V, 0), (20, V, 0), (70, W, 1)]] + short[::-1]
    return make_list(refs), make_list(reads)


def balanced_fill_case(n_cu, occ=20_000):
    """One seed with `occ` occurrences among seeds with one: more reads in front of the long one than 2.25 steps of a grid of one block
    per read."""
    n_front = (9 * n_cu * M.BLOCKS_PER_CU) // 4 + 7
    ones = [(i, 0x100000 + i, i & 1) for i in range(n_front + 5)]
    refs = [[(2 * i, V, (i // 3) & 1) for i in range(occ)], ones]
    reads = [[(i % 50, 0x100000 + i, 0)] for i in range(n_front)]
    reads += [[(3, 0x100000, 1), (8, V, 0), (9, 0x100001, 0)]] + [[(1, 0x100000 + n_front + i, 1)] for i in range(5)]
    return make_list(refs), make_list(reads)


# ---- past one step of every capped grid ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def capped_grid_case(n_cu, quarters):
    """quarters / 4 steps of a grid of n_cu * BLOCKS_PER_CU blocks of THREADS, of entries and of seeds, with at most one occurrence per
    seed: distinct values in the references (in shuffled order), every seed present (so the anchors are as many steps) but one in 64,
    three seeds per read (so the reads are more steps of the kernels that take a wave or a block per read)."""
    n = n_cu * M.BLOCKS_PER_CU * M.THREADS * quarters // 4 + 3
    rng = np.random.default_rng(0x51 + quarters)
    values = rng.permutation(n).astype(U64) * U64(0x9E3779B97F4A7C15 | 1)   # distinct: an odd multiplier is a bijection
    n_refs = 1000
    r_off = np.concatenate([[0], np.sort(rng.integers(0, n + 1, n_refs - 1)), [n]]).astype(U64)
    refs = M.as_list(r_off, rng.integers(0, 1 << 32, n, dtype=U64), values, rng.integers(0, 1 << 32, n, dtype=U64).astype(U32))
    seeds = values[rng.permutation(n)]
    absent = rng.integers(0, 64, n) == 0
    seeds[absent] += U64(1)    # (may be a key again: the model decides)
    q_off = np.concatenate([np.arange(0, n, 3), [n]]).astype(U64)
    reads = M.as_list(q_off, rng.integers(0, 1 << 32, n, dtype=U64), seeds, rng.integers(0, 2, n, dtype=U64).astype(U32))
    return refs, reads


# ---- random lists --------------------------------------------------------------------------------------------------------------------------

RANDOM_SEEDS = (0x5E1, 0x5E2, 0x5E3)
RANDOM_MAX_OCC = 3


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """Random lists over a small universe of values: 5 references, 40 reads, occ up to about 8, then the shapes a random draw need not
    hold, appended: a key with RANDOM_MAX_OCC occurrences and one with one more, a read without seeds, a read of absent seeds, a read
    on both strands of one reference, and a value twice in one read."""
    rng = np.random.default_rng(seed)
    universe = rng.integers(0, 1 << 64, 60, dtype=U64)
    exact, over, twice = U64(0xE0E0), U64(0xE1E1), U64(0xE2E2)
    refs = [[(int(p), int(universe[rng.integers(0, 40)]), int(rng.integers(0, 2))) for p in np.sort(rng.integers(0, 5000, rng.integers(0, 60)))]
            for _ in range(5)]
    refs[0] += [(6000 + i, int(exact), 0) for i in range(RANDOM_MAX_OCC)] + [(7000, int(twice), 0), (7100, int(twice), 1)]
    refs[4] += [(6000 + i, int(over), i & 1) for i in range(RANDOM_MAX_OCC + 1)]
    reads = [[(int(p), int(universe[rng.integers(0, 60)]), int(rng.integers(0, 2))) for p in np.sort(rng.integers(0, 150, rng.integers(0, 25)))]
             for _ in range(40)]
    reads[7] = []
    reads[8] = [(1, int(universe[55]), 0), (9, int(universe[59]), 1)]
    reads[9] = [(4, int(exact), 0), (8, int(over), 1), (12, int(twice), 0), (16, int(twice), 0)]
    reads[39] = [(9, int(twice), 1), (2, int(twice), 0)]   # the last read: the fill's order is not the sorted one
    return make_list(refs), make_list(reads)


# ---- end to end through the minimizer lists ----------------------------------------------------------------------------------------------

END_TO_END = ((15, 10, 1, 2), (21, 11, 0, 0))   # k, w, order (1: HASH), path (2: bit-canonical, 0: bytes)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(seq: bytes) -> bytes:
    return seq.translate(_COMP)[::-1]


@functools.lru_cache(maxsize=None)
def sequences(seed=0x5EED51, n_refs=3, ref_len=2000, n_reads=60, read_len=150):
    """(references, reads, cuts): cuts[q] = (reference, start, reverse) of a read cut from a reference, None of a random one."""
    rng = np.random.default_rng(seed)
    rand = lambda n: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])   # noqa: E731
    refs = [rand(ref_len) for _ in range(n_refs)]
    reads, cuts = [], []
    for q in range(n_reads):
        if q % 6 == 5:
            reads.append(rand(read_len)); cuts.append(None)
            continue
        r, s, reverse = int(rng.integers(0, n_refs)), int(rng.integers(0, ref_len - read_len + 1)), bool(q & 1)
        piece = refs[r][s: s + read_len]
        reads.append(revcomp(piece) if reverse else piece); cuts.append((r, s, reverse))
    return refs, reads, cuts


def as_seed_list(csr):
    """A MinimizerList.read() / model CSR (offsets, pos, values, strand, span) as a list."""
    offsets, pos, values, strand, span = csr
    return M.as_list(offsets, pos, values, np.asarray(strand, dtype=U32) | np.asarray(span, dtype=U32) << U32(1))


def diagonal_exceptions(result, cuts, k, read_len=150):
    """The anchors of cut reads on their own reference that are off the diagonal of the cut or on the wrong strand, and the number
    that are on it."""
    a_offsets, ref, rev, rpos, qpos, _ = result
    off, on = [], 0
    for q, cut in enumerate(cuts):
        if cut is None:
            continue
        r, s, reverse = cut
        for i in range(int(a_offsets[q]), int(a_offsets[q + 1])):
            if int(ref[i]) != r:
                continue
            good = (int(rev[i]) == 1 and int(rpos[i]) + int(qpos[i]) == s + read_len - k) if reverse else \
                   (int(rev[i]) == 0 and int(rpos[i]) - int(qpos[i]) == s)
            on += good
            if not good:
                off.append((q, i))
    return off, on
