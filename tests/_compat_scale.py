"""Inputs of tests/test_gpu_compat_scale.py: the Sequence-trait entry points at the sizes where their kernels take a second level.

Every builder is deterministic and knows nothing about the library: the thresholds it aims at are restated here as plain numbers, and
tests/test_compat_scale_inputs.py holds them to the constants in the source text and every input to its threshold (no GPU needed), so
that a changed constant fails there instead of silently un-covering a branch.  Test infrastructure, like oracle/ and tests/_refs.py."""
import numpy as np

MI = 1 << 20

# ---- what the kernels split on (tests/test_compat_scale_inputs.py reads the same numbers out of the source) ----------------------------
COMPACT_BLOCK_BYTES = 4096            # kCompactThreads * kCompactPerThread: one block of compact_count / compact_write
SCAN_THREADS = 1024                   # compact_scan_kernel and cp_scan_kernel are one block of 1024 threads
CP_BLOCK_POSITIONS = 16384            # kCpThreads * kCpWords * 16: one block of cp_count / cp_scatter
PL_TILE = 2048                        # kPlThreads * kPlPer: one tile of the planes kernels; the grid is n_cu * PL_BLOCKS_PER_CU blocks
PL_BLOCKS_PER_CU = 8
GRID_CAP_ITEMS = (1 << 20) * 256      # grid_for: at most 2^20 blocks of 256 threads; beyond that a thread takes a second item
LONG_RECORD = 1 << 16                 # kLongRecord (ntk_compat_plan.hpp): ntk_minimizer_batch hands longer records to the one-block kernel
DEFAULT_CHUNK_BYTES = 16 * MI         # kCompatChunkBytes: ntk_ctx::compat_chunk by default
MIN_CHUNK_BYTES = 64                  # kCompatChunkMin: the least NTK_OPT_COMPAT_CHUNK_BYTES is set to
BANKS = 3                             # kCompatBanks: the chunks the batched calls keep in flight


def first_difference(got, want):
    """Index of the first differing element of two byte strings / arrays (the shorter length if one is a prefix of the other), or None."""
    a = np.frombuffer(got, dtype=np.uint8) if isinstance(got, (bytes, bytearray)) else np.asarray(got)
    b = np.frombuffer(want, dtype=np.uint8) if isinstance(want, (bytes, bytearray)) else np.asarray(want)
    n = min(len(a), len(b))
    ne = np.flatnonzero(a[:n] != b[:n])
    if len(ne):
        return int(ne[0])
    return None if len(a) == len(b) else n


def assert_same(got, want, what, unit=1, unit_name="block"):
    """got == want element for element; a failure names the first differing index and the block / tile (index // unit) it lies in."""
    same = got == want if isinstance(got, (bytes, bytearray)) else (got.dtype == want.dtype and np.array_equal(got, want))
    if not same:
        i = first_difference(got, want)
        raise AssertionError(f"{what}: lengths {len(got)} / {len(want)}, first difference at index {i}"
                             + (f" ({unit_name} {i // unit})" if i is not None and unit > 1 else ""))


# ---- (a) normalize / strip_returns: the block scan of compact_scan_kernel -------------------------------------------------------------
COMPACT_SIZES = (4 * MI, 4 * MI + 1, 8 * MI + 4097, 12 * MI - 5)
COMPACT_CLEAN_SIZE = 4 * MI + 1


def compact_newline_blocks(n):
    """The 4096-byte blocks of input A that hold nothing but newlines: the first, both sides of the split after 1024 blocks, the last."""
    nblocks = (n + COMPACT_BLOCK_BYTES - 1) // COMPACT_BLOCK_BYTES
    return sorted({b for b in (0, SCAN_THREADS - 1, SCAN_THREADS, nblocks - 1) if b < nblocks})


def compact_input_a(n):
    """Uniform over all 256 byte values, about 5 % whitespace on top (the output offsets drift away from the input offsets), whole blocks
    of newlines where compact_newline_blocks says (block_kept = 0 on both sides of the split)."""
    rng = np.random.default_rng([0xC0A, n])
    a = rng.integers(0, 256, n, dtype=np.uint8)
    ws = np.flatnonzero(rng.integers(0, 20, n, dtype=np.uint8) == 0)
    a[ws] = np.frombuffer(b" \t\r\n", dtype=np.uint8)[rng.integers(0, 4, len(ws))]
    for b in compact_newline_blocks(n):
        a[b * COMPACT_BLOCK_BYTES:(b + 1) * COMPACT_BLOCK_BYTES] = 0x0A
    return a.tobytes()


def compact_input_b(n=COMPACT_CLEAN_SIZE):
    """Nothing to change and nothing to delete: normalize reports `None`, strip_returns borrows."""
    unit = b"ACGTNACGT-"
    return (unit * (n // len(unit) + 1))[:n]


# ---- (b) reverse_complement / quality_mask: the second trip of the grid-stride loop ---------------------------------------------------
GRID_N = (1 << 28) + 4097
QUALITY_SCORE = 100


def grid_inputs(n=GRID_N):
    """(sequence, quality): n random bytes of any value each."""
    rng = np.random.default_rng(0x6B1D)
    return rng.bytes(n), rng.bytes(n)


# ---- (c) item arrays: the carry of cp_scan_kernel ---------------------------------------------------------------------------------------
# One record past 1024 blocks of 16 384 positions.  All-N stretches of 40 000 bytes at the start, over position 16 Mi (the last block of
# scan tile 0 and the first block of tile 1 hold no item) and at the end; between the middle stretch and the last one lie some 22 000
# bases, so that scan tile 1 holds items of its own: their offsets are the carry, and a capacity that ends 1000 items into tile 1 can run out.
CP_N_STRETCH = 40_000
CP_SPLIT = SCAN_THREADS * CP_BLOCK_POSITIONS                      # position 16 Mi
CP_RECORD_LEN = CP_SPLIT + 5 * CP_BLOCK_POSITIONS + 5
CP_RAGGED_CHUNK_BYTES = 40 * MI
CP_RAGGED_MIN_BYTES = 20 * MI
CP_SMALL = (b"ACGTTGCAnACGTACGTACGTTTGACCAGTacgtacgGATTACA" * 9, b"TTGACCAGTNNACGTACGATCGATCGTAGCTAGCTAGCTAGCATCGAT" * 5, b"GATTACA" * 40)


def cp_record():
    rng = np.random.default_rng(0xC9)
    n = CP_RECORD_LEN
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
    a[rng.integers(0, n, n // 5000)] = ord("N")
    a[:CP_N_STRETCH] = ord("N")
    a[CP_SPLIT - CP_N_STRETCH // 2: CP_SPLIT + CP_N_STRETCH // 2] = ord("N")
    a[n - CP_N_STRETCH:] = ord("N")
    return a.tobytes()


def cp_batch(record):
    """[small, the record, small, empty, small]: at the default chunk size the oversize record becomes a chunk of its own."""
    return [CP_SMALL[0], record, CP_SMALL[1], b"", CP_SMALL[2]]


def ragged_records(min_bytes, seed, alphabet, forced_starts=()):
    """Records of 0..4000 bytes drawn from `alphabet` until they total min_bytes or more.  forced_starts: byte offsets (ascending, at
    most 4000 apart from whatever precedes them) at which a record has to begin - the record before it is given the length that ends there."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    forced = sorted(set(forced_starts))
    lengths, at, f = [], 0, 0
    while at < min_bytes or f < len(forced):
        n = int(rng.integers(0, 4001))
        if f < len(forced) and forced[f] - at <= 4000:   # (a drawn length never passes a forced start: it is at most 4000)
            n = forced[f] - at
            f += 1
        lengths.append(n)
        at += n
    flat = letters[rng.integers(0, len(letters), at)].tobytes()
    offs = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    return [flat[offs[i]:offs[i + 1]] for i in range(len(lengths))]


def cp_ragged_records():
    """About 10 500 ragged records, mixed case, N and '-', 20 MiB or more: one chunk once NTK_OPT_COMPAT_CHUNK_BYTES is 40 MiB."""
    return ragged_records(CP_RAGGED_MIN_BYTES, 0xC7, b"ACGT" * 12 + b"acgt" + b"Nn-")


# ---- (d) planes: several tiles per block -------------------------------------------------------------------------------------------------
def planes_min_bytes(cu):
    return (2 * cu * PL_BLOCKS_PER_CU + 3) * PL_TILE + 777


def planes_forced_starts(cu):
    """Records that begin exactly on a tile boundary, one byte before and one after it: near the start, at the first tile that is some
    block's second (tile n_cu * 8) and deep in the second round."""
    grid = cu * PL_BLOCKS_PER_CU
    out = []
    for j in (1, 2, 37, grid - 1, grid, grid + 1, grid + 500, 2 * grid):
        out += [PL_TILE * j - 1, PL_TILE * j, PL_TILE * j + 1]
    return out


def planes_records(cu):
    return ragged_records(planes_min_bytes(cu), [0xD1, cu], b"ACGT" * 12 + b"acgt" + b"NnUu", planes_forced_starts(cu))


def expected_planes(rec_bit, n_words, items, with_values=False):
    """The valid16 / rc16 planes (and the dense values) from per-record oracle arrays: items[i] = (pos, [val,] flag) of record i, placed at
    plane position rec_bit[i] + pos; bit 15 - p % 16 of word p / 16."""
    v = np.zeros(n_words * 16, dtype=np.uint8)
    r = np.zeros(n_words * 16, dtype=np.uint8)
    vals = np.zeros(n_words * 16, dtype=np.uint64) if with_values else None
    for i, it in enumerate(items):
        idx = int(rec_bit[i]) + it[0].astype(np.int64)
        v[idx] = 1
        r[idx] = it[-1]
        if with_values:
            vals[idx] = it[1]
    pack = lambda bits: np.packbits(bits).view(">u2").astype(np.uint16)
    return pack(v), pack(r), vals


# ---- (e) minimizer: thousands of candidates per thread, ties across threads and waves ---------------------------------------------------
MINIMIZER_N = 262_144 + 37
MINIMIZER_LENGTHS = (1, 21, 40)
MINIMIZER_BATCH_LENGTH = 12


def _random_bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _revcomp_acgt(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def minimizer_inputs():
    """name -> sequence.  Every one but `random` is full of ties for every length: equal candidates held by different threads and waves."""
    n = MINIMIZER_N
    rng = np.random.default_rng(0xE1)
    h = _random_bases(rng, n // 2)
    return {
        "random": _random_bases(rng, n, b"ACGTacgtN"),
        "homopolymer": b"A" * n,
        "AT": b"AT" * (n // 2),
        "ACGT": b"ACGT" * (n // 4),
        "inverted_repeat": h + _revcomp_acgt(h),   # (its own reverse complement: forward and reverse window i are equal for every i)
    }


MINIMIZER_TIE_HEAVY = ("homopolymer", "AT", "ACGT", "inverted_repeat")


def minimizer_batch_records():
    """Both sides of the hand-over from the wave kernel to the one-block kernel, and three long records in one chunk (they share d_best)."""
    rng = np.random.default_rng(0xE2)
    small = b"GATTACAGATTACA"
    return [small, _random_bases(rng, LONG_RECORD - 1), _random_bases(rng, LONG_RECORD), _random_bases(rng, LONG_RECORD + 1), b"AC" * 100_000,
            _random_bases(rng, 70_000), b"TTTTTTTTTTTTTTTTTTTTTTTTT"]


# ---- the chunk pipeline of the batched calls (tests/test_gpu_parity.py; tests/test_compat_plan.py cuts the same lists on the CPU) --------
def parity_item_records():
    """The batch of test_batched_compat_face_matches_the_iterators_per_record: ragged, empty and all-N records, mixed case."""
    rng = np.random.default_rng(21)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNn-", dtype=np.uint8)
    records = [b"", b"A", b"N" * 40, b"ACGT" * 10, b"acgtACGTnACGTTGCA" * 3]
    for _ in range(400):
        records.append(bytes(alphabet[rng.integers(0, len(alphabet), int(rng.integers(0, 400)))]))
    records += [b"", bytes(alphabet[rng.integers(0, 4, 3000)])]
    return records


def parity_bit_plane_records():
    """The batch of test_bit_kmers_planes_face_matches_the_iterator_per_record: as above, with U (a break on the bit path) and palindromes."""
    rng = np.random.default_rng(57)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNnU-", dtype=np.uint8)
    records = [b"", b"A", b"N" * 40, b"ACGT" * 10, b"acgtACGTnACGTTGCA" * 3, b"AATT", b"GAATTC" * 6]
    for _ in range(300):
        records.append(bytes(alphabet[rng.integers(0, len(alphabet), int(rng.integers(0, 400)))]))
    records.append(bytes(rng.choice(list(b"ACGT"), size=5000).astype(np.uint8)))
    return records


PIPELINE_CHUNK_OPTIONS = (64, 97)     # the NTK_OPT_COMPAT_CHUNK_BYTES values at which the two kinds of batch below are run
PIPELINE_RECORD_LEN = 40              # 40 + 1 <= 64 < 2 * (40 + 1) and 40 <= 64 < 2 * 40: one record per chunk at 64, packed or not
PIPELINE_BATCH_SIZES = (1, 2, 3, 4, 7)   # chunk counts below, at and above BANKS, and past two turns of the banks


def empties_around_oversize():
    """Chunks of nothing but empty records on both sides of a record larger than the chunk: {0}, {1}, {2, 3} where records are uploaded
    as they lie; with a break byte per record at a chunk of 64, {0}, {1}, {2, 3} as well (1 <= 64 < 102; 2 <= 64)."""
    return [b"", b"ACGT" * 25, b"", b""]


def bank_count_batches():
    """Batches of 1, 2, 3, 4 and 7 records of PIPELINE_RECORD_LEN bytes (mixed case, an N): chunk counts around the bank count."""
    rng = np.random.default_rng(0xBA)
    letters = np.frombuffer(b"ACGT" * 6 + b"acgtN", dtype=np.uint8)
    return [[bytes(letters[rng.integers(0, len(letters), PIPELINE_RECORD_LEN)]) for _ in range(n)] for n in PIPELINE_BATCH_SIZES]
