"""The inputs of tests/test_gpu_minimizer_list.py, in one place so that tests/test_minimizer_list_model.py can prove them non-vacuous on
the CPU from the host model alone.  Importable without a GPU."""
import itertools

import numpy as np

import _minimizer_list_model as MM

SEED = 0x317157
CUTOFF = 53
KW = ((21, 11), (15, 10), (31, 19), (32, 256), (1, 1), (32, 1), (5, 16), (7, 17))
SEAM_W = (2, 16, 17, 256)
SEAM_K = 5
CHUNK_KW = ((21, 11), (32, 256))
CHUNK_BYTES = MM.CHUNK + (8 << 10)
EARLY_AT = 1000            # a few entries in the first chunk, so that the second chunk's entries are added to a list that holds some
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def short_records():
    """Every record over ACGT of length 0..7: 21 845 of them."""
    return [bytes(t) for n in range(8) for t in itertools.product(b"ACGT", repeat=n)]


def random_records(k, w, seed=SEED):
    """Records of lengths {0, 1, k - 1, k, k + w - 2, k + w - 1, k + w, 150, 700} with N runs, lower case, U / u and IUPAC letters, and
    their qualities, 5 % of them under CUTOFF."""
    rng = np.random.default_rng([seed, k, w])
    lens = [0, 1, k - 1, k, k + w - 2, k + w - 1, k + w] * 3 + [150] * 12 + [700] * 4 + [0, 0]
    recs, quals = [], []
    for L in (lens[i] for i in rng.permutation(len(lens))):
        a = _ACGT[rng.integers(0, 4, L)].copy()
        if L >= 150:
            for _ in range(int(rng.integers(0, 3))):
                s = int(rng.integers(0, L))
                a[s: s + int(rng.integers(1, 4))] = ord("N")
            m = rng.random(L) < 0.01
            extra = np.frombuffer(b"UuacgtRYn", dtype=np.uint8)
            a[m] = extra[rng.integers(0, extra.size, int(m.sum()))]
            if rng.random() < 0.25:   # a low-complexity stretch: ties
                s = int(rng.integers(0, L - 60))
                a[s: s + 60] = _ACGT[int(rng.integers(0, 4))]
        q = np.full(L, 70, dtype=np.uint8)
        q[rng.random(L) < 0.05] = CUTOFF - 1
        recs.append(a.tobytes())
        quals.append(q.tobytes())
    return recs, quals


def aimed_piece(k, w):
    """T * (w + 1), A * k, T * (w + 1) on the forward bit path: the all-A k-mer is the smallest key of every window that holds it, w of
    them, and the first of those ends where the k-mer ends: at byte w + k of the piece."""
    return b"T" * (w + 1) + b"A" * k + b"T" * (w + 1)


def aim_offset(k, w):
    return w + k


class Sparse:
    """A batch of `n_bytes` of N with pieces at given positions; every piece is a record that starts `lead` bytes before it (the first
    record at 0) and ends with a break byte."""

    def __init__(self, n_bytes, pieces, lead=3, one_record=False):
        self.n_bytes, self.pieces = n_bytes, sorted(pieces)
        for (p, b), (q, _) in zip(self.pieces, self.pieces[1:]):
            assert p + len(b) + lead + 1 <= q, "pieces are apart"
        assert self.pieces[0][0] >= lead and self.pieces[-1][0] + len(self.pieces[-1][1]) < n_bytes
        starts = [0] if one_record else [0] + [p - lead for p, _ in self.pieces[1:]]
        self.offsets = np.array(starts + [n_bytes], dtype=np.uint64)

    def region(self, lo, hi):
        """The bytes [lo, hi) of the batch."""
        a = np.full(hi - lo, ord("N"), dtype=np.uint8)
        for p, b in self.pieces:
            s, e = max(p, lo), min(p + len(b), hi)
            if s < e:
                a[s - lo: e - lo] = np.frombuffer(b, dtype=np.uint8)[s - p: e - p]
        breaks = self.offsets[1:].astype(np.int64) - 1
        a[breaks[(breaks >= lo) & (breaks < hi)] - lo] = ord("\n")
        return a

    def buf(self):
        return self.region(0, self.n_bytes)

    def entries(self, k, w, path, pre, order):
        """The model's entries: the pieces are laid side by side with an N between them, and every entry is moved to where its piece
        lies in the batch (no window spans two pieces)."""
        compact = b"N".join(b for _, b in self.pieces)
        at = np.concatenate([[0], np.cumsum([len(b) + 1 for _, b in self.pieces])])[:-1]
        ent = MM.entries_of(compact, k, w, path, pre, order)
        piece = np.searchsorted(at, ent.end, side="right") - 1
        shift = np.array([p for p, _ in self.pieces], dtype=np.int64)[piece] - at[piece]
        return MM.Entries(ent.end + shift, ent.picked + shift, ent.value, ent.strand, ent.span)

    def csr(self, k, w, path, pre, order):
        return MM.csr(self.entries(k, w, path, pre, order), self.offsets, self.n_bytes, k)


def tile_seam_batch(w, grid_tiles, k=SEAM_K):
    """The all-A k-mer's first window end at tile boundary + d for every d in -(w + 1) .. w + 1, each d in the first, a middle and the
    last step of a block's loop over the tiles (the grid is `grid_tiles` blocks, block b takes the tiles b, b + grid, b + 2 grid): the d-th
    aim is at the boundaries in front of the tiles 1 + 3 d', grid + 1 + 3 d' and 2 grid + 1 + 3 d'.  Then a record of 3 000 T across a
    boundary: an entry at every window.  Returns (Sparse, the aimed first window ends)."""
    ds = list(range(-(w + 1), w + 2))
    assert 3 * len(ds) + 2 < grid_tiles and len(aimed_piece(k, w)) + 8 < MM.TILE
    pieces, aims = [], []
    for step in range(3):
        for i, d in enumerate(ds):
            e = (step * grid_tiles + 1 + 3 * i) * MM.TILE + d
            aims.append(e)
            pieces.append((e - aim_offset(k, w), aimed_piece(k, w)))
    last = (2 * grid_tiles + 3 * len(ds) + 4) * MM.TILE
    pieces.append((last - 1500, b"T" * 3000))
    return Sparse(last + 4 * MM.TILE, pieces), aims


def chunk_seam_ds(k, w):
    return list(range(-(w + k), w + k + 1))


def chunk_seam_case(k, w, d):
    """One record across the chunk seam: a few T in the first chunk, and the all-A k-mer's first window end at seam + d."""
    e = MM.CHUNK + d
    return Sparse(CHUNK_BYTES, [(EARLY_AT, b"T" * (k + w + 3)), (e - aim_offset(k, w), aimed_piece(k, w))], one_record=True), e


def chunk_seam_region(k, w):
    """The bytes [lo, hi) of the batch that the cases of (k, w) rewrite."""
    reach = 2 * (w + k) + len(aimed_piece(k, w)) + 16
    return MM.CHUNK - reach, MM.CHUNK + reach


def growth_case(k, w):
    """One record across the chunk seam whose second chunk adds more entries than the first allocation of the held list holds: a few T
    early in the first chunk, and 2 000 T across the seam - an entry at every window.  Returns (Sparse, the region it rewrites)."""
    at = MM.CHUNK - 700
    return Sparse(CHUNK_BYTES, [(EARLY_AT, b"T" * (k + w + 3)), (at, b"T" * 2000)], one_record=True), (at - 16, at + 2016)


def stream_batches():
    """(true, decoy) of the stream-order case: tests/_stream_order.py's batches at k = 21."""
    import _stream_order as S
    return S.batches(21)


# ---- exact past one step of the capped grid ------------------------------------------------------------------------------------------------

GRID_STEPS = 1.25
# (k, w, order, path, pre)
GRID_CASES = ((11, 5, MM.HASH, MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE), (15, 19, MM.LEX, MM.PATH_BITS_CANONICAL, MM.PRE_NONE))
_grid_cache = {}


def grid_batch(grid_tiles, seed=SEED):
    """Random 150-base reads over GRID_STEPS steps of a grid of `grid_tiles` blocks (a block takes a tile of MM.TILE window ends per step):
    (packed batch, quality stream, offsets).  One base in 512 is an N, 2 % of the quality bytes are under CUTOFF.  Made once per size."""
    if grid_tiles not in _grid_cache:
        rng = np.random.default_rng([seed, grid_tiles])
        n_reads = -(-int(GRID_STEPS * grid_tiles * MM.TILE) // 151)
        a = _ACGT[rng.integers(0, 4, n_reads * 151)]
        a[rng.random(a.size) < 1 / 512] = ord("N")
        a[150::151] = ord("\n")
        qual = np.full(a.size, 70, dtype=np.uint8)
        qual[rng.random(a.size) < 0.02] = CUTOFF - 1
        _grid_cache.clear()
        _grid_cache[grid_tiles] = (a.tobytes(), qual, np.arange(n_reads + 1, dtype=np.uint64) * 151)
    return _grid_cache[grid_tiles]


# ---- many records around the chunk seam ----------------------------------------------------------------------------------------------------

SEAM_LO, SEAM_HI = MM.CHUNK - (24 << 10), MM.CHUNK + (8 << 10)
SEAM_LAYOUTS = ("straddle", "starts")
SEAM_LONG = 300


class Packed(Sparse):
    """A batch of `n_bytes` of N with an early piece and, from `lo` on, packed records (each followed by its break byte).  Record 0 is
    the bytes in front of `lo`, the last record what follows the packed ones; both end with a break byte."""

    def __init__(self, n_bytes, early, lo, records):
        self.n_bytes, self.records, self.lo = n_bytes, records, lo
        packed = b"".join(r + b"\n" for r in records)
        self.pieces = [early, (lo, packed)]
        starts = lo + np.concatenate([[0], np.cumsum([len(r) + 1 for r in records])])
        assert early[0] + len(early[1]) < lo and starts[-1] < n_bytes
        self.offsets = np.concatenate([[0], starts, [n_bytes]]).astype(np.uint64)


def seam_records(k, w, layout, seed=SEED):
    """A few thousand packed records of 0 .. 300 bases in [SEAM_LO, SEAM_HI) of the chunk-seam batch - most of them of 0 .. 2 bases, one
    in 40 of 280 .. 300 (long enough for a window at k + w = 288), one in 40 of any length - around a fixed middle:
      "straddle"  one record of 300 bases from CHUNK - 20 on: it straddles the seam, and its start lies inside the halo of every (k, w);
      "starts"    records that start exactly at CHUNK - 1 and CHUNK (both empty) and at CHUNK + 1 (300 bases)."""
    rng = np.random.default_rng([seed, k, w, SEAM_LAYOUTS.index(layout)])
    rand = lambda n: _ACGT[rng.integers(0, 4, n)].tobytes()   # noqa: E731

    def draw():
        u = rng.random()
        return rand(int(rng.integers(0, 3)) if u < 0.95 else int(rng.integers(280, SEAM_LONG + 1)) if u < 0.975 else int(rng.integers(0, SEAM_LONG + 1)))

    middle_at, middle = (MM.CHUNK - 20, [rand(SEAM_LONG)]) if layout == "straddle" else (MM.CHUNK - 1, [b"", b"", rand(SEAM_LONG)])
    recs, at = [], SEAM_LO
    while middle_at - at > SEAM_LONG + 1:
        recs.append(draw())
        at += len(recs[-1]) + 1
    recs.append(rand(middle_at - at - 1))     # 0 .. 300 bases: the next record starts at middle_at
    recs += middle
    at = middle_at + sum(len(r) + 1 for r in middle)
    while True:
        r = draw()
        if at + len(r) + 1 > SEAM_HI:
            break
        recs.append(r)
        at += len(r) + 1
    return Packed(CHUNK_BYTES, (EARLY_AT, b"T" * (k + w + 3)), SEAM_LO, recs)


# ---- offsets the header defines and the packer never makes ---------------------------------------------------------------------------------

ODD_KW = (7, 17)
ODD_TILES = 6
ODD_RUN = 5000
ODD_TAIL = 36            # equal starts in front of the last one: a doubling search from the first of them steps over offsets[n_records]


def odd_offsets_batch(seed=SEED):
    """(batch, offsets) of ODD_TILES tiles: random bases in the tiles 0, 1, 4 and 5, N in the tiles 2 and 3.  The offsets are
    non-decreasing and not the packer's: offsets[0] = 100, offsets[n_records] = n_bytes - 144, a run of ODD_RUN equal starts in the middle
    of tile 1 and another in the N of tile 2, and ODD_TAIL equal starts stand in front of the last one, offsets[n_records], which is a
    start of its own.  A break byte stands in front of every start, so that no record starts inside a window.  (Six tiles are six blocks
    of ml_scatter_kernel with one tile each: nothing is carried from tile to tile here - `carry_batch` is the case for that.)"""
    rng = np.random.default_rng([seed, 0x0DD])
    n = ODD_TILES * MM.TILE
    a = _ACGT[rng.integers(0, 4, n)].copy()
    a[2 * MM.TILE: 4 * MM.TILE] = ord("N")
    distinct = [100, 400, 401, 1000, MM.TILE + 500, MM.TILE + 900, 2 * MM.TILE + 700, 4 * MM.TILE - 3, 4 * MM.TILE + 600, 5 * MM.TILE, n - 344, n - 144]
    a[np.array(distinct) - 1] = ord("\n")
    a[n - 1] = ord("\n")
    runs = {MM.TILE + 500: ODD_RUN, 2 * MM.TILE + 700: ODD_RUN, n - 344: ODD_TAIL}
    off = np.concatenate([np.full(runs.get(s, 1), s, dtype=np.uint64) for s in distinct])
    return a.tobytes(), off


# ---- the two pre-steps no other case passes --------------------------------------------------------------------------------------------------

IUPAC_KW = (15, 10)
# (path, pre): STRIP_RETURNS on the bit paths, NORMALIZE_IUPAC on every path
IUPAC_PATH_PRES = ((MM.PATH_BITS, MM.PRE_STRIP_RETURNS), (MM.PATH_BITS_CANONICAL, MM.PRE_STRIP_RETURNS),
                   (MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE_IUPAC), (MM.PATH_BITS, MM.PRE_NORMALIZE_IUPAC),
                   (MM.PATH_BITS_CANONICAL, MM.PRE_NORMALIZE_IUPAC))


def iupac_records(seed=SEED):
    """40 records of 0 .. 400 bases; one byte in 40 is an IUPAC letter (either case), U or u, one in 10 a lower-case base."""
    rng = np.random.default_rng([seed, 0x1CAC])
    extra = np.frombuffer(b"RYKMSWBDHVNrykmswbdhvnUu", dtype=np.uint8)
    recs = []
    for L in [0, 1, 14, 15, 24, 25] + [int(x) for x in rng.integers(26, 401, 34)]:
        a = _ACGT[rng.integers(0, 4, L)].copy()
        m = rng.random(L)
        a[m < 0.1] |= 0x20
        sel = m > 1 - 1 / 40
        a[sel] = extra[rng.integers(0, extra.size, int(sel.sum()))]
        recs.append(a.tobytes())
    return recs


# ---- the record starts a block of ml_scatter_kernel carries along its run of tiles ----------------------------------------------------------

CARRY_KW = (11, 5)
CARRY_RUN = 5000


def carry_tiles(grid_tiles):
    """(n_tiles, per, early, mid, late): a batch of 2.25 steps of a grid of `grid_tiles` blocks, so that a block of ml_scatter_kernel takes
    per = 3 consecutive tiles, and the first tile of the three blocks the case is about."""
    n_tiles = 2 * grid_tiles + grid_tiles // 4
    per = -(-n_tiles // grid_tiles)
    return n_tiles, per, per * 1, per * (grid_tiles // 3), per * (n_tiles // per - 1)


class Tiles(Sparse):
    """A batch of N whose pieces are whole tiles of packed records; the offsets are the caller's."""

    def __init__(self, n_bytes, pieces, offsets):
        self.n_bytes, self.pieces, self.offsets = n_bytes, sorted(pieces), np.asarray(offsets, dtype=np.uint64)


def carry_batch(grid_tiles, seed=SEED):
    """N but for a few tiles of packed random records of 100 .. 200 bases, laid out against the runs of `per` = 3 tiles that the blocks of
    ml_scatter_kernel take on a device whose capped grid is `grid_tiles` blocks (block b: the tiles 3 b, 3 b + 1, 3 b + 2):
      early  records, records, N: CARRY_RUN equal starts at a record start in the middle of the first tile - the block carries the starts
             it counted there into its second tile;
      mid    records, N, records: CARRY_RUN equal starts in the middle of the N tile - the block skips it (`continue`) and goes on from the
             starts it knew at the end of its first tile, CARRY_RUN and more behind what the third tile needs;
      late   N, N, records: 100 equal starts in the second tile - both are skipped with nothing known, and the third tile searches all
             the starts of the batch.
    One more tile of records is the first of a block of its own.  Returns (Tiles, {name: first tile of the block})."""
    rng = np.random.default_rng([seed, 0xCA44, grid_tiles])
    T = MM.TILE
    n_tiles, per, early, mid, late = carry_tiles(grid_tiles)
    assert per == 3 and early + per <= per * 7 < mid and mid + per <= late
    pieces, starts = [], []

    def records(t):
        """Tile t as packed records; returns its record starts."""
        lens, left = [], T
        while left > 201:
            lens.append(int(rng.integers(100, 201)))
            left -= lens[-1] + 1
        lens.append(left - 1)
        a = np.concatenate([np.append(_ACGT[rng.integers(0, 4, n)], np.uint8(ord("\n"))) for n in lens])
        pieces.append((t * T, a.tobytes()))
        at = t * T + np.concatenate([[0], np.cumsum([n + 1 for n in lens])])[:-1]
        starts.extend(int(x) for x in at)
        return at

    first = records(early)
    starts += [int(first[len(first) // 2])] * (CARRY_RUN - 1)
    records(early + 1)
    records(per * 7)
    records(mid)
    starts += [(mid + 1) * T + T // 2] * CARRY_RUN
    records(mid + 2)
    starts += [(late + 1) * T + T // 2] * 100
    records(late + 2)
    return Tiles(n_tiles * T, pieces, sorted(starts) + [n_tiles * T]), dict(early=early, mid=mid, late=late)
