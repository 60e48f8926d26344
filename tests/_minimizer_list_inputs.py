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
