"""The host model of the minimizer-list library (tests/_minimizer_list_model.py) against the oracle, and the inputs of
tests/test_gpu_minimizer_list.py (tests/_minimizer_list_inputs.py) against the model: no GPU.

The identity the GPU tests lean on: with entries collapsed by the leftmost rule, the sum of span, the sum of span over flag 0, the sum
of span * value mod 2^64 and the xor of the values with odd span (and the histogram with span as the weight) are n_total, n_fwd, sum,
xor and hist of the oracle's windowed-minimizer reduce, which applies sequence::minimizer to every window."""
import numpy as np
import pytest

import _minimizer_list_inputs as I
import _minimizer_list_model as MM
import oracle as O  # the checker

KW = ((1, 1), (3, 1), (4, 5), (5, 16), (7, 17), (21, 11), (31, 19), (32, 3), (6, 49), (2, 64), (32, 256))
# (path, pre, the oracle's (accept_u, tie_rc))
BYTE_RULE = (MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE, (True, True))
BIT_RULE = (MM.PATH_BITS_CANONICAL, MM.PRE_NONE, (False, False))
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def inputs(k, w, seed=0x51):
    """Random, N-bearing, tandem-repeat, poly-A / poly-T and palindromic sequences, long enough for windows of w k-mers; '\\n' between."""
    rng = np.random.default_rng([seed, k, w])
    L = 2 * (k + w) + 300
    rand = lambda n: _ACGT[rng.integers(0, 4, n)].tobytes()   # noqa: E731
    with_n = bytearray(rand(L))
    for _ in range(4):
        s = int(rng.integers(0, L))
        with_n[s: s + int(rng.integers(1, 4))] = b"N" * len(with_n[s: s + int(rng.integers(1, 4))])
    unit = rand(int(rng.integers(1, 7)))
    half = rand(k + w)
    pal = half + half[::-1].translate(_COMP)
    return [rand(L), bytes(with_n), unit * (L // len(unit)), b"A" * L, b"T" * (L // 2) + b"A" * (L // 2), pal + rand(20) + pal, rand(k + w - 2),
            rand(k + w - 1), b""]


@pytest.mark.parametrize("k,w", KW)
def test_lex_digest_on_a_canonical_path_is_the_oracles(k, w):
    seqs = inputs(k, w)
    buf = b"".join(s + b"\n" for s in seqs)
    for path, pre, rule in (BYTE_RULE, BIT_RULE):
        ent = MM.entries_of(buf, k, w, path, pre, MM.LEX)
        want = O.minimizers_reduce(buf, k, w, *rule)
        assert want["n_total"] > 0
        assert MM.same_digest(MM.digest(ent.value, ent.strand, ent.span, k), want), (k, w, path)
        assert np.all(ent.span >= 1) and np.all(ent.span <= w) and np.all(np.diff(ent.end) > 0)
        # inside a run of windows the positions strictly increase: a run ends where the next entry does not follow on
        follows = ent.end[1:] == ent.end[:-1] + ent.span[:-1]
        assert np.all(np.diff(ent.picked)[follows] > 0)
        # whatever the offsets: one record, the packer's, and cuts that are nobody's
        for off in ([0, len(buf)], MM.packed_offsets(seqs), [0, 7, 7, len(buf) // 2, len(buf) + 50]):
            out, pos, values, strand, span = MM.csr(ent, off, len(buf), k)
            assert MM.same_digest(MM.digest(values, strand, span, k), want) and out[0] == 0 and out[-1] == len(ent)


@pytest.mark.parametrize("k", [1, 3, 4, 21, 32])
def test_with_w_1_the_entries_are_the_iterators_items(k):
    seqs = inputs(k, 3, seed=0x52)
    for path in (MM.PATH_BITS, MM.PATH_BITS_CANONICAL, MM.PATH_BYTES_CANONICAL):
        pre = MM.PRE_NORMALIZE if path == MM.PATH_BYTES_CANONICAL else MM.PRE_NONE
        for order in (MM.LEX, MM.HASH):
            out, pos, values, strand, span = MM.lists(seqs, k, 1, path, pre, order)
            for r, s in enumerate(seqs):
                lo, hi = int(out[r]), int(out[r + 1])
                if path == MM.PATH_BYTES_CANONICAL:
                    rc = O.reverse_complement(s)
                    items = [(p, O.bytes_to_bitmer(sl), f) for p, sl, f in O.canonical_kmers(s, rc, k)]
                else:
                    items = [(p, v, f) for p, (v, _), f in O.bit_kmers(s, k, path == MM.PATH_BITS_CANONICAL)]
                assert list(zip(pos[lo:hi].tolist(), values[lo:hi].tolist(), strand[lo:hi].astype(bool).tolist())) == items, (k, path, r)
                assert np.all(span[lo:hi] == 1)


def test_hash_order_differs_from_lex_where_it_must():
    """poly-A between random flanks: in LEX order the all-A k-mer (value 0) wins every window it is in; by hash it need not.  And the two
    orders are the same rule on other keys: sorting by hash gives the HASH order's picks."""
    k, w = 7, 9
    rng = np.random.default_rng(0x53)
    seq = _ACGT[rng.integers(0, 4, 200)].tobytes() + b"A" * 40 + _ACGT[rng.integers(0, 4, 200)].tobytes()
    lex, hsh = (MM.lists([seq], k, w, MM.PATH_BITS, MM.PRE_NONE, order) for order in (MM.LEX, MM.HASH))
    assert (lex[2] == 0).sum() > 20 and (lex[2] == 0).sum() > (hsh[2] == 0).sum()
    assert lex[1].tolist() != hsh[1].tolist() and int(lex[4].sum()) == int(hsh[4].sum()) == len(seq) - (k + w - 1) + 1
    values, valid, _ = MM.planes(seq + b"\n", k, MM.PATH_BITS, MM.PRE_NONE)
    whole, picked = MM.windows(MM.fmix64(values ^ np.uint64(MM.XOR)), valid, w, MM.LEX)
    whole2, picked2 = MM.windows(values, valid, w, MM.HASH)
    assert np.array_equal(whole, whole2) and np.array_equal(picked[whole], picked2[whole])
    assert int(MM.fmix64(np.array([0], dtype=np.uint64))[0]) == 0 and len(set(MM.fmix64(np.arange(1000, dtype=np.uint64)).tolist())) == 1000


def test_a_quality_mask_ends_windows():
    k, w = 5, 4
    seq = b"ACGTTGCAAGGCTTACGATCGGATCAGCTA"
    qual = np.full(len(seq) + 1, 70, dtype=np.uint8)
    qual[15] = 10
    plain = MM.lists([seq], k, w, MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE)
    masked = MM.lists([seq], k, w, MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE, quals=[qual[:-1].tobytes()], cutoff=53)
    same = MM.lists([seq[:15] + b"N" + seq[16:]], k, w, MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE)
    assert int(masked[4].sum()) < int(plain[4].sum()) and all(np.array_equal(a, b) for a, b in zip(masked, same))


# ---- the inputs of the GPU file are not vacuous -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", I.SEAM_W)
def test_tile_seam_inputs_put_a_first_window_on_each_side(w):
    k, grid = I.SEAM_K, 256 * MM.BLOCKS_PER_CU
    sp, aims = I.tile_seam_batch(w, grid)
    ent = sp.entries(k, w, MM.PATH_BITS, MM.PRE_NONE, MM.LEX)
    aimed = ent.end[ent.value == 0]
    assert aimed.tolist() == sorted(aims) and np.all(ent.span[ent.value == 0] == w) and np.all(ent.picked[ent.value == 0] == aimed)
    d = np.array(aims) - (np.array(aims) + MM.TILE // 2) // MM.TILE * MM.TILE     # the distance to the nearest tile boundary
    assert sorted(set(d.tolist())) == list(range(-(w + 1), w + 2))
    steps = {int(e) // MM.TILE // grid for e in aims}
    assert steps == {0, 1, 2} and sp.n_bytes > 2 * grid * MM.TILE, "the first, a middle and the last step of a block's loop"
    tail = ent.span[ent.end >= sp.pieces[-1][0]]
    assert tail.size == 3000 - (k + w - 1) + 1 and np.all(tail == 1)
    crossing = ent.end[ent.end >= sp.pieces[-1][0]]
    assert crossing.min() // MM.TILE < crossing.max() // MM.TILE


@pytest.mark.parametrize("k,w", I.CHUNK_KW)
def test_chunk_seam_inputs_put_a_first_window_on_each_side(k, w):
    sides, splits = set(), set()
    for d in I.chunk_seam_ds(k, w):
        sp, e = I.chunk_seam_case(k, w, d)
        ent = sp.entries(k, w, MM.PATH_BITS, MM.PRE_NONE, MM.LEX)
        hit = np.flatnonzero(ent.value == 0)
        assert hit.size == 1 and ent.end[hit[0]] == e == MM.CHUNK + d and ent.span[hit[0]] == w
        sides.add(e >= MM.CHUNK)
        if e < MM.CHUNK <= e + w - 1:
            splits.add(MM.CHUNK - e)     # the windows of the entry that end in front of the seam
        lo, hi = I.chunk_seam_region(k, w)
        assert lo <= sp.pieces[1][0] and sp.pieces[1][0] + len(sp.pieces[1][1]) <= hi and (ent.end < MM.CHUNK).any()
    assert sides == {False, True} and splits == set(range(1, w))
    assert I.chunk_seam_ds(k, w)[0] == -(w + k) and I.chunk_seam_ds(k, w)[-1] == w + k


def test_the_stream_order_decoy_has_another_answer():
    t, d = I.stream_batches()
    k, w = 21, 11
    true = MM.csr(MM.entries_of(t.buf, k, w, MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE, MM.HASH, t.qual, I.CUTOFF), t.offsets, t.n, k)
    assert true[1].size > 100
    for name, buf, qual, off in (("decoy batch", d.buf, t.qual, t.offsets), ("decoy qualities", t.buf, d.qual, t.offsets),
                                 ("decoy offsets", t.buf, t.qual, np.zeros_like(t.offsets)), ("clobbered batch", b"N" * t.n, t.qual, t.offsets),
                                 ("no qualities", t.buf, np.full(t.n, 0xFF, dtype=np.uint8), t.offsets)):
        other = MM.csr(MM.entries_of(buf, k, w, MM.PATH_BYTES_CANONICAL, MM.PRE_NORMALIZE, MM.HASH, qual, I.CUTOFF), off, t.n, k)
        assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(true, other)), name


def test_random_records_cover_their_lengths():
    for k, w in I.KW:
        recs, quals = I.random_records(k, w)
        lens = {len(r) for r in recs}
        assert {0, 1, k - 1, k, k + w - 2, k + w - 1, k + w, 150, 700} <= lens and all(len(r) == len(q) for r, q in zip(recs, quals))
        text = b"".join(recs)
        assert b"N" in text and b"U" in text or b"u" in text
        assert any(min(q) < I.CUTOFF for q in quals if q)
    assert len(I.short_records()) == sum(4 ** n for n in range(8))


def test_device_bytes_restates_the_header():
    """The model's restatement of the header's memory statement, which the GPU test holds stats.device_bytes to."""
    assert MM.device_bytes(0, 5, 21, 11, []) == MM.grow_half_again(6) * 8 == (6 + 3 + 64) * 8
    one = MM.device_bytes(1000, 3, 21, 11, [10])
    assert one == 1008 * 8 + 2 * 63 * 2 + 1008 * 2 + 2 * 2 * 4 + 16 + MM.grow_half_again(4) * 8 + MM.grow_half_again(10) * 28
    two = MM.device_bytes(MM.CHUNK + 100, 1, 32, 256, [4, 300])
    bases = MM.CHUNK + 288 + 255 + 1      # the halo of k + w = 288, the tail w - 1, up to a multiple of 16
    assert MM.halo(32, 256) == 288 and bases % 16 == 0
    assert two == bases * 8 + bases // 16 * 4 + bases * 2 + 2 * (65537 + 1) * 4 + 16 + MM.grow_half_again(2) * 8 + MM.grow_half_again(304) * 28


# ---- the inputs of the exact cases: the capped grid, many records at the chunk seam, odd offsets, the two other pre-steps ------------------

@pytest.mark.parametrize("k,w,order,path,pre", I.GRID_CASES)
def test_grid_batch_is_random_masked_and_crosses_tiles(k, w, order, path, pre):
    """At a grid of 64 blocks (the GPU test sizes it from the device): more than one step of tiles, entries of both strands across tile
    boundaries, and a quality stream that changes the result."""
    grid = 64
    buf, qual, off = I.grid_batch(grid)
    assert grid * MM.TILE < len(buf) < 1.3 * grid * MM.TILE and off[-1] == len(buf) and qual.size == len(buf) and set(np.diff(off).tolist()) == {151}
    ent = MM.entries_of(buf, k, w, path, pre, order, qual, I.CUTOFF)
    plain = MM.entries_of(buf, k, w, path, pre, order)
    assert len(ent) != len(plain) and int(ent.span.sum()) < int(plain.span.sum())
    last = ent.end + ent.span.astype(np.int64) - 1
    assert int((ent.end // MM.TILE < last // MM.TILE).sum()) > grid // 4, "entries whose windows end on both sides of a tile boundary"
    assert (ent.strand == 0).any() and (ent.strand == 1).any() and (ent.end >= grid * MM.TILE).any()
    assert I.GRID_STEPS == 1.25 and {c[2] for c in I.GRID_CASES} == {MM.LEX, MM.HASH}


@pytest.mark.parametrize("k,w", I.CHUNK_KW)
def test_seam_records_put_many_records_on_both_sides(k, w):
    starts_seen, halo_start, straddler = set(), False, False
    for layout in I.SEAM_LAYOUTS:
        sr = I.seam_records(k, w, layout)
        s = sr.offsets.astype(np.int64)
        assert len(s) - 1 >= 2000 and s[0] == 0 and s[1] == I.SEAM_LO and s[-1] == I.CHUNK_BYTES and s[-2] <= I.SEAM_HI and np.all(np.diff(s) >= 1)
        assert max(len(r) for r in sr.records) == I.SEAM_LONG and min(len(r) for r in sr.records) == 0
        region = sr.region(I.SEAM_LO - 16, I.SEAM_HI + 16)
        assert np.all(region[s[1:-1] - 1 - (I.SEAM_LO - 16)] == ord("\n")) and region.tobytes()[16:16 + s[-2] - I.SEAM_LO] == b"".join(r + b"\n" for r in sr.records)
        ent = sr.entries(k, w, MM.PATH_BITS, MM.PRE_NONE, MM.HASH)
        rec = np.searchsorted(s, ent.end, side="right") - 1
        first, second = ent.end < MM.CHUNK, ent.end >= MM.CHUNK
        assert (ent.end[first] < 2 * I.EARLY_AT).any(), "the early piece"
        assert len(set(rec[first & (ent.end >= I.SEAM_LO)])) >= 3 and len(set(rec[second])) >= 3, "entries in three records or more on each side"
        straddler |= bool(((s[rec] < MM.CHUNK) & second).any())   # the record starts in the first chunk, the entry's first window ends in the second
        starts_seen |= {int(x) - MM.CHUNK for x in s if abs(int(x) - MM.CHUNK) <= 1}
        halo_start |= bool(((s >= MM.CHUNK - MM.halo(k, w)) & (s < MM.CHUNK)).any())
        assert ((s[:-1] < MM.CHUNK) & (s[1:] > MM.CHUNK)).sum() == (layout == "straddle")   # a record with bytes on both sides of the seam
        want = MM.csr(ent, sr.offsets, sr.n_bytes, k)
        assert want[0][0] == 0 and want[0][-1] == len(ent) and int(want[1][int(want[0][1]):].max()) <= I.SEAM_LONG - k
    assert starts_seen == {-1, 0, 1} and halo_start and straddler


def test_odd_offsets_are_what_the_header_defines_and_the_packer_never_makes():
    k, w = I.ODD_KW
    buf, off = I.odd_offsets_batch()
    T = MM.TILE
    assert len(buf) == I.ODD_TILES * T >= 5 * T and np.all(np.diff(off.astype(np.int64)) >= 0) and off[0] > 0 and off[-1] < len(buf)
    values, counts = np.unique(off, return_counts=True)
    runs = values[counts == I.ODD_RUN].astype(np.int64)
    assert runs.size == 2 and sorted(counts.tolist())[:-3] == [1] * (values.size - 3)
    # starts_from searches from the first of the ODD_TAIL equal starts (the start before them is the tile's first end) at from + 0, 1, 3,
    # 7, ...: it steps over offsets[n_records], whose own value only the search between the last two steps finds
    assert counts[-1] == 1 and counts[-2] == I.ODD_TAIL and values[-3] == 5 * T and I.ODD_TAIL not in [2 ** i - 1 for i in range(8)]
    for order in (MM.LEX, MM.HASH):
        ent = MM.entries_of(buf, k, w, MM.PATH_BITS, MM.PRE_NONE, order)
        per_tile = np.bincount(ent.end // T, minlength=I.ODD_TILES)
        assert per_tile[runs[0] // T] > 0 and runs[0] % T in range(T // 4, 3 * T // 4), "a run in the middle of a tile with entries"
        assert per_tile[runs[1] // T] == 0 and per_tile[runs[1] // T + 1] == 0 and per_tile[runs[1] // T + 2] > 0, "a run in tiles without entries"
        assert (ent.end[ent.end > runs[0]] // T == runs[0] // T).any() and (ent.end[ent.end < runs[0]] // T == runs[0] // T).any()
        out, pos, _, _, _ = MM.csr(ent, off, len(buf), k)
        assert out[0] > 0 and out[-1] < len(ent), "entries in front of offsets[0] and behind offsets[n_records]: outside every range"
        assert np.all(np.diff(out.astype(np.int64)) >= 0) and int(pos.max()) < 2 * T   # no start inside a window: no pos wraps
        assert (ent.end >= int(values[-1])).any() and ((ent.end >= int(values[-2])) & (ent.end < int(values[-1]))).any()


def test_iupac_records_hold_what_the_two_pre_steps_differ_on():
    k, w = I.IUPAC_KW
    recs = I.iupac_records()
    text = b"".join(recs)
    assert set(b"RYKMSWBDHVN") & set(text) and set(b"rykmswbdhvn") & set(text) and b"U" in text and b"u" in text and not set(b"\r\n \t") & set(text)
    assert {p for _, p in I.IUPAC_PATH_PRES} == {MM.PRE_STRIP_RETURNS, MM.PRE_NORMALIZE_IUPAC}
    assert {p for p, pre in I.IUPAC_PATH_PRES if pre == MM.PRE_NORMALIZE_IUPAC} == {MM.PATH_BYTES_CANONICAL, MM.PATH_BITS, MM.PATH_BITS_CANONICAL}
    strip = MM.lists(recs, k, w, MM.PATH_BITS, MM.PRE_STRIP_RETURNS, MM.HASH)
    iupac = MM.lists(recs, k, w, MM.PATH_BITS, MM.PRE_NORMALIZE_IUPAC, MM.HASH)
    assert strip[1].size > 100 and iupac[1].size > 100 and int(iupac[4].sum()) > int(strip[4].sum()), "U is a base for NORMALIZE_IUPAC only"


@pytest.mark.parametrize("cu", [256, 304])
def test_carry_batch_puts_skipped_tiles_and_runs_of_starts_inside_one_blocks_tiles(cu):
    """ml_scatter_kernel: `per = ceil(tiles / gridDim.x)` consecutive tiles a block, the starts known at the end of one tile carried to
    the next, a tile without entries skipped.  At a capped grid of cu * ML_BLOCKS_PER_CU blocks the batch has per = 3, and the tiles of
    each of its three blocks are the same block's."""
    k, w = I.CARRY_KW
    grid, T = cu * MM.BLOCKS_PER_CU, MM.TILE
    sp, blocks = I.carry_batch(grid)
    n_tiles = sp.n_bytes // T
    assert sp.n_bytes % T == 0 and n_tiles > 2 * grid and min(n_tiles, grid) == grid
    per = -(-n_tiles // grid)   # `per` of the kernel at gridDim.x = grid_for(own_tiles, 1, resident) = grid
    assert per == 3
    scatter = open(I.MM.__file__.replace("_minimizer_list_model.py", "../needletail_amd/csrc/ntk_minimizer_list.hip")).read()
    assert "const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x, t_begin = blockIdx.x * per" in scatter
    assert "if (a.tile_base[t + 1] == a.tile_base[t]) continue;" in scatter and "uint64_t j_hi = 0;" in scatter
    s = sp.offsets.astype(np.int64)
    assert np.all(np.diff(s) >= 0) and s[-1] == sp.n_bytes and s.size - 1 > 2 * I.CARRY_RUN
    for order in (MM.LEX, MM.HASH):
        ent = sp.entries(k, w, MM.PATH_BITS, MM.PRE_NONE, order)
        per_tile = np.bincount(ent.end // T, minlength=n_tiles)
        in_tile = lambda t: int(((s >= t * T) & (s < (t + 1) * T)).sum())   # noqa: E731
        for name, t in blocks.items():
            assert t % per == 0 and {x // per for x in (t, t + 1, t + 2)} == {t // per}, (name, "one block's three tiles")
        t = blocks["early"]   # the run lies in a tile with entries, at a record start, and the block's next tile has entries
        assert per_tile[t] > 0 and per_tile[t + 1] > 0 and per_tile[t + 2] == 0 and in_tile(t) > I.CARRY_RUN
        run = np.flatnonzero(np.bincount(s[(s >= t * T) & (s < (t + 1) * T)] - t * T) >= I.CARRY_RUN)
        assert run.size == 1 and T // 4 < run[0] < 3 * T // 4 and sp.buf()[t * T + run[0] - 1] == ord("\n")
        assert ((ent.end // T == t) & (ent.end > t * T + run[0])).any() and ((ent.end // T == t) & (ent.end < t * T + run[0])).any()
        t = blocks["mid"]     # entries, none (the run of equal starts is there), entries: the skipped tile and the next one are one block's
        assert per_tile[t] > 0 and per_tile[t + 1] == 0 and per_tile[t + 2] > 0 and in_tile(t + 1) == I.CARRY_RUN
        assert int((s < t * T).sum()) > I.CARRY_RUN, "many starts behind the block"
        t = blocks["late"]    # none, none, entries: nothing is known when the third tile is reached
        assert per_tile[t] == 0 and per_tile[t + 1] == 0 and per_tile[t + 2] > 0 and in_tile(t + 1) == 100
        assert int((s <= (t + 2) * T).sum()) > 2 * I.CARRY_RUN
        want = MM.csr(ent, sp.offsets, sp.n_bytes, k)
        assert want[0][-1] == len(ent) and int(want[1].max()) <= 200 - k, "every pos is inside its record of at most 200 bases"
