"""The Sequence-trait entry points (the compat face of the C ABI) at the sizes where their kernels take a second level, against the CPU
oracle, bit for bit: the block scan of normalize / strip_returns past 1024 blocks, the grid-stride loop of reverse_complement /
quality_mask past grid_for's cap, the carry of cp_scan_kernel past 1024 blocks of 16 384 positions, the planes kernels with several tiles
per block, and sequence::minimizer with hundreds of candidates per thread and several long records in one chunk.  The inputs come from
tests/_compat_scale.py; tests/test_compat_scale_inputs.py proves without a GPU that each is past its threshold.  Every expectation is the
oracle's (oracle/, tests/_refs.py), never another device call; every comparison is `==` or array_equal.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
from needletail_amd import _lib as NL  # noqa: E402
import _compat_scale as S  # noqa: E402
from _refs import minimizer_with_position  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()   # (the scratch of the 2^28-byte calls and the banks of the 17 MB chunks go with it)


@pytest.fixture
def restore_options(ctx):
    yield
    for o in (NL.OPT_COMPAT_CHUNK_BYTES, NL.OPT_MINIMIZER_CHUNK_BYTES, NL.OPT_MINIMIZER_ROUTE, NL.OPT_COMPAT_PACK_THREADS):
        ctx.set_option(o, 0)


# ---- (a) normalize / strip_returns across the block-scan split -------------------------------------------------------------------------

@pytest.mark.parametrize("n", S.COMPACT_SIZES)
def test_normalize_and_strip_returns_across_the_block_scan_split(ctx, n):
    """compact_scan_kernel with 1024 blocks (one per thread), 1025 (per = 2) and per = 3: every thread sums and re-walks several blocks;
    blocks that keep nothing on both sides of the split."""
    seq = S.compact_input_a(n)
    for iupac in (False, True):
        want, want_changed = O.normalize(seq, iupac)
        got, changed = nt.normalize_opt(seq, iupac, ctx)
        assert changed == want_changed, (n, iupac)
        S.assert_same(got, want, f"normalize n={n} iupac={iupac} (output index)")
    want, borrowed = O.strip_returns(seq)
    assert not borrowed
    S.assert_same(nt.strip_returns(seq, ctx), want, f"strip_returns n={n} (output index)")


def test_clean_input_is_borrowed_across_the_block_scan_split(ctx):
    clean = S.compact_input_b()
    for iupac in (False, True):
        got, changed = nt.normalize_opt(clean, iupac, ctx)
        assert changed is False and got == clean
        assert nt.normalize(clean, iupac, ctx) is clean
    assert nt.strip_returns(clean, ctx) is clean


# ---- (b) reverse_complement / quality_mask past the grid cap ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def grid_inputs():
    return S.grid_inputs()


def test_reverse_complement_past_the_grid_cap(ctx, grid_inputs):
    seq = grid_inputs[0]
    S.assert_same(nt.reverse_complement(seq, ctx), O.reverse_complement(seq), "reverse_complement", 256, "thread block")


def test_quality_mask_past_the_grid_cap(ctx, grid_inputs):
    seq, qual = grid_inputs
    S.assert_same(nt.quality_mask(seq, qual, S.QUALITY_SCORE, ctx), O.quality_mask(seq, qual, S.QUALITY_SCORE), "quality_mask", 256, "thread block")


# ---- (c) item arrays across the cp_scan_kernel carry -------------------------------------------------------------------------------------

class CpCase:
    """The record of more than 16 Mi bases and the oracle's items for it, computed once."""
    def __init__(self):
        self.record = S.cp_record()
        self.bit21 = O.bit_kmers_arrays(self.record, 21, True)
        self.bit32 = O.bit_kmers_arrays(self.record, 32, False)
        self.can33 = O.canonical_kmers_arrays(self.record, O.reverse_complement(self.record), 33)


@pytest.fixture(scope="module")
def cp():
    return CpCase()


def _assert_items(got, want, what, shift=0):
    """Item arrays (pos, [val,] flag) equal; the first difference is named with the cp block the item's plane position lies in."""
    assert len(got) == len(want)
    assert len(got[0]) == len(want[0]), (what, "item count", len(got[0]), len(want[0]))
    for name, g, w in zip(("pos", "val", "flag") if len(got) == 3 else ("pos", "flag"), got, want):
        if not np.array_equal(g, w):
            i = S.first_difference(g, w)
            raise AssertionError(f"{what}: {name}[{i}] differs; the oracle's item there starts at {int(want[0][i])} "
                                 f"(cp block {(int(want[0][i]) + shift) // S.CP_BLOCK_POSITIONS})")


def test_item_arrays_of_one_record_across_the_scan_carry(ctx, cp):
    _assert_items(nt.bit_kmers_arrays(cp.record, 21, True, ctx), cp.bit21, "bit_kmers (21, canonical)", 20)
    _assert_items(nt.bit_kmers_arrays(cp.record, 32, False, ctx), cp.bit32, "bit_kmers (32, forward)", 31)
    _assert_items(nt.canonical_kmers_arrays(cp.record, 33, ctx), cp.can33, "canonical_kmers k=33")


def test_capacity_runs_out_behind_the_scan_carry(ctx, cp):
    """ntk_bit_kmers_batch with room for the items of scan tile 0 and 1000 more: NTK_ERR_CAPACITY, the needed count, the record's count,
    and the items that fit."""
    want_pos, want_val, want_flg = cp.bit21
    cap = int((want_pos < S.CP_SPLIT).sum()) + 1000
    assert cap < len(want_pos)
    offs = np.array([0, len(cp.record)], dtype=np.uint64)
    cnt = np.zeros(1, dtype=np.uint64)
    pos, val, flg = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint8)
    tot = C.c_uint64(0)
    rc = NL.lib().ntk_bit_kmers_batch(ctx._h, cp.record, offs.ctypes.data, 1, 21, 1, cnt.ctypes.data, pos.ctypes.data, val.ctypes.data,
                                      flg.ctypes.data, cap, C.byref(tot))
    assert rc == 5                                                    # NTK_ERR_CAPACITY
    assert tot.value == len(want_pos) and int(cnt[0]) == len(want_pos)
    _assert_items((pos, val, flg), (want_pos[:cap], want_val[:cap], want_flg[:cap]), "the first cap items", 20)


def test_batch_with_an_oversize_record_at_the_default_chunk(ctx, cp):
    """[small, the record, small, empty, small]: the record is a chunk of its own between two ordinary chunks."""
    records = S.cp_batch(cp.record)
    want = [cp.bit21 if r is cp.record else O.bit_kmers_arrays(r, 21, True) for r in records]
    counts, pos, val, flg = nt.bit_kmers_batch(records, 21, True, ctx)
    assert counts.tolist() == [len(w[0]) for w in want]
    _assert_items((pos, val, flg), tuple(np.concatenate([w[j] for w in want]) for j in range(3)), "bit_kmers_batch (21, canonical)", 20)
    want = [cp.can33 if r is cp.record else O.canonical_kmers_arrays(r, O.reverse_complement(r), 33) for r in records]
    counts, pos, flg = nt.canonical_kmers_batch(records, 33, ctx)
    assert counts.tolist() == [len(w[0]) for w in want]
    _assert_items((pos, flg), tuple(np.concatenate([w[j] for w in want]) for j in range(2)), "canonical_kmers_batch k=33")


def test_ragged_batch_in_one_chunk_across_the_scan_carry(ctx, restore_options):
    """NTK_OPT_COMPAT_CHUNK_BYTES = 40 MiB: some 10 500 ragged records (0..4000 bytes, mixed case, N, '-') lie in ONE chunk of more than
    1024 cp blocks; record by record against the oracle's iterators."""
    ctx.set_option(NL.OPT_COMPAT_CHUNK_BYTES, S.CP_RAGGED_CHUNK_BYTES)
    records = S.cp_ragged_records()
    assert sum(len(r) + 1 for r in records) <= S.CP_RAGGED_CHUNK_BYTES
    starts = np.cumsum([0] + [len(r) + 1 for r in records])           # packed start of every record (one break byte behind each)

    def check(got_counts, got, want, what):
        want_counts = np.array([len(w[0]) for w in want], dtype=np.uint64)
        if not np.array_equal(got_counts, want_counts):
            r = S.first_difference(got_counts, want_counts)
            raise AssertionError(f"{what}: counts[{r}] = {int(got_counts[r])}, the oracle's {int(want_counts[r])}; the record lies at packed "
                                 f"byte {int(starts[r])} (cp block {int(starts[r]) // S.CP_BLOCK_POSITIONS})")
        flat = tuple(np.concatenate([w[j] for w in want]) for j in range(len(got)))
        assert len(got[0]) == len(flat[0]), (what, "item count", len(got[0]), len(flat[0]))
        for name, g, w in zip(("pos", "val", "flag") if len(got) == 3 else ("pos", "flag"), got, flat):
            if not np.array_equal(g, w):
                i = S.first_difference(g, w)
                r = int(np.searchsorted(np.cumsum(want_counts), i, side="right"))
                raise AssertionError(f"{what}: {name}[{i}] differs, in record {r} at packed byte {int(starts[r])} "
                                     f"(cp block {int(starts[r]) // S.CP_BLOCK_POSITIONS})")

    counts, pos, val, flg = nt.bit_kmers_batch(records, 21, True, ctx)
    check(counts, (pos, val, flg), [O.bit_kmers_arrays(r, 21, True) for r in records], "bit_kmers_batch (21, canonical)")
    counts, pos, flg = nt.canonical_kmers_batch(records, 21, ctx)
    check(counts, (pos, flg), [O.canonical_kmers_arrays(r, O.reverse_complement(r), 21) for r in records], "canonical_kmers_batch k=21")


# ---- (d) planes with several tiles per block ----------------------------------------------------------------------------------------------

def _assert_planes(pl, records, items, what, with_values):
    """One chunk: rec_bit is the records' byte offsets; planes and values against the oracle's per-record arrays placed there."""
    offs = np.zeros(len(records) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in records], out=offs[1:])
    n_words = (int(offs[-1]) + 15) // 16
    assert len(pl.valid16) == len(pl.rc16) == n_words, what
    rec_bit = offs.copy()
    rec_bit[-1] = 16 * n_words
    assert np.array_equal(pl.rec_bit, rec_bit), what
    assert pl.total == sum(len(it[0]) for it in items), (what, "total", pl.total, sum(len(it[0]) for it in items))
    v16, r16, vals = S.expected_planes(offs, n_words, items, with_values)
    S.assert_same(pl.valid16, v16, what + ": valid16 (word index)", S.PL_TILE // 16, "tile")
    S.assert_same(pl.rc16, r16, what + ": rc16 (word index)", S.PL_TILE // 16, "tile")
    assert not (pl.rc16 & ~pl.valid16).any(), what
    if with_values:
        S.assert_same(pl.values, vals, what + ": values (plane position)", S.PL_TILE, "tile")   # (the emitted values, and 0 everywhere else)


def test_planes_with_several_tiles_per_block(ctx, restore_options):
    """Every block of the n_cu * 8 grid takes a second tile (LDS re-used behind the top-of-loop barrier, the block's count carried across
    tiles), a few take a third; records begin on, before and behind tile boundaries."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    records = S.planes_records(cu)
    total = sum(len(r) for r in records)
    assert total >= S.planes_min_bytes(cu) and (total + S.PL_TILE - 1) // S.PL_TILE >= 2 * cu * S.PL_BLOCKS_PER_CU + 3
    if total > S.DEFAULT_CHUNK_BYTES:
        ctx.set_option(NL.OPT_COMPAT_CHUNK_BYTES, total)
    assert total <= ctx.get_option(NL.OPT_COMPAT_CHUNK_BYTES)         # one chunk
    rcs = [O.reverse_complement(r) for r in records]
    for k in (21, 70):
        pl = nt.canonical_kmers_planes(records, k, ctx)
        _assert_planes(pl, records, [O.canonical_kmers_arrays(r, rc, k) for r, rc in zip(records, rcs)], f"canonical_kmers_planes k={k}", False)
    for k, canonical in ((21, True), (32, False)):
        pl = nt.bit_kmers_planes(records, k, canonical, ctx, values=True)
        _assert_planes(pl, records, [O.bit_kmers_arrays(r, k, canonical) for r in records], f"bit_kmers_planes ({k}, {canonical})", True)


def test_planes_of_the_oversize_record(ctx, cp):
    """The record of (c) through both planes faces: some 8 200 tiles, four per block at 256 CUs."""
    _assert_planes(nt.canonical_kmers_planes([cp.record], 33, ctx), [cp.record], [cp.can33], "canonical_kmers_planes k=33, one record", False)
    _assert_planes(nt.bit_kmers_planes([cp.record], 21, True, ctx, values=True), [cp.record], [cp.bit21], "bit_kmers_planes (21, canonical), one record", True)
    _assert_planes(nt.bit_kmers_planes([cp.record], 32, False, ctx, values=True), [cp.record], [cp.bit32], "bit_kmers_planes (32, forward), one record", True)


# ---- (e) minimizer at size ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def minimizer_inputs():
    return S.minimizer_inputs()


@pytest.mark.parametrize("name", ["random", "homopolymer", "AT", "ACGT", "inverted_repeat"])
def test_minimizer_of_a_long_sequence(ctx, minimizer_inputs, name):
    """minimizer_bytes_kernel with some 500 candidates per thread; on all but `random`, equal candidates in different threads and waves
    (the bytes are equal whichever wins, so a wrong pick among them cannot show here: the batch test below checks start and strand)."""
    seq = minimizer_inputs[name]
    for m in S.MINIMIZER_LENGTHS:
        assert nt.minimizer(seq, m, ctx) == O.minimizer(seq, m), (name, m)


def test_minimizer_batch_around_the_long_record_threshold(ctx):
    """65 535 / 65 536 bytes through the wave kernel, 65 537 / 200 000 / 70 000 through the one-block kernel, all in one chunk (the long
    records share one d_best); bytes, window start and strand as the reference's loop order decides them."""
    records = S.minimizer_batch_records()
    m = S.MINIMIZER_BATCH_LENGTH
    mins, pos, flg = nt.minimizer_batch(records, m, ctx, with_positions=True)
    for r, rec in enumerate(records):
        want = minimizer_with_position(rec, m)
        assert want[0] == O.minimizer(rec, m)
        assert (mins[r], int(pos[r]), int(flg[r])) == want, (r, len(rec))
