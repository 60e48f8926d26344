"""Per-read k-mer abundance (include/needletail_amd_abundance.h, needletail_amd.ReadAbundance) on a real MI355X.

Truth for every row: tests/_abundance_model.py on the oracle's literal iterators - the table is `oracle_items` of the batch that was
counted, a record's k-mers are `oracle_values(record + b"\\n")`, each looked up in those items.  Every comparison is
`np.array_equal` on the whole (n_records, 6) array; there is no tolerance anywhere."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import abundance  # noqa: E402
import _abundance_model as A  # noqa: E402
import _count_model as CM  # noqa: E402
from _count_helpers import CUTOFF, PATH_PRES, oracle_items, oracle_values, pack, quality_masked, random_records, upload  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (1, 5, 16, 21, 31, 32)
MIN_COUNTS = (0, 1, 3)
BYTES, BITS, BITS_CANON = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS, nt.PATH_BITS_CANONICAL
REG_WINDOWS, LONG_RECORD = 192, 65536   # ntk_abundance.hip kRegWindows, kLongRecord (tests/test_abundance_abi.py ties them)
ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 2, 5, 6
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def dev_offsets(off):
    t = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def run(ra, dev, n_bytes, off, pre, **kw) -> np.ndarray:
    rows = ra.run_device(dev, n_bytes, dev_offsets(off), len(off) - 1, pre, **kw)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (len(off) - 1, 6) and rows.is_cuda
    return rows.cpu().numpy().view(np.uint64)


def counted(ctx, k, path, pre, records, **kw):
    """A table that counted the records, and the oracle's items of the same batch."""
    buf = pack(records)
    t = nt.KmerTable(k, path, max(len(buf), 16), ctx)
    dev = upload(buf)
    t.count_device(dev, len(buf), pre, **kw)
    ctx.synchronize()
    return t, oracle_items(buf, k, path, pre)


def assert_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, what
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError((what, f"{bad.size} rows differ, first {int(bad[0])}", got[bad[0]].tolist(), want[bad[0]].tolist()))


# ---- 1. exact against the oracle -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [7, 0xAB0017])
def test_random_records_match_the_oracle(ctx, seed):
    """Every (path, pre) x k, the table counted from the same records and from every second record (absent k-mers), min_count 0, 1, 3."""
    recs = random_records(seed)
    buf, off = pack(recs), A.offsets(recs)
    dev = upload(buf)
    seen_absent = 0
    for path, pre in PATH_PRES:
        for k in KS:
            values = [A.record_values(r, k, path, pre) for r in recs]
            for tab in (recs, recs[::2]):
                t, items = counted(ctx, k, path, pre, tab)
                with t, nt.ReadAbundance(t) as ra:
                    for mc in MIN_COUNTS:
                        want = A.rows_from_values(values, items, mc)
                        assert_rows(run(ra, dev, len(buf), off, pre, min_count=mc), want, (seed, path, pre, k, len(tab), mc))
                    if tab is not recs:
                        seen_absent += int(((want[:, 1] < want[:, 0]) & (want[:, 2] == 0)).sum())
                    elif k == 21:   # the packer's route: the same records through ntk_batch_append, offsets from the packer
                        assert_rows(ra.run_records(recs, pre, min_count=3), A.rows_from_values(values, items, 3), ("records", path, pre))
    assert seen_absent > 1000


@functools.lru_cache(maxsize=None)
def genome_sampled_reads(seed=11, genome_len=20_000, n_reads=4_000):
    """Reads of 30..299 bases from a random genome: 1 % substitutions, half reverse-complemented, one N in 5 % of them."""
    rng = np.random.default_rng(seed)
    genome = ACGT[rng.integers(0, 4, genome_len)]
    out = []
    for _ in range(n_reads):
        L = int(rng.integers(30, 300))
        s = int(rng.integers(0, genome_len - L + 1))
        r = genome[s:s + L].copy()
        sub = rng.random(L) < 0.01
        r[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
        if rng.random() < 0.5:
            r = COMP[r[::-1]]
        if rng.random() < 0.05:
            r[int(rng.integers(0, L))] = ord("N")
        out.append(r.tobytes())
    return tuple(out)


@pytest.mark.parametrize("k,path,pre", [(21, BYTES, nt.PRE_NORMALIZE), (31, BITS_CANON, nt.PRE_NONE)])
def test_genome_sampled_reads_have_statistics_that_differ(ctx, k, path, pre):
    """~33x coverage with errors, min_count 3: the oracle's own rows must tell min, median and max apart in at least half the records
    and have absent or rare k-mers in at least a quarter, before the library's rows are held to them."""
    recs = list(genome_sampled_reads())
    t, items = counted(ctx, k, path, pre, recs)
    want = A.rows(recs, items, k, path, pre, 3)
    apart = int(((want[:, 2] < want[:, 3]) & (want[:, 3] < want[:, 4])).sum())
    rare = int((want[:, 1] < want[:, 0]).sum())
    print(f"k = {k}: min < median < max in {apart}, n_present < n_kmers in {rare} of {len(recs)} records")
    assert apart >= len(recs) // 2 and rare >= len(recs) // 4
    buf = pack(recs)
    with t, nt.ReadAbundance(t) as ra:
        assert_rows(run(ra, upload(buf), len(buf), A.offsets(recs), pre, min_count=3), want, (k, path))


def test_foreign_reads_are_absent(ctx):
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    t, items = counted(ctx, k, path, pre, list(genome_sampled_reads()))
    rng = np.random.default_rng(12)
    foreign = [ACGT[rng.integers(0, 4, 150)].tobytes() for _ in range(500)]
    want = A.rows(foreign, items, k, path, pre)
    assert (want[:, 0] == 130).all() and not want[:, [1, 3, 4]].any()
    buf = pack(foreign)
    with t, nt.ReadAbundance(t) as ra:
        assert_rows(run(ra, upload(buf), len(buf), A.offsets(foreign), pre), want, "foreign")


def test_quality_stream_masks_as_the_table_does(ctx):
    recs = random_records(0xAB0021)
    buf, off = pack(recs), A.offsets(recs)
    rng = np.random.default_rng(9)
    qual = rng.integers(33, 75, len(buf)).astype(np.uint8)
    quals = [qual[int(off[i]): int(off[i + 1]) - 1] for i in range(len(recs))]
    dev, dq, masked = upload(buf), upload(qual.tobytes(), fill=0xFF), quality_masked(buf, qual)
    for path, pre, k in ((BYTES, nt.PRE_NORMALIZE, 21), (BITS, nt.PRE_NONE, 5), (BITS_CANON, nt.PRE_STRIP_RETURNS, 32), (BYTES, nt.PRE_NORMALIZE_IUPAC, 16)):
        items = oracle_items(masked, k, path, pre)
        plain = oracle_items(buf, k, path, pre)
        with nt.KmerTable(k, path, len(buf), ctx) as t, nt.ReadAbundance(t) as ra:
            t.count_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=CUTOFF)
            want = A.rows(recs, items, k, path, pre, 1, quals, CUTOFF)
            assert_rows(run(ra, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=CUTOFF), want, ("quality", path, k))
            # cutoff 0 or no stream: no mask on the read side (the table still holds the masked counts)
            unmasked = A.rows(recs, items, k, path, pre)
            assert not np.array_equal(unmasked, want)
            assert_rows(run(ra, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=0), unmasked, ("cutoff 0", path, k))
            assert_rows(run(ra, dev, len(buf), off, pre), unmasked, ("no stream", path, k))
            # masked reads against the unmasked table
            t.reset()
            t.count_device(dev, len(buf), pre)
            assert_rows(run(ra, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=CUTOFF),
                        A.rows(recs, plain, k, path, pre, 1, quals, CUTOFF), ("masked reads", path, k))


def _golden_records(name):
    return [r.raw_seq for r in nt.parse_fastx_file(os.path.join(GOLDEN, name))]


def _packed(ctx, recs, pre):
    """The packer's bytes and offsets of the records."""
    b = nt.Batch(ctx, sum(len(r) for r in recs) + len(recs), len(recs))
    for r in recs:
        assert b.append(r, pre)
    seq, off = b.buffers()
    out = seq.tobytes(), np.array(off, copy=True)
    b.release()
    return out


def test_golden_28s_and_prjna271013(ctx):
    for name in ("28S.fasta", "PRJNA271013_head.fq"):
        recs = _golden_records(name)
        for k, path, pre in ((21, BYTES, nt.PRE_NORMALIZE), (4, BYTES, nt.PRE_NORMALIZE), (31, BITS_CANON, nt.PRE_STRIP_RETURNS)):
            buf, off = _packed(ctx, recs, pre)
            packed = [buf[int(off[i]): int(off[i + 1]) - 1] for i in range(len(recs))]   # what the packer made of each record
            assert pack(packed) == buf
            items = oracle_items(buf, k, path, pre)
            want = A.rows(packed, items, k, path, pre, 2)
            assert want[:, 0].sum() > 1000
            with nt.KmerTable(k, path, len(buf), ctx) as t, nt.ReadAbundance(t) as ra:
                t.count_records(recs, pre)
                assert_rows(ra.run_records(recs, pre, min_count=2), want, (name, k, path))


# ---- 2. geometry ---------------------------------------------------------------------------------------------------------------------

def _genome(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)]


def _periodic(genome, start, n):
    """n bases of the genome read round and round from `start`."""
    reps = (start + n) // genome.size + 1
    return np.tile(genome, reps)[start:start + n].tobytes()


def _coverage_reads(genome, seed, n_reads):
    """Short error-free reads of the circular genome at uneven depth: counts that differ along it."""
    rng = np.random.default_rng(seed)
    return [_periodic(genome, int(rng.integers(0, genome.size) ** 2 // genome.size), int(rng.integers(40, 200))) for _ in range(n_reads)]


@pytest.mark.parametrize("k", [1, 5, 21, 32])
def test_records_of_every_short_length(ctx, k):
    """Records of 0 .. k + 2 bases (none, one, two, three k-mers), each length several times, with and without an N."""
    genome = _genome(0x60 + k, 64)
    rng = np.random.default_rng(k)
    recs = []
    for L in list(range(0, k + 3)) * 3:
        r = bytearray(_periodic(genome, int(rng.integers(0, 64)), L))
        if L and rng.random() < 0.3:
            r[int(rng.integers(0, L))] = ord("N")
        recs.append(bytes(r))
    buf = pack(recs)
    for path, pre in ((BYTES, nt.PRE_NORMALIZE), (BITS, nt.PRE_NONE), (BITS_CANON, nt.PRE_NORMALIZE)):
        t, items = counted(ctx, k, path, pre, recs)
        want = A.rows(recs, items, k, path, pre)
        assert {0, 1, 2, 3} <= set(want[:, 0].tolist())
        with t, nt.ReadAbundance(t) as ra:
            assert_rows(run(ra, upload(buf), len(buf), A.offsets(recs), pre), want, (k, path))
    empty = [b""] * 5   # a batch of break bytes only
    with nt.KmerTable(k, BITS, 16, ctx) as t, nt.ReadAbundance(t) as ra:
        got = run(ra, upload(pack(empty)), 5, A.offsets(empty), nt.PRE_NONE)
        assert got.shape == (5, 6) and not got.any()


@pytest.mark.parametrize("k,path,pre", [(21, BYTES, nt.PRE_NORMALIZE), (1, BITS, nt.PRE_NONE), (32, BITS_CANON, nt.PRE_NONE)])
def test_window_counts_at_the_lane_and_register_seams(ctx, k, path, pre):
    """Records with exactly 63, 64, 65, 127, 128, 129, 191, 192, 193 (and a few more) windows: whole and partial rounds of the wave, and the
    last record the wave holds in registers; each as pure bases, and with one N that invalidates k windows in the middle."""
    genome = _genome(0x70, 300)
    table_reads = _coverage_reads(genome, 0x71, 120)
    rng = np.random.default_rng(0x72)
    recs = []
    for w in (1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130, 190, 191, REG_WINDOWS, 193, 194, 255, 256, 257, 383, 384, 385, 449):
        r = _periodic(genome, int(rng.integers(0, 300)), w + k - 1)
        recs.append(r)
        if w > 2 * k:
            holed = bytearray(r)
            holed[len(r) // 2] = ord("N")
            recs.append(bytes(holed))
    t, items = counted(ctx, k, path, pre, table_reads)
    want = A.rows(recs, items, k, path, pre, 3)
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193} <= set(want[:, 0].tolist())
    if k > 1:
        assert int((want[:, 2] < want[:, 3]).sum()) > 5 and int((want[:, 3] < want[:, 4]).sum()) > 5
    buf = pack(recs)
    with t, nt.ReadAbundance(t) as ra:
        assert_rows(run(ra, upload(buf), len(buf), A.offsets(recs), pre, min_count=3), want, (k, path))


def test_long_records_on_both_sides_of_the_threshold(ctx):
    """One record with exactly LONG_RECORD windows (the last the wave kernel takes), one with LONG_RECORD + 1 (the first of
    ra_block_kernel) and one of 300 000 bases, each a 2 000-base genome read round and round, among short reads; the table holds short
    reads of that genome at uneven depth, so min < median < max in the long rows."""
    genome = _genome(0x80, 2000)
    table_reads = _coverage_reads(genome, 0x81, 600)
    short = _coverage_reads(genome, 0x82, 40)
    for k, path, pre in ((21, BYTES, nt.PRE_NORMALIZE), (31, BITS_CANON, nt.PRE_NONE)):
        longs = [_periodic(genome, 5, LONG_RECORD + k - 1), _periodic(genome, 700, LONG_RECORD + k), _periodic(genome, 1500, 300_000),
                 _periodic(genome, 0, LONG_RECORD - 1 + k - 1), b"N" * (LONG_RECORD + 500)]
        recs = short[:10] + [longs[0]] + short[10:20] + [longs[1], longs[2]] + short[20:30] + [longs[3], longs[4]] + short[30:]
        t, items = counted(ctx, k, path, pre, table_reads)
        want = A.rows(recs, items, k, path, pre, 2)
        by_len = {int(r[0]): r for r in want}
        assert {LONG_RECORD - 1, LONG_RECORD, LONG_RECORD + 1, 300_000 - k + 1} <= set(by_len)
        for n in (LONG_RECORD, LONG_RECORD + 1, 300_000 - k + 1):
            assert by_len[n][2] < by_len[n][3] < by_len[n][4], by_len[n]
        buf = pack(recs)
        with t, nt.ReadAbundance(t) as ra:
            assert_rows(run(ra, upload(buf), len(buf), A.offsets(recs), pre, min_count=2), want, (k, path))


def test_a_record_longer_than_a_chunk(ctx):
    """A single record of 75.5 M bases (more than the 64 MiB chunk, the size of test_chunk_boundaries_are_counted_once's batch) between short
    records: a 2 000-base genome read round and round, so a window's value repeats with the period and the oracle's values of one
    period (`oracle_values` of the first period + k - 1 bases) stand for every window; `weighted_row` weighs each by how often the
    record reaches it."""
    genome = _genome(0x90, 2000)
    P, L = genome.size, 500_000 * 151
    assert L > CM.CHUNK
    table_reads = _coverage_reads(genome, 0x91, 600)
    before, after = _coverage_reads(genome, 0x92, 30), _coverage_reads(genome, 0x93, 30)
    head, tail = pack(before), pack(after)
    n_bytes = len(head) + L + 1 + len(tail)
    dev = torch.full(((n_bytes + 15) // 16 * 16 + 64,), ord("\n"), dtype=torch.uint8, device="cuda")
    dev[:len(head)] = torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).cuda()
    dev[len(head):len(head) + L] = torch.from_numpy(genome.copy()).cuda().repeat(L // P + 1)[:L]
    dev[len(head) + L + 1:n_bytes] = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    off = np.concatenate([A.offsets(before), len(head) + L + 1 + A.offsets(after)]).astype(np.uint64)
    assert off[-1] == n_bytes and len(off) == 62
    for k, path, pre in ((21, BYTES, nt.PRE_NORMALIZE), (32, BITS, nt.PRE_NONE)):
        t, items = counted(ctx, k, path, pre, table_reads)
        period = oracle_values(_periodic(genome, 0, P + k - 1) + b"\n", k, path, pre)   # windows ending at k - 1 .. P + k - 2
        assert period.size == P
        again = oracle_values(_periodic(genome, 0, 2 * P + k - 1) + b"\n", k, path, pre)
        assert np.array_equal(again[:P], period) and np.array_equal(again[P:], period)   # the period, checked on the oracle itself
        windows = L - k + 1
        weights = np.full(P, windows // P) + (np.arange(P) < windows % P)
        big = A.weighted_row(A.lookup(period, items), weights, 2)
        assert big[0] == windows and big[2] < big[3] < big[4]
        want = np.vstack([A.rows(before, items, k, path, pre, 2), big[None, :], A.rows(after, items, k, path, pre, 2)])
        with t, nt.ReadAbundance(t) as ra:
            assert_rows(run(ra, dev, n_bytes, off, pre, min_count=2), want, (k, path))
    del dev
    torch.cuda.empty_cache()


SEAMS = (CM.CHUNK, 2 * CM.CHUNK, 3 * CM.CHUNK)
SEAM_KS = (1, 17, 18, 32)   # halos 0, 16 (17 fits it exactly, 18 is one over) and 32
SEAM_MODES = ((BYTES, nt.PRE_NORMALIZE), (BITS, nt.PRE_NONE))


class SeamLayout:
    """One device batch that is filler except for small regions of records around the chunk seams.  The filler between two regions
    is one giant record of N (its last byte a break byte): the oracle's row of it is all-zero without walking it, and a record with
    no k-mer at all goes through the long-record path."""

    def __init__(self, n_bytes):
        self.n_bytes = n_bytes
        self.dev = torch.empty(((n_bytes + 15) // 16 * 16 + 64,), dtype=torch.uint8, device="cuda")

    def lay(self, placed):
        """placed: (start, [records]) ascending.  Returns (all region records, the batch's offsets, the index of each region record)."""
        self.dev.fill_(ord("N"))
        self.dev[self.n_bytes - 1:] = ord("\n")
        offs, where, recs, end = [0], [], [], 0
        for start, region in placed:
            reg = pack(region)
            assert start > end + 1 and start + len(reg) < self.n_bytes - 1
            self.dev[start - 1] = ord("\n")          # the filler's break byte
            self.dev[start:start + len(reg)] = torch.from_numpy(np.frombuffer(reg, dtype=np.uint8).copy()).cuda()
            offs.append(start)                       # the filler record [end, start)
            for r in region:
                where.append(len(offs) - 1)
                offs.append(offs[-1] + len(r) + 1)
                recs.append(r)
            end = start + len(reg)
        offs.append(self.n_bytes)                    # the last filler
        torch.cuda.synchronize()
        return recs, np.array(offs, dtype=np.uint64), np.array(where)


def _around_seam(seed, rec, offset, seam):
    """Random records, then `rec` so that `seam` falls on its byte `offset` (offset len(rec): on its break byte), then random records."""
    before, after = random_records(seed, 5), random_records(seed + 1, 5)
    return seam - len(pack(before)) - offset, before + [rec] + after


def _check_seam_layout(ctx, layout, placed, ks, what):
    recs, off, where = layout.lay(placed)
    for path, pre in SEAM_MODES:
        for k in ks:
            items = oracle_items(pack(recs), k, path, pre)
            want = np.zeros((len(off) - 1, 6), dtype=np.uint64)   # the fillers: records of N
            want[where] = A.rows(recs, items, k, path, pre)
            with nt.KmerTable(k, path, 1 << 15, ctx) as t, nt.ReadAbundance(t) as ra:
                t.count_device(layout.dev, layout.n_bytes, pre)
                assert_rows(run(ra, layout.dev, layout.n_bytes, off, pre), want, (what, path, k))


def test_chunk_seams_row_by_row(ctx):
    """Seams at 64, 128 and 192 MiB, each falling on byte 0..33 of a short record (every k's halo, the exact fit of k = 17 and one byte
    over it), on the break byte after a record of exactly k bases, on that record's last base, and on the first base of a record of
    exactly k bases: the record whose windows come from two chunks has the oracle's row, and so have its neighbours."""
    layout = SeamLayout(SEAMS[-1] + 8192)
    rng = np.random.default_rng(0x5EAC)
    bases = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()   # noqa: E731
    offsets = list(range(34))
    for g in range(0, len(offsets), len(SEAMS)):
        placed = [_around_seam(1000 * g + 10 * i, bases(int(rng.integers(40, 64))), o, s)
                  for i, (o, s) in enumerate(zip(offsets[g:g + len(SEAMS)], SEAMS))]
        _check_seam_layout(ctx, layout, placed, SEAM_KS, ("offsets", offsets[g:g + len(SEAMS)]))
    for k in SEAM_KS:
        placed = [_around_seam(7000 + k, bases(k), k, SEAMS[0]),        # ends at seam - 1: the seam is on its break byte
                  _around_seam(7100 + k, bases(k), k - 1, SEAMS[1]),    # ends at the seam
                  _around_seam(7200 + k, bases(k), 0, SEAMS[2])]        # starts at the seam, after a break byte
        _check_seam_layout(ctx, layout, placed, (k,), ("k-base records", k))
    del layout
    torch.cuda.empty_cache()


# ---- 3. counts far above the record's length, order, reuse -----------------------------------------------------------------------------

def test_hot_table_slot(ctx):
    """A record of 5 000 A against a table that counted 2^20 A: every count is 2^20 - k + 1, far above the record's length."""
    hot = b"A" * (1 << 20)
    recs = [b"A" * 5000, b"ACGT" * 30, b"A" * 100 + b"C" + b"A" * 100]
    for k, path, pre in ((21, BYTES, nt.PRE_NORMALIZE), (32, BITS, nt.PRE_NONE)):
        t, items = counted(ctx, k, path, pre, [hot])
        want = A.rows(recs, items, k, path, pre)
        c = (1 << 20) - k + 1
        assert want[0].tolist() == [5000 - k + 1, 5000 - k + 1, c, c, c, (5000 - k + 1) * c]
        assert want[2][2] == 0 and want[2][4] == c
        with t, nt.ReadAbundance(t) as ra:
            assert_rows(run(ra, upload(pack(recs)), len(pack(recs)), A.offsets(recs), pre), want, (k, path))


def test_rows_follow_the_records_when_shuffled(ctx):
    recs = list(genome_sampled_reads())[:1500] + [_periodic(_genome(0xA0, 1000), 0, 150_000)]
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    t, _ = counted(ctx, k, path, pre, recs)
    order = np.random.default_rng(0xA1).permutation(len(recs))
    shuffled = [recs[i] for i in order]
    with t, nt.ReadAbundance(t) as ra:
        a = run(ra, upload(pack(recs)), len(pack(recs)), A.offsets(recs), pre, min_count=3)
        b = run(ra, upload(pack(shuffled)), len(pack(shuffled)), A.offsets(shuffled), pre, min_count=3)
    assert_rows(b, a[order], "shuffled")
    assert len({tuple(r) for r in a.tolist()}) > 1000


def test_repeated_calls_grow_shrink_and_trim(ctx):
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    reads = list(genome_sampled_reads())
    t, items = counted(ctx, k, path, pre, reads)
    sizes = (50, 4000, 700, 1, 2500)
    want = {n: A.rows(reads[:n], items, k, path, pre, 3) for n in sizes}
    with t, nt.ReadAbundance(t) as ra:
        for trim in (False, True):
            for n in sizes:
                buf = pack(reads[:n])
                assert_rows(run(ra, upload(buf), len(buf), A.offsets(reads[:n]), pre, min_count=3), want[n], (trim, n))
                if trim:
                    ra.trim()
        ra.trim()
        ra.trim()   # nothing left to free
        with nt.ReadAbundance(t) as never_ran:
            never_ran.trim()


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------------

def _status(ra, dev, n_bytes, d_off, n_records, k, path, pre, flags=0, rows=None, min_count=1):
    p = NL.Params(k, path, pre, flags)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    return abundance.lib().ntk_read_abundance_run_device(ra._h, ptr(dev), None, n_bytes, ptr(d_off), n_records, C.byref(p), min_count, ptr(rows))


def test_errors(ctx):
    recs = random_records(0xAB0031, 40)
    buf, off = pack(recs), A.offsets(recs)
    dev, d_off = upload(buf), dev_offsets(off)
    n, pattern = len(recs), 0x5A5A5A5A5A5A5A5A
    rows = torch.full((n, 6), pattern, dtype=torch.int64, device="cuda")
    untouched = lambda: bool((rows == pattern).all())   # noqa: E731
    with nt.KmerTable(21, BITS_CANON, len(buf), ctx) as t, nt.ReadAbundance(t) as ra:
        t.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        args = (ra, dev, len(buf), d_off, n)
        assert _status(*args, 20, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG            # k is not the table's
        assert _status(*args, 33, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG
        assert _status(*args, 21, BITS, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG                  # nor the path
        assert _status(*args, 21, BITS_CANON, nt.PRE_NORMALIZE, flags=5, rows=rows) == ERR_BAD_ARG   # a minimizer window
        assert _status(*args, 21, BITS_CANON, nt.PRE_NORMALIZE, flags=NL.FLAG_RESET, rows=rows) == ERR_BAD_ARG
        assert _status(*args, 21, BITS_CANON, 4, rows=rows) == ERR_BAD_ARG                           # no such pre-step
        assert _status(*args, 21, BITS_CANON, nt.PRE_NORMALIZE, rows=None) == ERR_BAD_ARG            # null pointers, sizes not zero
        assert _status(ra, None, len(buf), d_off, n, 21, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG
        assert _status(ra, dev, len(buf), None, n, 21, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG
        assert untouched()
        # nothing to do: NTK_OK, nothing touched, whatever the pointers
        assert _status(ra, dev, len(buf), d_off, 0, 21, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == 0
        assert _status(ra, None, 0, None, 0, 21, BITS_CANON, nt.PRE_NORMALIZE, rows=None) == 0
        assert _status(ra, dev, 0, d_off, n, 21, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == 0
        assert untouched()
        empty = ra.run_device(dev, len(buf), d_off, 0, nt.PRE_NORMALIZE)
        assert tuple(empty.shape) == (0, 6) and ra.run_records([], nt.PRE_NORMALIZE).shape == (0, 6)
        # and the call that is right
        assert _status(*args, 21, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == 0
        assert_rows(rows.cpu().numpy().view(np.uint64), A.rows(recs, oracle_items(buf, 21, BITS_CANON, nt.PRE_NORMALIZE), 21, BITS_CANON,
                                                               nt.PRE_NORMALIZE), "after the errors")
    lib = abundance.lib()
    h = C.c_void_p()
    with nt.KmerTable(21, BYTES, len(buf), ctx) as t:
        assert lib.ntk_read_abundance_create(None, t._h, C.byref(h)) == ERR_BAD_ARG
        assert lib.ntk_read_abundance_create(ctx._h, None, C.byref(h)) == ERR_BAD_ARG
        assert lib.ntk_read_abundance_create(ctx._h, t._h, None) == ERR_BAD_ARG
        assert lib.ntk_read_abundance_trim(None) == ERR_BAD_ARG
        lib.ntk_read_abundance_destroy(None)
        with nt.ReadAbundance(t) as ra:   # un-normalised byte-path input, as for the table
            rows.fill_(pattern)
            for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):
                assert _status(ra, dev, len(buf), d_off, n, 21, BYTES, pre, rows=rows) == ERR_UNSUPPORTED
            assert untouched()
            with pytest.raises(nt.NtkError) as e:
                ra.run_device(dev, len(buf), d_off, n, nt.PRE_NONE)
            assert e.value.status == ERR_UNSUPPORTED


def test_incomplete_table_writes_no_row(ctx):
    recs = random_records(0xAB0032, 40)
    buf, off = pack(recs), A.offsets(recs)
    dev, d_off = upload(buf), dev_offsets(off)
    pattern = 0x5A5A5A5A5A5A5A5A
    rows = torch.full((len(recs), 6), pattern, dtype=torch.int64, device="cuda")
    with nt.KmerTable(21, BITS_CANON, 1, ctx) as t, nt.ReadAbundance(t) as ra:
        t.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        assert t.stats()["n_dropped"] > 0
        assert _status(ra, dev, len(buf), d_off, len(recs), 21, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == ERR_CAPACITY
        torch.cuda.synchronize()
        assert bool((rows == pattern).all())
        with pytest.raises(nt.NtkError) as e:
            ra.run_records(recs, nt.PRE_NORMALIZE)
        assert e.value.status == ERR_CAPACITY
        t.reset()   # the same handle on the table once it is complete again
        assert not run(ra, dev, len(buf), off, nt.PRE_NORMALIZE)[:, 1:].any()


def test_wide_table_is_refused(ctx):
    with nt.WideKmerTable(40, BYTES, 1000, ctx) as w:
        with pytest.raises(TypeError, match="33..63"):
            nt.ReadAbundance(w)


# ---- 5. the example ---------------------------------------------------------------------------------------------------------------------

def test_read_abundance_cli(ctx, tmp_path):
    exe = os.path.join(ROOT, "examples", "read_abundance")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    reads = list(genome_sampled_reads())[:300] + [b"A", b"ACGT", b"N" * 50]
    names = [f"read{i}" for i in range(len(reads))]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (n.encode(), r, b"I" * len(r)) for n, r in zip(names, reads)))
    rng = np.random.default_rng(0xC1)
    ref = [ACGT[rng.integers(0, 4, 3000)].tobytes(), reads[0] + reads[5] + reads[9]]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">ref%d\n%s\n" % (i, r) for i, r in enumerate(ref)))
    pre = nt.PRE_NORMALIZE
    for k, mc, table, extra in ((21, 1, reads, []), (21, 3, reads, ["-m", "3"]), (15, 1, ref, ["-r", str(fa)]), (15, 2, ref, ["-r", str(fa), "-m", "2"])):
        items = oracle_items(pack(table), k, BYTES, pre)
        want = "".join(A.cli_line(n, row) + "\n" for n, row in zip(names, A.rows(reads, items, k, BYTES, pre, mc)))
        r = subprocess.run([exe, "-k", str(k), *extra, str(fq)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (k, mc, extra)
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 2
