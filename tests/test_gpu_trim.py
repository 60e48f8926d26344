"""Trimming reads by k-mer abundance (include/needletail_amd_trim.h, needletail_amd.ReadTrimmer) on a real MI355X.

Truth for every row and every output byte: tests/_trim_model.py on the oracle's literal iterators - the table is `oracle_items` of the
batch that was counted, a record's windows are the iterators' positions and values, each looked up in those items.  Every comparison
is `np.array_equal` on whole arrays; there is no tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import trimming  # noqa: E402
import _count_model as CM  # noqa: E402
import _trim_model as T  # noqa: E402
from _count_helpers import CUTOFF, PATH_PRES, oracle_items, pack, quality_masked, random_records, upload  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (1, 5, 16, 21, 31, 32)
MIN_COUNTS = (0, 1, 3)
MODES = (T.PREFIX, T.LONGEST)
BYTES, BITS, BITS_CANON = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS, nt.PATH_BITS_CANONICAL
GROUP_WORDS, LONG_PIECES = 32, 2048   # ntk_trim.hip kGroup * kGroupRounds, kLongPieces (tests/test_trim_abi.py ties them)
ROUND = 64 * 64                       # windows a wave takes per round of rt_interval_kernel's long path
ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 2, 5, 6
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def dev_u64(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64) if t.dtype == torch.int64 else t.cpu().numpy()


def run(rt, dev, n_bytes, off, pre, **kw) -> np.ndarray:
    rows = rt.run_device(dev, n_bytes, dev_u64(off), len(off) - 1, pre, **kw)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (len(off) - 1, 4) and rows.is_cuda
    return host(rows)


def counted(ctx, k, path, pre, records, **kw):
    """A table that counted the records, and the oracle's items of the same batch."""
    buf = pack(records)
    t = nt.KmerTable(k, path, max(len(buf), 16), ctx)
    t.count_device(upload(buf), len(buf), pre, **kw)
    ctx.synchronize()
    return t, oracle_items(buf, k, path, pre)


def assert_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, what
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError((what, f"{bad.size} rows differ, first {int(bad[0])}", got[bad[0]].tolist(), want[bad[0]].tolist()))


def bases(rng, n) -> bytes:
    return ACGT[rng.integers(0, 4, n)].tobytes()


def once_weak(rng, k, windows, weak):
    """A random record of `windows` windows and the reads that count each of its k-mers twice, but those at the window indices
    `weak` once: at min_count 2 exactly those windows are weak (the k-mers of random bases at k >= 21 do not repeat)."""
    r = bases(rng, windows + k - 1)
    cuts = [-1] + sorted(weak) + [windows]
    second = [r[a + 1: b + k - 1] for a, b in zip(cuts[:-1], cuts[1:]) if b - a > 1]   # the windows a + 1 .. b - 1 once more
    return r, [r] + second


# ---- 1. exact against the model --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [7, 0x7B0017])
def test_random_records_match_the_model(ctx, seed):
    """Every (path, pre) x k, the table counted from the same records and from every second record (absent k-mers), both modes,
    min_count 0, 1, 3 and min_length 0, k, 50."""
    recs = random_records(seed)
    buf, off = pack(recs), T.offsets(recs)
    dev = upload(buf)
    kept, lens = {m: 0 for m in MODES}, np.array([len(r) for r in recs], dtype=np.uint64)
    for path, pre in PATH_PRES:
        for k in KS:
            wins = [T.record_windows(r, k, path, pre) for r in recs]
            for tab in (recs, recs[::2]):
                t, items = counted(ctx, k, path, pre, tab)
                with t, nt.ReadTrimmer(t) as rt:
                    for mc in MIN_COUNTS:
                        for mode in MODES:
                            for ml in (0, k, 50):
                                want = T.rows_from_windows(recs, wins, items, k, mode, mc, ml)
                                got = run(rt, dev, len(buf), off, pre, min_count=mc, mode=mode, min_length=ml)
                                assert_rows(got, want, (seed, path, pre, k, len(tab), mc, mode, ml))
                                if ml == 0:
                                    kept[mode] += int(((want[:, 1] > 0) & (want[:, 1] < lens)).sum())
    assert min(kept.values()) > 1000   # records that are cut, not kept whole or dropped


def test_quality_stream_masks_as_the_table_does(ctx):
    recs = random_records(0x7B0021)
    buf, off = pack(recs), T.offsets(recs)
    rng = np.random.default_rng(9)
    qual = rng.integers(33, 75, len(buf)).astype(np.uint8)
    quals = [qual[int(off[i]): int(off[i + 1]) - 1] for i in range(len(recs))]
    dev, dq = upload(buf), upload(qual.tobytes(), fill=0xFF)
    for path, pre, k in ((BYTES, nt.PRE_NORMALIZE, 21), (BITS, nt.PRE_NONE, 5), (BITS_CANON, nt.PRE_STRIP_RETURNS, 32), (BYTES, nt.PRE_NORMALIZE_IUPAC, 16)):
        for tab in (recs, recs[::2]):
            tbuf = pack(tab)
            tq = np.concatenate([np.append(quals[i], 0xFF) for i in range(0, len(recs), 1 if tab is recs else 2)]).astype(np.uint8)
            items = oracle_items(quality_masked(tbuf, tq), k, path, pre)
            with nt.KmerTable(k, path, len(buf), ctx) as t, nt.ReadTrimmer(t) as rt:
                t.count_device(upload(tbuf), len(tbuf), pre, d_qual=upload(tq.tobytes(), fill=0xFF), quality_cutoff=CUTOFF)
                for mode in MODES:
                    for mc, ml in ((1, 0), (3, 0), (0, 50)):
                        want = T.rows(recs, items, k, path, pre, mode, mc, ml, quals, CUTOFF)
                        got = run(rt, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=CUTOFF, min_count=mc, mode=mode, min_length=ml)
                        assert_rows(got, want, ("quality", path, k, len(tab), mode, mc, ml))
                    unmasked = T.rows(recs, items, k, path, pre, mode)
                    assert not np.array_equal(unmasked, T.rows(recs, items, k, path, pre, mode, 1, 0, quals, CUTOFF))
                    assert_rows(run(rt, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=0, mode=mode), unmasked, ("cutoff 0", path, k))
                    assert_rows(run(rt, dev, len(buf), off, pre, mode=mode), unmasked, ("no stream", path, k))


def test_rows_agree_with_read_abundance(ctx):
    """n_kmers / n_solid are ReadAbundance's n_kmers / n_present on the same call."""
    recs = random_records(0x7B0022, 400)
    buf, off = pack(recs), T.offsets(recs)
    dev, d_off = upload(buf), dev_u64(off)
    weak = 0
    for path, pre, k in ((BYTES, nt.PRE_NORMALIZE, 21), (BITS, nt.PRE_NONE, 5), (BITS_CANON, nt.PRE_NONE, 31)):
        t, _ = counted(ctx, k, path, pre, recs[::2])
        with t, nt.ReadAbundance(t) as ra, nt.ReadTrimmer(t) as rt:
            for mc in MIN_COUNTS:
                a = host(ra.run_device(dev, len(buf), d_off, len(recs), pre, min_count=mc))
                for mode in MODES:
                    r = host(rt.run_device(dev, len(buf), d_off, len(recs), pre, min_count=mc, mode=mode, min_length=50))
                    assert np.array_equal(r[:, 2], a[:, 0]) and np.array_equal(r[:, 3], a[:, 1]), (path, k, mc, mode)
                weak += int((a[:, 1] < a[:, 0]).sum())
    assert weak > 500   # records with windows the table does not hold often enough


# ---- 2. geometry -----------------------------------------------------------------------------------------------------------------------

def _at_every_offset(recs_by_kind, rng):
    """Every record of every kind 64 times, each copy after a record of N whose length puts the copy's start on the next offset
    mod 64.  Returns the records and, per record, its start offset mod 64 (-1 for the spacers)."""
    out, starts, at = [], [], 0
    for r in recs_by_kind:
        for target in range(64):
            pad = (target - at - 1) % 64   # the spacer takes pad bytes and its break byte
            out.append(b"N" * pad)
            starts.append(-1)
            at += pad + 1
            assert at % 64 == target
            out.append(r)
            starts.append(target)
            at += len(r) + 1
    return out, np.array(starts)


@pytest.mark.parametrize("k,path,pre", [(21, BYTES, nt.PRE_NORMALIZE), (1, BITS, nt.PRE_NONE), (32, BITS_CANON, nt.PRE_NONE)])
def test_window_counts_at_the_word_group_and_round_seams_at_every_offset(ctx, k, path, pre):
    """Records of 0, 1, 63..65, 127..129, 2047..2049 (the last a group of lanes takes and the first of the whole wave) and 4095..4097
    windows (one round of the wave and the next), each starting at every offset mod 64: all solid, with an N in the middle, and with
    rare k-mers (min_count 3 against reads of uneven depth)."""
    rng = np.random.default_rng(0x70 + k)
    genome = bases(rng, 5000)
    table_reads = [genome[s:s + int(n)] for s, n in zip(rng.integers(0, 4800, 250) ** 2 // 4800, rng.integers(40, 200, 250))] + [genome]
    kinds = []
    for w in (0, 1, 63, 64, 65, 127, 128, 129, GROUP_WORDS * 64 - 1, GROUP_WORDS * 64, GROUP_WORDS * 64 + 1, ROUND - 1, ROUND, ROUND + 1):
        L = w + k - 1
        s = int(rng.integers(0, 5000 - L)) if L < 5000 else 0
        r = genome[s:s + L]
        kinds.append(r)
        if w > 2 * k + 2:
            kinds.append(r[:L // 2] + b"N" + r[L // 2 + 1:])
    recs, starts = _at_every_offset(kinds, rng)
    buf, off = pack(recs), T.offsets(recs)
    assert set((off[:-1][starts >= 0] % 64).tolist()) == set(range(64))
    t, items = counted(ctx, k, path, pre, table_reads)
    wins = [T.record_windows(r, k, path, pre) for r in recs]
    with t, nt.ReadTrimmer(t) as rt:
        dev = upload(buf)
        for mode in MODES:
            for mc in (1, 3):
                want = T.rows_from_windows(recs, wins, items, k, mode, mc)
                if mc == 1:
                    assert {0, 1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097} <= set(want[:, 2].tolist())
                elif k > 1:
                    assert int(((want[:, 3] < want[:, 2]) & (want[:, 3] > 0)).sum()) > 300
                assert_rows(run(rt, dev, len(buf), off, pre, min_count=mc, mode=mode), want, (k, path, mode, mc))


@pytest.mark.parametrize("k,path,pre", [(21, BYTES, nt.PRE_NORMALIZE), (31, BITS_CANON, nt.PRE_NONE)])
def test_one_weak_window_at_every_position(ctx, k, path, pre):
    """Records of 70 and 131 windows (two and three plane words), record i with exactly window i weak, the records one after the
    other so that their starts fall on every offset mod 64."""
    rng = np.random.default_rng(0x7D)
    recs, table = [], []
    for windows in (70, 131):
        for i in range(windows):
            r, reads = once_weak(rng, k, windows, [i])
            recs.append(r)
            table += reads
    buf, off = pack(recs), T.offsets(recs)
    assert set((off[:-1] % 64).tolist()) == set(range(64))
    t, items = counted(ctx, k, path, pre, table)
    wins = [T.record_windows(r, k, path, pre) for r in recs]
    with t, nt.ReadTrimmer(t) as rt:
        dev = upload(buf)
        for mode in MODES:
            want = T.rows_from_windows(recs, wins, items, k, mode, 2)
            assert (want[:, 3] == want[:, 2] - 1).all()   # the case is what it claims: one weak window per record
            if mode == T.PREFIX:
                assert want[:70, 1].tolist() == [0] + [k - 1 + i for i in range(1, 70)]
            else:
                assert want[:70, 0].tolist() == [i + 1 if 69 - i > i else 0 for i in range(70)]
            assert_rows(run(rt, dev, len(buf), off, pre, min_count=2, mode=mode), want, (k, path, mode))


def test_two_equal_runs(ctx):
    """Two (and three) solid runs of the same length: the leftmost is kept, whether the runs lie in one word, in the words of a group,
    or in different rounds of the wave; a later run that is one window longer wins."""
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    rng = np.random.default_rng(0x7E)
    recs = []
    for n in (1, 2, 20, 44, 64, 100, 1000, ROUND - 7, ROUND, 3 * ROUND + 5):
        a, b, c = (bases(rng, n + k - 1) for _ in range(3))
        recs += [a + b"N" + b, a + b"N" + b + b"N" + c, a + b"N" + b + bases(rng, 1), bases(rng, 7) + b"N" + a + b"NN" + b]
    buf, off = pack(recs), T.offsets(recs)
    t, items = counted(ctx, k, path, pre, recs)
    want = T.rows(recs, items, k, path, pre, T.LONGEST)
    assert (want[0::4, 0] == 0).all() and (want[1::4, 0] == 0).all()           # ties: the first run
    assert (want[2::4, 0] > 0).all() and (want[3::4, 0] == 8).all()            # a longer second run; a tie after a short first run
    with t, nt.ReadTrimmer(t) as rt:
        assert_rows(run(rt, upload(buf), len(buf), off, pre, mode=T.LONGEST), want, "ties")
        assert_rows(run(rt, upload(buf), len(buf), off, pre, mode=T.PREFIX), T.rows(recs, items, k, path, pre, T.PREFIX), "prefix")


def test_a_batch_above_a_chunk_with_weak_windows_around_the_seam(ctx):
    """A batch of 64 MiB + 8 KiB: records of N up to a region of short records around the chunk seam, one of them across it with one
    weak window that ends at the seam - k .. the seam + k."""
    n_bytes = CM.CHUNK + 8192
    dev = torch.empty(((n_bytes + 15) // 16 * 16 + 64,), dtype=torch.uint8, device="cuda")
    for k, path, pre in ((21, BYTES, nt.PRE_NORMALIZE), (32, BITS, nt.PRE_NONE)):
        rng = np.random.default_rng(0x5EA0 + k)
        windows, inside = 300, 170   # the seam falls on byte `inside` of the record
        before, after = random_records(0x7F, 4), random_records(0x80, 4)
        for d in range(-k, k + 1):
            weak = inside + d - (k - 1)           # the window that ends at the seam + d
            r, reads = once_weak(rng, k, windows, [weak])
            region = before + [r] + after
            start = CM.CHUNK - inside - len(pack(before))
            dev.fill_(ord("N"))
            dev[n_bytes - 1:] = ord("\n")
            dev[start - 1] = ord("\n")
            reg = pack(region)
            dev[start:start + len(reg)] = torch.from_numpy(np.frombuffer(reg, dtype=np.uint8).copy()).cuda()
            off = np.concatenate([[0], start + T.offsets(region), [n_bytes]]).astype(np.uint64)
            assert off[1 + len(before)] + inside == CM.CHUNK
            t, items = counted(ctx, k, path, pre, reads + before + before + after + after)
            with t, nt.ReadTrimmer(t) as rt:
                for mode in MODES:
                    want = np.zeros((len(off) - 1, 4), dtype=np.uint64)   # the two fillers: records of N
                    want[1:-1] = T.rows(region, items, k, path, pre, mode, 2)
                    me = want[1 + len(before)]
                    assert me[2] == windows and me[3] == windows - 1
                    assert me[1] == (k - 1 + weak if mode == T.PREFIX else max(weak, windows - 1 - weak) + k - 1)
                    assert_rows(run(rt, dev, n_bytes, off, pre, min_count=2, mode=mode), want, (k, path, d, mode))
    del dev
    torch.cuda.empty_cache()


def _long_record(rng, n, k, holes):
    r = bytearray(bases(rng, n))
    for h in holes:
        r[h] = ord("N")
    return bytes(r)


def test_one_record_of_four_million_bases(ctx):
    """One record of 2^22 + 1000 bases between short ones, all solid but for single N at the wave's round seams (window ends at
    multiples of 4096 from the record's first plane word, one before and one after), so that the leading run, the longest run and the
    trailing run each cross rounds; then its compaction, which goes through rt_copy_long_kernel, with a parallel stream."""
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    rng = np.random.default_rng(0x81)
    n = (1 << 22) + 1000
    head = [bases(rng, 100), bases(rng, 57)]
    first = len(pack(head))   # the long record's first byte in the batch
    seam = lambda j: ((first + k - 1) // 64 + 64 * j) * 64 - first   # noqa: E731  (the record byte at which round j's windows start to end)
    holes = [seam(3) + 5, seam(3) + 5 + 2 * ROUND, seam(700), seam(701) - 1, seam(900) + 1, seam(1000) - k, n - 3 * ROUND]
    big = _long_record(rng, n, k, holes)
    recs = head + [big] + [bases(rng, 80)]
    buf, off = pack(recs), T.offsets(recs)
    t, items = counted(ctx, k, path, pre, recs)
    dev, d_off = upload(buf), dev_u64(off)
    aux = rng.integers(33, 127, len(buf)).astype(np.uint8)
    d_aux = upload(aux.tobytes())
    with t, nt.ReadTrimmer(t) as rt:
        for mode in MODES:
            want = T.rows(recs, items, k, path, pre, mode)
            assert want[2][2] == n - k + 1 - k * len(holes) and want[2][1] > 2 * ROUND and (mode == T.PREFIX or want[2][0] > 0)
            rows = rt.run_device(dev, len(buf), d_off, len(recs), pre, mode=mode)
            assert_rows(host(rows), want, ("4M", mode))
            _check_compaction(rt, recs, buf, off, dev, d_off, rows, want, aux, d_aux, ("4M", mode))
            assert mode == T.PREFIX or (want[2][1] + 16) // 16 > LONG_PIECES   # the longest run goes through rt_copy_long_kernel


# ---- 3. the compaction ------------------------------------------------------------------------------------------------------------------

def _check_compaction(rt, recs, buf, off, dev, d_off, d_rows, rows, aux, d_aux, what):
    """compact_device against the model: bytes, padding, offsets, sources, and the parallel stream with the source's break bytes."""
    auxs = None if aux is None else [aux[int(off[i]): int(off[i + 1]) - 1] for i in range(len(recs))]
    brks = None if aux is None else [int(aux[int(off[i + 1]) - 1]) for i in range(len(recs))]
    want = T.compact(recs, rows, auxs, brks)
    got = rt.compact_device(dev, len(buf), d_off, len(recs), d_rows, d_aux)
    assert len(got) == len(want) and got[1] == want[1], what
    pad = len(want[0])
    assert pad == (want[1] + 15) // 16 * 16
    assert got[0].dtype == torch.uint8 and got[0].is_cuda and got[2].dtype == got[3].dtype == torch.int64
    assert np.array_equal(host(got[0])[:pad], np.frombuffer(want[0], dtype=np.uint8)), what
    assert np.array_equal(host(got[2]), want[2]) and np.array_equal(host(got[3]), want[3]), what
    if aux is not None:
        assert np.array_equal(host(got[4])[:pad], np.frombuffer(want[4], dtype=np.uint8)), what
    return got


def test_compaction_matches_the_model(ctx):
    """Rows of both modes on random records and on reads of every length 0..200 (every alignment of source and destination), with and
    without a parallel stream; then the output fed back: trimmed again with the same table and min_count, every record is kept whole."""
    rng = np.random.default_rng(0x82)
    genome = bases(rng, 3000)
    ladder = [genome[s:s + L] for L in range(0, 201) for s in (int(rng.integers(0, 2800)),)]
    for i in range(60, len(ladder), 3):   # a substitution in the middle: k weak windows
        r = bytearray(ladder[i])
        r[len(r) // 2] = b"CGTA"[b"ACGT".index(r[len(r) // 2])]
        ladder[i] = bytes(r)
    for recs, k, path, pre, mc in ((random_records(0x7B0041, 300), 5, BITS, nt.PRE_NONE, 3),
                                   (random_records(0x7B0042, 300), 21, BYTES, nt.PRE_NORMALIZE, 1),
                                   (ladder + random_records(0x7B0043, 100), 16, BITS_CANON, nt.PRE_NORMALIZE, 2)):
        buf, off = pack(recs), T.offsets(recs)
        dev, d_off = upload(buf), dev_u64(off)
        aux = rng.integers(33, 127, len(buf)).astype(np.uint8)
        d_aux = upload(aux.tobytes())
        t, items = counted(ctx, k, path, pre, recs[::2] + [genome, genome])
        with t, nt.ReadTrimmer(t) as rt:
            for mode in MODES:
                for ml in (0, 50):
                    rows = rt.run_device(dev, len(buf), d_off, len(recs), pre, min_count=mc, mode=mode, min_length=ml)
                    want = T.rows(recs, items, k, path, pre, mode, mc, ml)
                    assert_rows(host(rows), want, (k, mode, ml))
                    n_cut = int(((want[:, 1] > 0) & (want[:, 1] < np.array([len(r) for r in recs]))).sum())
                    assert n_cut > 20 and int((want[:, 1] == 0).sum()) > 0   # some cut, some dropped
                    _check_compaction(rt, recs, buf, off, dev, d_off, rows, want, None, None, (k, mode, ml))
                    out = _check_compaction(rt, recs, buf, off, dev, d_off, rows, want, aux, d_aux, (k, mode, ml, "aux"))
                    # the property: every kept interval holds solid windows only, so a second pass keeps every record whole
                    n_out = len(out[3])
                    again = host(rt.run_device(out[0], out[1], out[2], n_out, pre, min_count=mc, mode=mode, min_length=ml))
                    o = host(out[2])
                    assert (again[:, 0] == 0).all() and np.array_equal(again[:, 1], o[1:] - o[:-1] - 1), (k, mode, ml)
                    assert (again[:, 2] == again[:, 3]).all() and n_out > 50
                    same = rt.compact_device(out[0], out[1], out[2], n_out, rt.run_device(out[0], out[1], out[2], n_out, pre, min_count=mc,
                                                                                           mode=mode, min_length=ml))
                    assert same[1] == out[1] and torch.equal(same[0][:out[1]], out[0][:out[1]]) and torch.equal(same[2], out[2])
                    assert host(same[3]).tolist() == list(range(n_out))


def test_all_solid_records_come_back_unchanged_and_all_weak_ones_leave_nothing(ctx):
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    rng = np.random.default_rng(0x83)
    recs = [bases(rng, int(n)) for n in rng.integers(k, 400, 500)]
    buf, off = pack(recs), T.offsets(recs)
    dev, d_off = upload(buf), dev_u64(off)
    t, _ = counted(ctx, k, path, pre, recs)
    with t, nt.ReadTrimmer(t) as rt:
        for mode in MODES:
            rows = rt.run_device(dev, len(buf), d_off, len(recs), pre, mode=mode)
            seq, n, o, src = rt.compact_device(dev, len(buf), d_off, len(recs), rows)
            assert n == len(buf) and host(seq)[:n].tobytes() == buf and np.array_equal(host(o), off)
            assert host(src).tolist() == list(range(len(recs)))
            assert (host(seq)[n:(n + 15) // 16 * 16] == ord("\n")).all()
            # nothing reaches min_count: every record is dropped, which is NTK_OK with 0 records and 0 bytes
            rows = rt.run_device(dev, len(buf), d_off, len(recs), pre, min_count=1000, mode=mode)
            assert not host(rows)[:, [0, 1, 3]].any()
            seq, n, o, src = rt.compact_device(dev, len(buf), d_off, len(recs), rows)
            assert n == 0 and host(o).tolist() == [0] and len(src) == 0
        assert rt.trim_records([], pre) == []


def _compact_status(rt, dev, aux, n_bytes, d_off, n_records, rows, out_seq, out_aux, cap_bytes, out_off, out_src, cap_records):
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    nb, nr = C.c_uint64(77), C.c_uint64(77)
    rc = trimming.lib().ntk_read_trim_compact_device(rt._h, ptr(dev), ptr(aux), n_bytes, ptr(d_off), n_records, ptr(rows), ptr(out_seq),
                                                     ptr(out_aux), cap_bytes, ptr(out_off), ptr(out_src), cap_records, C.byref(nb), C.byref(nr))
    return rc, nb.value, nr.value


def test_capacity_protocol_and_hand_made_rows(ctx):
    """The size query, capacities one too small and exact, and rows that did not come from run_device, some reaching beyond their record."""
    k, path, pre = 5, BITS, nt.PRE_NONE
    rng = np.random.default_rng(0x84)
    recs = [bases(rng, int(n)) for n in rng.integers(0, 90, 200)]
    buf, off = pack(recs), T.offsets(recs)
    dev, d_off = upload(buf), dev_u64(off)
    L = np.array([len(r) for r in recs], dtype=np.uint64)
    rows = np.zeros((len(recs), 4), dtype=np.uint64)
    rows[:, 0] = rng.integers(0, 100, len(recs))
    rows[:, 1] = rng.integers(0, 100, len(recs))
    rows[3] = [0, (1 << 64) - 1, 0, 0]            # length beyond everything
    rows[4] = [(1 << 64) - 1, (1 << 64) - 1, 0, 0]
    rows[5] = [(1 << 63), 5, 0, 0]
    rows[:, 2:] = rng.integers(0, 1 << 62, (len(recs), 2))   # the counters are not read
    assert int((rows[:, 0] + rows[:, 1] > L).sum()) > 50 and int((rows[:, 0] + rows[:, 1] <= L).sum()) > 10
    d_rows = dev_u64(rows.reshape(-1)).reshape(len(recs), 4)
    want = T.compact(recs, rows)
    n_out, need = len(want[3]), len(want[0])
    assert 0 < n_out < len(recs) and want[1] % 16
    t, _ = counted(ctx, k, path, pre, recs)
    with t, nt.ReadTrimmer(t) as rt:
        got = rt.compact_device(dev, len(buf), d_off, len(recs), d_rows)
        assert got[1] == want[1] and host(got[0])[:need].tobytes() == want[0]
        assert np.array_equal(host(got[2]), want[2]) and np.array_equal(host(got[3]), want[3])
        args = (rt, dev, None, len(buf), d_off, len(recs), d_rows)
        assert _compact_status(*args, None, None, 0, None, None, 0) == (ERR_CAPACITY, want[1], n_out)       # the size query
        pattern = 0x5A
        out_seq = torch.full((need + 64,), pattern, dtype=torch.uint8, device="cuda")
        out_off = torch.full((n_out + 1,), pattern, dtype=torch.int64, device="cuda")
        out_src = torch.full((n_out,), pattern, dtype=torch.int64, device="cuda")
        untouched = lambda: bool((out_seq == pattern).all() and (out_off == pattern).all() and (out_src == pattern).all())   # noqa: E731
        assert _compact_status(*args, out_seq, None, need - 16, out_off, out_src, n_out) == (ERR_CAPACITY, want[1], n_out)
        assert _compact_status(*args, out_seq, None, need, out_off, out_src, n_out - 1) == (ERR_CAPACITY, want[1], n_out)
        assert _compact_status(*args, out_seq, None, want[1], out_off, out_src, n_out) == (ERR_CAPACITY, want[1], n_out)   # not rounded up
        torch.cuda.synchronize()
        assert untouched()
        assert _compact_status(*args, out_seq, None, need, out_off, out_src, n_out) == (0, want[1], n_out)   # exactly enough
        assert host(out_seq)[:need].tobytes() == want[0] and bool((out_seq[need:] == pattern).all())
        assert np.array_equal(host(out_off), want[2]) and np.array_equal(host(out_src), want[3])
        # the worst case always suffices
        big_seq = torch.empty((len(buf) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        big_off, big_src = torch.empty(len(recs) + 1, dtype=torch.int64, device="cuda"), torch.empty(len(recs), dtype=torch.int64, device="cuda")
        assert _compact_status(*args, big_seq, None, big_seq.numel(), big_off, big_src, len(recs)) == (0, want[1], n_out)
        # nothing kept: NTK_OK with 0 and 0, also as a size query
        zero = torch.zeros((len(recs), 4), dtype=torch.int64, device="cuda")
        assert _compact_status(rt, dev, None, len(buf), d_off, len(recs), zero, None, None, 0, None, None, 0) == (0, 0, 0)
        assert _compact_status(rt, dev, None, len(buf), d_off, len(recs), zero, out_seq, None, need, out_off, out_src, n_out) == (0, 0, 0)
        assert int(out_off[0]) == 0


# ---- 4. order, reuse ---------------------------------------------------------------------------------------------------------------------

def test_repeated_calls_grow_shrink_and_release(ctx):
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    rng = np.random.default_rng(0x85)
    genome = bases(rng, 20_000)
    reads = [genome[s:s + int(n)] for s, n in zip(rng.integers(0, 19_700, 3000), rng.integers(30, 300, 3000))]
    t, items = counted(ctx, k, path, pre, reads[::3])
    sizes = (50, 3000, 700, 1, 2500)
    want = {n: T.rows(reads[:n], items, k, path, pre, T.LONGEST, 2) for n in sizes}
    with t, nt.ReadTrimmer(t) as rt:
        for release in (False, True):
            for n in sizes:
                buf, off = pack(reads[:n]), T.offsets(reads[:n])
                dev, d_off = upload(buf), dev_u64(off)
                rows = rt.run_device(dev, len(buf), d_off, n, pre, min_count=2, mode=T.LONGEST)
                assert_rows(host(rows), want[n], (release, n))
                _check_compaction(rt, reads[:n], buf, off, dev, d_off, rows, want[n], None, None, (release, n))
                if release:
                    rt.release()
        rt.release()
        rt.release()   # nothing left to free
        with nt.ReadTrimmer(t) as never_ran:
            never_ran.release()
        # the packer's route
        kept = rt.trim_records(reads[:700], pre, mode="longest", min_count=2)
        model = T.compact(reads[:700], want[700])
        o = model[2]
        assert kept == [(int(s), model[0][int(o[i]): int(o[i + 1]) - 1]) for i, s in enumerate(model[3])]
        quals = [bytes(rng.integers(33, 127, len(r)).astype(np.uint8)) for r in reads[:700]]
        kept_q = rt.trim_records(reads[:700], pre, mode=T.LONGEST, min_count=2, quals=quals)
        assert [x[:2] for x in kept_q] == kept
        assert [x[2] for x in kept_q] == [quals[s][int(want[700][s][0]): int(want[700][s][0] + want[700][s][1])] for s, _ in kept]


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------------

def _status(rt, dev, n_bytes, d_off, n_records, k, path, pre, flags=0, rows=None, min_count=1, mode=0, min_length=0, qual=None):
    p = NL.Params(k, path, pre, flags)
    ptr = lambda x: None if x is None else (C.c_void_p(x) if isinstance(x, int) else C.c_void_p(x.data_ptr()))   # noqa: E731
    return trimming.lib().ntk_read_trim_run_device(rt._h, ptr(dev), ptr(qual), n_bytes, ptr(d_off), n_records, C.byref(p), min_count, mode,
                                                   min_length, ptr(rows))


def test_errors(ctx):
    recs = random_records(0x7B0031, 40)
    buf, off = pack(recs), T.offsets(recs)
    dev, d_off = upload(buf), dev_u64(off)
    n, pattern = len(recs), 0x5A5A5A5A5A5A5A5A
    rows = torch.full((n, 4), pattern, dtype=torch.int64, device="cuda")
    untouched = lambda: bool((rows == pattern).all())   # noqa: E731
    ok = (21, BITS_CANON, nt.PRE_NORMALIZE)
    with nt.KmerTable(21, BITS_CANON, len(buf), ctx) as t, nt.ReadTrimmer(t) as rt:
        t.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        args = (rt, dev, len(buf), d_off, n)
        for mode in (2, 3, 0xFFFFFFFF):
            assert _status(*args, *ok, rows=rows, mode=mode) == ERR_BAD_ARG                          # no such mode
        assert _status(*args, 20, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG            # k is not the table's
        assert _status(*args, 33, BITS_CANON, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG
        assert _status(*args, 21, BITS, nt.PRE_NORMALIZE, rows=rows) == ERR_BAD_ARG                  # nor the path
        assert _status(*args, *ok, flags=5, rows=rows) == ERR_BAD_ARG                                # a minimizer window
        assert _status(*args, *ok, flags=NL.FLAG_RESET, rows=rows) == ERR_BAD_ARG
        assert _status(*args, 21, BITS_CANON, 4, rows=rows) == ERR_BAD_ARG                           # no such pre-step
        assert _status(*args, *ok, rows=None) == ERR_BAD_ARG                                         # null pointers, sizes not zero
        assert _status(rt, None, len(buf), d_off, n, *ok, rows=rows) == ERR_BAD_ARG
        assert _status(rt, dev, len(buf), None, n, *ok, rows=rows) == ERR_BAD_ARG
        # misaligned pointers
        assert _status(rt, dev.data_ptr() + 8, len(buf) - 8, d_off, n, *ok, rows=rows) == ERR_BAD_ARG
        assert _status(*args, *ok, rows=rows, qual=dev.data_ptr() + 1) == ERR_BAD_ARG
        assert _status(rt, dev, len(buf), d_off.data_ptr() + 4, n, *ok, rows=rows) == ERR_BAD_ARG
        assert _status(*args, *ok, rows=rows.data_ptr() + 4) == ERR_BAD_ARG
        assert untouched()
        # nothing to do: NTK_OK, nothing touched, whatever the pointers
        assert _status(rt, dev, len(buf), d_off, 0, *ok, rows=rows) == 0
        assert _status(rt, None, 0, None, 0, *ok, rows=None) == 0
        assert _status(rt, dev, 0, d_off, n, *ok, rows=rows) == 0
        assert untouched()
        assert tuple(rt.run_device(dev, len(buf), d_off, 0, nt.PRE_NORMALIZE).shape) == (0, 4)
        # the compaction's arguments
        out_seq = torch.empty(len(buf) + 64, dtype=torch.uint8, device="cuda")
        out_off, out_src = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
        good = rt.run_device(dev, len(buf), d_off, n, nt.PRE_NORMALIZE)
        cap = (len(buf) + 15) // 16 * 16
        assert _compact_status(rt, dev, dev, len(buf), d_off, n, good, out_seq, None, cap, out_off, out_src, n)[0] == ERR_BAD_ARG   # one aux only
        assert _compact_status(rt, dev, None, len(buf), d_off, n, good, out_seq, out_seq, cap, out_off, out_src, n)[0] == ERR_BAD_ARG
        assert _compact_status(rt, None, None, len(buf), d_off, n, good, out_seq, None, cap, out_off, out_src, n)[0] == ERR_BAD_ARG
        assert _compact_status(rt, dev, None, len(buf), None, n, good, out_seq, None, cap, out_off, out_src, n)[0] == ERR_BAD_ARG
        assert _compact_status(rt, dev, None, len(buf), d_off, n, None, out_seq, None, cap, out_off, out_src, n)[0] == ERR_BAD_ARG
        assert _compact_status(rt, dev, None, len(buf), d_off, n, good, None, None, cap, out_off, out_src, n)[0] == ERR_BAD_ARG
        assert _compact_status(rt, dev, None, len(buf), d_off, n, good, out_seq, None, cap, None, out_src, n)[0] == ERR_BAD_ARG
        assert _compact_status(rt, dev, None, len(buf), d_off, n, good, out_seq[8:], None, cap, out_off, out_src, n)[0] == ERR_BAD_ARG   # misaligned
        assert _compact_status(rt, dev, None, 0, d_off, n, good, out_seq, None, cap, out_off, out_src, n) == (0, 0, 0)
        assert _compact_status(rt, dev, None, len(buf), d_off, 0, good, out_seq, None, cap, out_off, out_src, n) == (0, 0, 0)
        lib = trimming.lib()
        assert lib.ntk_read_trim_compact_device(rt._h, None, None, 0, None, 0, None, None, None, 0, None, None, 0, None, None) == ERR_BAD_ARG
        # and the calls that are right, after release as well
        want = T.rows(recs, oracle_items(buf, *ok), *ok, T.PREFIX)
        assert _status(*args, *ok, rows=rows) == 0
        assert_rows(host(rows), want, "after the errors")
        rt.release()
        assert _status(*args, *ok, rows=rows, mode=1, min_length=30) == 0
        assert_rows(host(rows), T.rows(recs, oracle_items(buf, *ok), *ok, T.LONGEST, 1, 30), "after release")
    lib = trimming.lib()
    h = C.c_void_p()
    with nt.KmerTable(21, BYTES, len(buf), ctx) as t:
        assert lib.ntk_read_trim_create(None, t._h, C.byref(h)) == ERR_BAD_ARG
        assert lib.ntk_read_trim_create(ctx._h, None, C.byref(h)) == ERR_BAD_ARG
        assert lib.ntk_read_trim_create(ctx._h, t._h, None) == ERR_BAD_ARG
        assert lib.ntk_read_trim_release(None) == ERR_BAD_ARG
        lib.ntk_read_trim_destroy(None)
        with nt.ReadTrimmer(t) as rt:   # un-normalised byte-path input, as for the table
            rows.fill_(pattern)
            for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):
                assert _status(rt, dev, len(buf), d_off, n, 21, BYTES, pre, rows=rows) == ERR_UNSUPPORTED
            assert untouched()
            with pytest.raises(nt.NtkError) as e:
                rt.run_device(dev, len(buf), d_off, n, nt.PRE_NONE)
            assert e.value.status == ERR_UNSUPPORTED
            with pytest.raises(nt.NtkError) as e:
                rt.run_device(dev, len(buf), d_off, n, nt.PRE_NORMALIZE, mode=7)
            assert e.value.status == ERR_BAD_ARG


def test_incomplete_table_writes_no_row(ctx):
    recs = random_records(0x7B0032, 40)
    buf, off = pack(recs), T.offsets(recs)
    dev, d_off = upload(buf), dev_u64(off)
    pattern = 0x5A5A5A5A5A5A5A5A
    rows = torch.full((len(recs), 4), pattern, dtype=torch.int64, device="cuda")
    with nt.KmerTable(21, BITS_CANON, 1, ctx) as t, nt.ReadTrimmer(t) as rt:
        t.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        assert t.stats()["n_dropped"] > 0
        for mode in MODES:
            assert _status(rt, dev, len(buf), d_off, len(recs), 21, BITS_CANON, nt.PRE_NORMALIZE, rows=rows, mode=mode) == ERR_CAPACITY
        torch.cuda.synchronize()
        assert bool((rows == pattern).all())
        with pytest.raises(nt.NtkError) as e:
            rt.trim_records(recs, nt.PRE_NORMALIZE)
        assert e.value.status == ERR_CAPACITY
        t.reset()   # the same handle on the table once it is complete again: nothing is solid
        assert not run(rt, dev, len(buf), off, nt.PRE_NORMALIZE)[:, [0, 1, 3]].any()


def test_wide_table_is_refused(ctx):
    with nt.WideKmerTable(40, BYTES, 1000, ctx) as w:
        with pytest.raises(TypeError, match="33..63"):
            nt.ReadTrimmer(w)


# ---- 6. the example ---------------------------------------------------------------------------------------------------------------------

def test_trim_reads_cli(ctx, tmp_path):
    """trim_reads on the golden FASTQ head at k = 21, MIN_COUNT 2 (chosen on the CPU: the model keeps some records whole, shortens
    some and drops some in both modes), against the model's text; then as FASTA, and against a reference."""
    import oracle as O  # the checker
    exe = os.path.join(ROOT, "examples", "trim_reads")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    fq = os.path.join(GOLDEN, "PRJNA271013_head.fq")
    parsed = list(nt.parse_fastx_file(fq))
    names, quals = [r.id for r in parsed], [r.qual.encode() for r in parsed]
    seqs = [O.normalize(r.raw_seq)[0] for r in parsed]
    assert all(len(s) == len(q) == len(r.raw_seq) for s, q, r in zip(seqs, quals, parsed))
    k, pre = 21, nt.PRE_NORMALIZE
    items = oracle_items(pack(seqs), k, BYTES, pre)
    wins = [T.record_windows(s, k, BYTES, pre) for s in seqs]
    L = np.array([len(s) for s in seqs], dtype=np.uint64)
    for mode, ml, extra in ((T.PREFIX, 0, []), (T.LONGEST, 0, ["--longest"]), (T.LONGEST, 50, ["--longest", "-l", "50"])):
        rows = T.rows_from_windows(seqs, wins, items, k, mode, 2, ml)
        whole, dropped = int((rows[:, 1] == L).sum()), int((rows[:, 1] == 0).sum())
        shortened = len(seqs) - whole - dropped
        print(f"mode {mode}, min_length {ml}: {whole} whole, {shortened} shortened, {dropped} dropped")
        assert whole > 0 and shortened > 0 and dropped > 0
        r = subprocess.run([exe, "-k", str(k), "-m", "2", *extra, fq], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == T.cli_text(names, seqs, rows, quals), (mode, ml)
        kept = rows[:, 1] > 0
        assert r.stderr.strip().splitlines()[-1] == (f"trim_reads: {len(seqs)} records in, {int(kept.sum())} out; "
                                                     f"{int(L.sum())} bases in, {int(rows[:, 1].sum())} out")
    # FASTA in, FASTA out, against a reference: the first 200 reads count, min_count 1
    fa, ref = tmp_path / "reads.fa", tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), r.raw_seq) for n, r in zip(names, parsed)))
    ref.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), r.raw_seq) for n, r in zip(names[:200], parsed[:200])))
    rows = T.rows_from_windows(seqs, wins, oracle_items(pack(seqs[:200]), k, BYTES, pre), k, T.LONGEST, 1, 30)
    assert 200 <= int((rows[:, 1] > 0).sum()) < len(seqs)
    r = subprocess.run([exe, "-k", str(k), "-r", str(ref), "--longest", "-l", "30", str(fa)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == T.cli_text(names, seqs, rows)
    # a FASTQ sequence that holds a byte the pre-step deletes is refused
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"@a\nACGT ACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    r = subprocess.run([exe, str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "deletes" in r.stderr and r.stdout == ""
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 2
