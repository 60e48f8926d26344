"""The coloured k-mer index and its read screen (include/needletail_amd_colors.h, needletail_amd.KmerColors) on a real MI355X.

Truth for every answer: tests/_colors_model.py - the index is a dict built by OR, a record's k-mers are the checker's literal iterators
on `record + b"\\n"`, rows and matrices follow by definition.  Every comparison is `np.array_equal` on whole arrays; there is no
tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import coloring  # noqa: E402
import _colors_model as KM  # noqa: E402
import _count_model as CM  # noqa: E402
from _lib_fuzz import random_masks  # noqa: E402  (the structured fuzz draws its masks the same way)
from _count_helpers import CUTOFF, PATH_PRES, pack, quality_masked, random_records, upload  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (1, 5, 16, 21, 31, 32)
COLORS = (1, 3, 64)
BYTES, BITS, BITS_CANON = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS, nt.PATH_BITS_CANONICAL
LONG_RECORD = KM.LONG_RECORD   # ntk_colors.hip kLongRecord (tests/test_colors_abi.py ties them)
ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 2, 5, 6
M64 = KM.M64
PATTERN = 0x5A5A5A5A5A5A5A5A
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def to_dev(values):
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    t = torch.from_numpy(v.view(np.int64).copy()).cuda() if v.size else torch.empty(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def kset(ctx, keys, k, path):
    """A KmerSet over `keys` as they are (the index takes keys as given)."""
    t = to_dev(keys)
    return nt.KmerSet(t, torch.ones_like(t), int(np.size(keys)), k, path, ctx)


def run(kc, dev, n_bytes, off, pre, single=True, **kw):
    n = len(off) - 1
    rows, hits, alone = kc.run_device(dev, n_bytes, to_dev(off), n, pre, single=single, **kw)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (n, 5) and tuple(hits.shape) == (n, kc.n_colors) and rows.is_cuda
    assert (alone is None) == (not single)
    view = lambda t: t.cpu().numpy().view(np.uint64)   # noqa: E731
    return view(rows), view(hits), None if alone is None else view(alone)


def assert_screen(got, want, what):
    for name, g, w in zip(("rows", "hits", "single"), got, want):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype == np.uint64, (what, name)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).any(axis=1))[0]
            raise AssertionError((what, name, f"{bad.size} records differ, first {int(bad[0])}", g[bad[0]].tolist(), w[bad[0]].tolist()))


def indexed(ctx, k, path, n_colors, values, seed):
    """An index over overlapping subsets of the batch's own k-mers plus foreign keys, and its model: per-key masks in one call, then two
    references as lists under one colour each."""
    rng = np.random.default_rng(seed)
    own = np.unique(np.concatenate([np.zeros(0, np.uint64)] + list(values)))
    foreign = rng.integers(0, min(4 ** k, 1 << 63), 64, dtype=np.uint64)
    keys = np.concatenate([own, foreign, own[::5]])   # some keys twice in one call
    masks = random_masks(rng, keys.size, n_colors)
    model = KM.Index(n_colors)
    kc = nt.KmerColors(k, path, n_colors, 2 * keys.size + 16, ctx)
    kc.add_masks(keys, masks)
    model.add(keys, masks)
    for color, step in ((n_colors - 1, 3), (0, 4)):
        kc.add(kset(ctx, own[::step], k, path), color)
        model.add(own[::step], 1 << color)
    ctx.synchronize()
    return kc, model


def assert_stats(kc, model, what):
    st = kc.stats()
    assert st["n_dropped"] == 0 and st["n_keys"] == model.n_keys and st["n_masked_bits"] == model.n_masked_bits, (what, st)
    assert st["per_color"] == model.per_color(), what
    assert (st["n_colors"], st["k"], st["path"]) == (kc.n_colors, kc.k, kc.path)
    return st


# ---- 1. exact against the model ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [7, 0xC010])
def test_random_records_match_the_model(ctx, seed):
    """Every (path, pre) x k x n_colors; masks with 0, 1, several and all bits, the colour-63 bit among them; with and without d_single."""
    recs = random_records(seed)
    buf, off = pack(recs), KM.offsets(recs)
    dev = upload(buf)
    seen = {"absent": 0, "single": 0, "several": 0, "bit63": 0}
    for path, pre in PATH_PRES:
        for k in KS:
            values = [KM.record_values(r, k, path, pre) for r in recs]
            for n_colors in COLORS:
                kc, model = indexed(ctx, k, path, n_colors, values, seed + 31 * k + n_colors)
                with kc:
                    want = KM.screen_values(values, model)
                    what = (seed, path, pre, k, n_colors)
                    assert_screen(run(kc, dev, len(buf), off, pre), want, what)
                    assert_screen(run(kc, dev, len(buf), off, pre, single=False), want, what + ("no single",))
                    if k == 21 and n_colors == 3:
                        assert_stats(kc, model, what)
                        assert_screen(kc.run_records(recs, pre), want, what + ("records",))   # the packer's route
                seen["absent"] += int((want[0][:, 1] < want[0][:, 0]).sum())
                seen["single"] += int(want[0][:, 2].sum())
                seen["several"] += int((want[0][:, 1] - want[0][:, 2]).sum())
                seen["bit63"] += int(want[1][:, 63].sum()) if n_colors == 64 else 0
    assert all(v > 1000 for v in seen.values()), seen


def _genome(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)]


def _periodic(genome, start, n):
    """n bases of the genome read round and round from `start`."""
    reps = (start + n) // genome.size + 1
    return np.tile(genome, reps)[start:start + n].tobytes()


def _reads(genome, seed, n_reads, lo=40, hi=200):
    rng = np.random.default_rng(seed)
    return [_periodic(genome, int(rng.integers(0, genome.size)), int(rng.integers(lo, hi))) for _ in range(n_reads)]


@pytest.mark.parametrize("k,path,pre", [(21, BYTES, nt.PRE_NORMALIZE), (31, BITS_CANON, nt.PRE_NONE)])
def test_hits_are_the_products_own_columns(ctx, k, path, pre):
    """Against the product, not the model: hits[:, c] is the n_present column of ReadAbundance on a KmerTable that counted reference c, and
    n_kmers is its n_kmers.  Three references that overlap: reads of three genomes of which two share a half."""
    a, b, c = _genome(0xD0, 3000), _genome(0xD1, 3000), _genome(0xD2, 3000)
    b[:1500] = a[:1500]
    refs = [_reads(g, 0xD3 + i, 300) for i, g in enumerate((a, b, c))]
    reads = _reads(a, 0xD7, 150) + _reads(b, 0xD8, 150) + _reads(c, 0xD9, 100) + _reads(_genome(0xDA, 3000), 0xDB, 50) + [b"", b"ACG", b"N" * 60]
    buf, off = pack(reads), KM.offsets(reads)
    dev, d_off = upload(buf), to_dev(off)
    with nt.KmerColors(k, path, 3, sum(len(pack(r)) for r in refs), ctx) as kc:
        columns = []
        for color, ref in enumerate(refs):
            with nt.KmerTable(k, path, len(pack(ref)), ctx) as t, nt.ReadAbundance(t) as ra:
                t.count_records(ref, pre)
                kc.add(t, color)
                columns.append(ra.run_device(dev, len(buf), d_off, len(reads), pre).cpu().numpy().view(np.uint64))
        rows, hits, single = run(kc, dev, len(buf), off, pre)
    for color, col in enumerate(columns):
        assert np.array_equal(hits[:, color], col[:, 1]), color
        assert np.array_equal(rows[:, 0], col[:, 0])
    assert (hits[:, 0] > 0).sum() > 200 and ((hits[:, 0] > 0) & (hits[:, 1] > 0)).sum() > 50 and (rows[:, 1] == 0).sum() >= 50
    assert np.array_equal(rows[:, 2], single.sum(axis=1)) and (single <= hits).all()


# ---- 2. the index through lookup ---------------------------------------------------------------------------------------------------------

def test_index_edges_through_lookup(ctx):
    k, path = 32, BITS
    with nt.KmerColors(k, path, 3, 6, ctx) as kc:   # 8 slots, probe bound 8
        slots = CM.slots_for(6)
        assert kc.stats()["slots"] == slots == 8 and kc.lookup([]).shape == (0,) and kc.lookup([5]).tolist() == [0]
        kc.add_masks([], [])
        last = [int(v) for v in CM.keys_with_home(slots - 1, slots, 32, 3)]   # the probe wraps past the last slot
        model = KM.Index(3)
        for keys, masks in (([0], [1]), ([M64], [2]), (last, [1, 2, 4]), ([0], [4]), ([last[1], last[1]], [1, 4]), ([77, 78], [0, 8 | 16]),
                            ([M64], [8])):
            kc.add_masks(keys, masks)
            model.add(keys, masks)
        kc.add(kset(ctx, [last[2], 0], k, path), 1)   # the same key under another colour in another call
        model.add([last[2], 0], 2)
        queries = [0, M64, *last, 77, 78, 5]
        assert np.array_equal(kc.lookup(queries), model.lookup(queries))
        assert model.lookup(queries).tolist() == [7, 2, 1, 7, 6, 0, 0, 0]
        st = assert_stats(kc, model, "edges")
        assert (st["n_keys"], st["n_masked_bits"], st["per_color"]) == (5, 3, [3, 4, 3])
        assert kc.lookup([last[0]]).tolist() == [1]   # n = 1
        # the all-ones key through the screen: a record of T at k = 32 on the forward path
        recs = [b"T" * 40, b"A" * 40, b"T" * 31]
        got = run(kc, upload(pack(recs)), len(pack(recs)), KM.offsets(recs), nt.PRE_NONE)
        assert_screen(got, KM.screen(recs, model, k, path, nt.PRE_NONE), "the side word")
        assert got[0].tolist() == [[9, 9, 9, 1, KM.NONE], [9, 9, 0, 0, 1], [0, 0, 0, KM.NONE, KM.NONE]]
        # a uniform mask with a bit at or above n_colors is refused on the host, and nothing changes
        t = to_dev([1, 2])
        assert coloring.lib().ntk_kmer_colors_add_device(kc._h, C.c_void_p(t.data_ptr()), None, 8, 2) == ERR_BAD_ARG
        assert coloring.lib().ntk_kmer_colors_add_device(kc._h, None, None, 1, 2) == ERR_BAD_ARG
        assert kc.stats()["n_keys"] == 5
        # capacity exceeded: lookup and run_device refuse and write nothing
        kc.add_masks(np.arange(100, 120), np.ones(20))
        st = kc.stats()
        assert st["n_dropped"] > 0 and st["n_keys"] == 8 + 1   # every slot, and the side word
        out = torch.full((4,), PATTERN, dtype=torch.int64, device="cuda")
        q = to_dev([0, 1, 2, 3])
        assert coloring.lib().ntk_kmer_colors_lookup_device(kc._h, C.c_void_p(q.data_ptr()), 4, C.c_void_p(out.data_ptr())) == ERR_CAPACITY
        dev, d_off = upload(pack(recs)), to_dev(KM.offsets(recs))
        rows, hits = torch.full((3, 5), PATTERN, dtype=torch.int64, device="cuda"), torch.full((3, 3), PATTERN, dtype=torch.int64, device="cuda")
        p = NL.Params(k, path, nt.PRE_NONE, 0)
        assert coloring.lib().ntk_kmer_colors_run_device(kc._h, C.c_void_p(dev.data_ptr()), None, len(pack(recs)), C.c_void_p(d_off.data_ptr()), 3,
                                                         C.byref(p), C.c_void_p(rows.data_ptr()), C.c_void_p(hits.data_ptr()), None) == ERR_CAPACITY
        torch.cuda.synchronize()
        assert bool((out == PATTERN).all()) and bool((rows == PATTERN).all()) and bool((hits == PATTERN).all())
        with pytest.raises(nt.NtkError) as e:
            kc.lookup([1])
        assert e.value.status == ERR_CAPACITY
        # reset, then reuse
        kc.reset()
        st = kc.stats()
        assert (st["n_keys"], st["n_dropped"], st["n_masked_bits"], st["per_color"]) == (0, 0, 0, [0, 0, 0])
        assert kc.lookup(queries).tolist() == [0] * len(queries)
        kc.add_masks([M64, 9], [4, 1])
        assert kc.lookup([M64, 9, 0]).tolist() == [4, 1, 0] and kc.stats()["n_keys"] == 2


def test_a_chain_longer_than_the_probe_bound_is_dropped(ctx):
    """4097 keys with one home in 8192 slots: the bound of 4096 holds, one occurrence is dropped, and the index refuses to be read."""
    slots = CM.slots_for(6000)
    chain = CM.keys_with_home(100, slots, 32, 4097)
    with nt.KmerColors(32, BITS, 2, 6000, ctx) as kc:
        kc.add_masks(chain[:4096], np.full(4096, 1))
        assert kc.stats()["n_dropped"] == 0 and np.array_equal(kc.lookup(chain), np.array([1] * 4096 + [0], dtype=np.uint64))
        kc.add_masks(chain[4096:], [2])
        st = kc.stats()
        assert (st["n_keys"], st["n_dropped"], st["per_color"]) == (4096, 1, [4096, 0])
        with pytest.raises(nt.NtkError) as e:
            kc.lookup(chain[:1])
        assert e.value.status == ERR_CAPACITY


# ---- 3. record shapes ----------------------------------------------------------------------------------------------------------------------

def _index_of_genome(ctx, genome, k, path, pre, n_colors, seed):
    """An index over the k-mers of the circular genome, every key with a random mask."""
    values = [KM.record_values(_periodic(genome, 0, genome.size + k - 1), k, path, pre)]
    return indexed(ctx, k, path, n_colors, values, seed)


def test_records_of_every_length_around_the_rounds(ctx):
    """k = 21: empty, shorter than k, exactly k, all N, and every length k - 1 .. k + 130 (0 .. 131 windows: the rounds of 64 and their
    seams), each as pure bases and with an N in the middle."""
    k, genome = 21, _genome(0xE0, 500)
    rng = np.random.default_rng(0xE1)
    recs = [b"", b"A", b"ACGT" * 5, _periodic(genome, 3, k), b"N" * 100, b"N" * k]
    for n in range(k - 1, k + 131):
        r = _periodic(genome, int(rng.integers(0, 500)), n)
        recs.append(r)
        holed = bytearray(r)
        holed[n // 2] = ord("N")
        recs.append(bytes(holed))
    buf, off = pack(recs), KM.offsets(recs)
    for path, pre in ((BYTES, nt.PRE_NORMALIZE), (BITS, nt.PRE_NONE)):
        kc, model = _index_of_genome(ctx, genome, k, path, pre, 5, 0xE2)
        with kc:
            want = KM.screen(recs, model, k, path, pre)
            assert set(range(0, 132)) <= set(want[0][:, 0].tolist()) and want[0][:6, 0].tolist() == [0, 0, 0, 1, 0, 0]
            assert want[0][4].tolist() == [0, 0, 0, KM.NONE, KM.NONE] and not want[1][4].any()
            assert_screen(run(kc, upload(buf), len(buf), off, pre), want, path)


def test_long_records_on_both_sides_of_the_threshold(ctx):
    """One record with exactly LONG_RECORD windows (the last the wave kernel takes), one with LONG_RECORD + 1 (the first of
    kc_long_kernel), one of LONG_RECORD * 3 + 5 windows, whose row the waves of many blocks share, and one of N, among short reads."""
    genome, k = _genome(0xE8, 2000), 21
    short = _reads(genome, 0xE9, 40)
    longs = [_periodic(genome, 5, LONG_RECORD + k - 1), _periodic(genome, 700, LONG_RECORD + k), _periodic(genome, 1500, LONG_RECORD * 3 + 5 + k - 1),
             _periodic(genome, 0, LONG_RECORD - 1 + k - 1), b"N" * (LONG_RECORD + 500)]
    recs = short[:10] + [longs[0]] + short[10:20] + [longs[1], longs[2]] + short[20:30] + [longs[3], longs[4]] + short[30:]
    buf, off = pack(recs), KM.offsets(recs)
    for path, pre, n_colors in ((BYTES, nt.PRE_NORMALIZE, 3), (BITS_CANON, nt.PRE_NONE, 64)):
        kc, model = _index_of_genome(ctx, genome, k, path, pre, n_colors, 0xEA)
        with kc:
            want = KM.screen(recs, model, k, path, pre)
            assert {LONG_RECORD - 1, LONG_RECORD, LONG_RECORD + 1, LONG_RECORD * 3 + 5} <= set(want[0][:, 0].tolist())
            assert_screen(run(kc, upload(buf), len(buf), off, pre), want, (path, n_colors))
            assert_screen(run(kc, upload(buf), len(buf), off, pre, single=False), want, (path, n_colors, "no single"))


def test_rows_follow_the_records_when_shuffled(ctx):
    genome, k, path, pre = _genome(0xF0, 4000), 21, BYTES, nt.PRE_NORMALIZE
    recs = _reads(genome, 0xF1, 600) + _reads(_genome(0xF2, 4000), 0xF3, 100) + [_periodic(genome, 0, LONG_RECORD + 3000)]
    kc, _ = _index_of_genome(ctx, genome, k, path, pre, 8, 0xF4)
    order = np.random.default_rng(0xF5).permutation(len(recs))
    shuffled = [recs[i] for i in order]
    with kc:
        a = run(kc, upload(pack(recs)), len(pack(recs)), KM.offsets(recs), pre)
        b = run(kc, upload(pack(shuffled)), len(pack(shuffled)), KM.offsets(shuffled), pre)
    assert_screen(b, tuple(x[order] for x in a), "shuffled")
    assert len({tuple(r) for r in a[1].tolist()}) > 300


# ---- 4. a chunk seam -----------------------------------------------------------------------------------------------------------------------

SEAM = CM.CHUNK
SEAM_KS = (17, 18, 32)   # halos 16 (17 fits it exactly, 18 is one over) and 32
SEAM_MODES = ((BYTES, nt.PRE_NORMALIZE), (BITS, nt.PRE_NONE))


class SeamLayout:
    """One device batch that is filler except for small regions of records around the chunk seam (the manner of
    tests/test_gpu_abundance.py).  The filler between two regions is one giant record of N (its last byte a break byte): its row is
    all-zero without walking it, and a record with no k-mer at all goes through the long-record path."""

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


def test_chunk_seam_record_by_record(ctx):
    """A batch of 64 MiB + 8 KiB whose one seam falls on byte 0, k - 1, k and the break byte of a short record, at k = 17, 18, 32 on the
    byte and the bit path: the record whose windows come from two chunks has the model's rows (each chunk adds its share), so have its
    neighbours, and the fillers have all-zero rows.  A record longer than a chunk takes the same add-per-chunk path and is not run at
    full size."""
    layout = SeamLayout(SEAM + 8192)
    rng = np.random.default_rng(0x5EAD)
    for k in SEAM_KS:
        rec = ACGT[rng.integers(0, 4, k + 25)].tobytes()
        for at in (0, k - 1, k, len(rec)):
            before, after = random_records(9000 + k, 5), random_records(9100 + k, 5)
            start = SEAM - len(pack(before)) - at
            recs, off, where = layout.lay([(start, before + [rec] + after)])
            assert int(off[where[5]]) + at == SEAM
            for path, pre in SEAM_MODES:
                values = [KM.record_values(r, k, path, pre) for r in recs]
                kc, model = indexed(ctx, k, path, 3, values, 0x5EAE + k + at)
                with kc:
                    rows, hits, single = KM.screen_values(values, model)
                    n = len(off) - 1
                    want = (np.zeros((n, 5), np.uint64), np.zeros((n, 3), np.uint64), np.zeros((n, 3), np.uint64))
                    want[0][:, 3:] = KM.NONE
                    want[0][where], want[1][where], want[2][where] = rows, hits, single
                    assert rows[5][0] == 26 and rows[5][1] > 0
                    assert_screen(run(kc, layout.dev, layout.n_bytes, off, pre), want, (k, at, path))
    del layout
    torch.cuda.empty_cache()


# ---- 5. quality, best / second, errors, reuse ----------------------------------------------------------------------------------------------

def test_quality_stream_masks_as_the_table_does(ctx):
    recs = random_records(0xC021)
    buf, off = pack(recs), KM.offsets(recs)
    rng = np.random.default_rng(9)
    qual = rng.integers(33, 75, len(buf)).astype(np.uint8)
    quals = [qual[int(off[i]): int(off[i + 1]) - 1] for i in range(len(recs))]
    dev, dq = upload(buf), upload(qual.tobytes(), fill=0xFF)
    assert quality_masked(buf, qual) != buf
    for path, pre, k in ((BYTES, nt.PRE_NORMALIZE, 21), (BITS, nt.PRE_NONE, 5), (BITS_CANON, nt.PRE_STRIP_RETURNS, 32)):
        values = [KM.record_values(r, k, path, pre) for r in recs]
        kc, model = indexed(ctx, k, path, 4, values, 0xC022 + k)
        with kc:
            want = KM.screen(recs, model, k, path, pre, quals, CUTOFF)
            plain = KM.screen_values(values, model)
            assert not np.array_equal(want[0], plain[0])
            assert_screen(run(kc, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=CUTOFF), want, ("quality", path, k))
            assert_screen(run(kc, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=0), plain, ("cutoff 0", path, k))
            assert_screen(run(kc, dev, len(buf), off, pre), plain, ("no stream", path, k))


def test_best_and_second(ctx):
    """A tie between colours 0 and 5, a tie among all, a single colour, no hit; and a second that trails."""
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    s, t, u, v = (_genome(0xF8 + i, 600) for i in range(4))
    val = lambda g: KM.record_values(_periodic(g, 0, g.size + k - 1), k, path, pre)   # noqa: E731
    model = KM.Index(8)
    with nt.KmerColors(k, path, 8, 4096, ctx) as kc:
        for keys, mask in ((val(s), 1 | 32), (val(t), 255), (val(u), 8), (val(v)[:100], 2), (val(v), 64)):
            kc.add_masks(keys, np.full(keys.size, mask))
            model.add(keys, mask)
        recs = [_periodic(s, 10, 100), _periodic(t, 10, 100), _periodic(u, 10, 100), _periodic(_genome(0xFF, 600), 0, 100),
                _periodic(v, 0, 200), _periodic(s, 0, 80) + b"N" + _periodic(u, 0, 90)]
        want = KM.screen(recs, model, k, path, pre)
        assert want[0][:, 3:].tolist() == [[0, 5], [0, 1], [3, KM.NONE], [KM.NONE, KM.NONE], [6, 1], [3, 0]]
        got = run(kc, upload(pack(recs)), len(pack(recs)), KM.offsets(recs), pre)
        assert_screen(got, want, "best and second")
        assert coloring.classify(got[0], got[1]).tolist() == [0, 0, 3, -1, 6, 3]
        assert coloring.classify(got[0], got[1], min_hits=75).tolist() == [0, 0, 3, -1, 6, -1]
        assert coloring.classify(got[0], got[1], 1, (3, 5)).tolist() == [0, 0, 3, -1, 6, -1]   # 70 of 130 is below three fifths


def _status(kc, dev, n_bytes, d_off, n_records, k, path, pre, flags=0, rows=None, hits=None, single=None, qual=None):
    p = NL.Params(k, path, pre, flags)
    ptr = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())   # noqa: E731
    return coloring.lib().ntk_kmer_colors_run_device(kc._h, ptr(dev), ptr(qual), n_bytes, ptr(d_off), n_records, C.byref(p), ptr(rows), ptr(hits),
                                                     ptr(single))


def test_errors(ctx):
    recs = random_records(0xC031, 40)
    buf, off = pack(recs), KM.offsets(recs)
    dev, d_off = upload(buf), to_dev(off)
    n, k, path, pre = len(recs), 21, BITS_CANON, nt.PRE_NORMALIZE
    rows, hits = torch.full((n, 5), PATTERN, dtype=torch.int64, device="cuda"), torch.full((n, 3), PATTERN, dtype=torch.int64, device="cuda")
    single = torch.full((n, 3), PATTERN, dtype=torch.int64, device="cuda")
    untouched = lambda: bool((rows == PATTERN).all()) and bool((hits == PATTERN).all()) and bool((single == PATTERN).all())   # noqa: E731
    values = [KM.record_values(r, k, path, pre) for r in recs]
    kc, model = indexed(ctx, k, path, 3, values, 0xC032)
    with kc:
        args, out = (kc, dev, len(buf), d_off, n), dict(rows=rows, hits=hits, single=single)
        assert _status(*args, 20, path, pre, **out) == ERR_BAD_ARG                       # k is not the handle's
        assert _status(*args, 33, path, pre, **out) == ERR_BAD_ARG
        assert _status(*args, k, BITS, pre, **out) == ERR_BAD_ARG                        # nor the path
        assert _status(*args, k, path, pre, flags=5, **out) == ERR_BAD_ARG               # a minimizer window
        assert _status(*args, k, path, pre, flags=NL.FLAG_RESET, **out) == ERR_BAD_ARG
        assert _status(*args, k, path, 4, **out) == ERR_BAD_ARG                          # no such pre-step
        assert _status(*args, k, path, pre, rows=None, hits=hits) == ERR_BAD_ARG         # null outputs, sizes not zero
        assert _status(*args, k, path, pre, rows=rows, hits=None) == ERR_BAD_ARG
        assert _status(kc, None, len(buf), d_off, n, k, path, pre, **out) == ERR_BAD_ARG
        assert _status(kc, dev, len(buf), None, n, k, path, pre, **out) == ERR_BAD_ARG
        assert _status(kc, dev.data_ptr() + 8, len(buf) - 8, d_off, n, k, path, pre, **out) == ERR_BAD_ARG    # misaligned pointers
        assert _status(*args, k, path, pre, qual=dev.data_ptr() + 4, **out) == ERR_BAD_ARG
        assert _status(kc, dev, len(buf), d_off.data_ptr() + 4, n, k, path, pre, **out) == ERR_BAD_ARG
        assert _status(*args, k, path, pre, rows=rows.data_ptr() + 4, hits=hits) == ERR_BAD_ARG
        assert _status(*args, k, path, pre, rows=rows, hits=hits, single=single.data_ptr() + 4) == ERR_BAD_ARG
        assert untouched()
        # nothing to do: NTK_OK, nothing touched, whatever the pointers
        assert _status(kc, dev, len(buf), d_off, 0, k, path, pre, **out) == 0
        assert _status(kc, None, 0, None, 0, k, path, pre) == 0
        assert _status(kc, dev, 0, d_off, n, k, path, pre, **out) == 0
        assert untouched()
        empty = kc.run_device(dev, len(buf), d_off, 0, pre)
        assert tuple(empty[0].shape) == (0, 5) and tuple(empty[1].shape) == (0, 3) and kc.run_records([], pre)[1].shape == (0, 3)
        # and the call that is right
        assert _status(*args, k, path, pre, **out) == 0
        view = lambda t: t.cpu().numpy().view(np.uint64)   # noqa: E731
        assert_screen((view(rows), view(hits), view(single)), KM.screen_values(values, model), "after the errors")
    with nt.KmerColors(21, BYTES, 3, 100, ctx) as kc:   # un-normalised byte-path input, as for the table
        rows.fill_(PATTERN)
        for bad_pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):
            assert _status(kc, dev, len(buf), d_off, n, 21, BYTES, bad_pre, rows=rows, hits=hits) == ERR_UNSUPPORTED
        assert bool((rows == PATTERN).all())
        with pytest.raises(nt.NtkError) as e:
            kc.run_device(dev, len(buf), d_off, n, nt.PRE_NONE)
        assert e.value.status == ERR_UNSUPPORTED
    lib, h = coloring.lib(), C.c_void_p()
    assert lib.ntk_kmer_colors_create(None, 21, 0, 3, 100, C.byref(h)) == ERR_BAD_ARG
    assert lib.ntk_kmer_colors_create(ctx._h, 21, 0, 65, 100, C.byref(h)) == ERR_BAD_ARG and not h.value
    assert lib.ntk_kmer_colors_create(ctx._h, 33, 0, 3, 100, C.byref(h)) == 1 and not h.value


def test_repeated_calls_grow_shrink_and_release(ctx):
    """stats.device_bytes follows the header's memory statement: the index, then the scratch of the longest batch so far, until release."""
    genome, k, path, pre = _genome(0xC040, 5000), 21, BYTES, nt.PRE_NORMALIZE
    reads = _reads(genome, 0xC041, 3000)
    kc, model = _index_of_genome(ctx, genome, k, path, pre, 6, 0xC042)
    sizes = (50, 3000, 700, 1, 2500)
    want = {n: KM.screen(reads[:n], model, k, path, pre) for n in sizes}
    with kc:
        slots = kc.stats()["slots"]
        assert kc.stats()["device_bytes"] == KM.device_bytes(slots, 0, k)
        for release in (False, True):
            longest = 0
            for n in sizes:
                buf = pack(reads[:n])
                assert_screen(run(kc, upload(buf), len(buf), KM.offsets(reads[:n]), pre), want[n], (release, n))
                longest = len(buf) if release else max(longest, len(buf))
                assert kc.stats()["device_bytes"] == KM.device_bytes(slots, longest, k), (release, n)
                if release:
                    kc.release()
                    assert kc.stats()["device_bytes"] == KM.device_bytes(slots, 0, k)
            kc.release()
        kc.release()   # nothing left to free
        launches = kc.stats()["n_launches"]
        assert kc.stats()["n_launches"] == launches + 1   # the census pass of stats itself
        assert_stats(kc, model, "after the calls")


# ---- 6. golden data and the example --------------------------------------------------------------------------------------------------------

def _golden_records(name):
    return [r.raw_seq for r in nt.parse_fastx_file(os.path.join(GOLDEN, name))]


def _packed(ctx, recs, pre):
    """What the packer makes of each record."""
    b = nt.Batch(ctx, sum(len(r) for r in recs) + len(recs), len(recs))
    for r in recs:
        assert b.append(r, pre)
    seq, off = b.buffers()
    buf, off = seq.tobytes(), np.array(off, copy=True)
    b.release()
    return [buf[int(off[i]): int(off[i + 1]) - 1] for i in range(len(recs))]


def test_from_sets_end_to_end_on_golden_data(ctx):
    """Colour 0 is 28S.fasta, colour 1 the first reads of PRJNA271013_head.fq; the rest of the reads, and the reference itself, are
    screened against the model."""
    k, path, pre = 21, BYTES, nt.PRE_NORMALIZE
    ref, reads = _golden_records("28S.fasta"), _golden_records("PRJNA271013_head.fq")
    half = len(reads) // 2
    sets, model = [], KM.Index(2)
    for color, src in enumerate((ref, reads[:half])):
        with nt.KmerTable(k, path, sum(len(r) for r in src) + 16, ctx) as t:
            t.count_records(src, pre)
            sets.append(nt.KmerSet.from_table(t))
        for r in _packed(ctx, src, pre):
            model.add(KM.record_values(r, k, path, pre), 1 << color)
    rest = reads[half:] + ref
    with nt.KmerColors.from_sets(sets) as kc:
        st = assert_stats(kc, model, "golden")
        assert st["n_keys"] <= len(sets[0]) + len(sets[1]) and st["per_color"] == [len(sets[0]), len(sets[1])]
        want = KM.screen(_packed(ctx, rest, pre), model, k, path, pre)
        assert want[0][:, 0].sum() > 1000 and want[1][-len(ref):, 0].sum() == want[0][-len(ref):, 0].sum() > 0
        assert_screen(kc.run_records(rest, pre), want, "golden")


def test_screen_reads_cli(ctx, tmp_path):
    exe = os.path.join(ROOT, "examples", "screen_reads")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    a, b, c = _genome(0xCC0, 3000), _genome(0xCC1, 3000), _genome(0xCC2, 3000)
    b[:1000] = a[:1000]
    reads = _reads(a, 0xCC3, 100) + _reads(b, 0xCC4, 100) + _reads(c, 0xCC5, 60) + _reads(_genome(0xCC6, 3000), 0xCC7, 20) + [b"A", b"N" * 50]
    names = [f"read{i}" for i in range(len(reads))]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (n.encode(), r, b"I" * len(r)) for n, r in zip(names, reads)))
    refs = []
    for i, g in enumerate((a, b, c)):
        fa = tmp_path / f"ref{i}.fa"
        fa.write_bytes(b">g%d\n%s\n>tail\n%s\n" % (i, g.tobytes(), g[:100].tobytes()))
        refs += ["-r", str(fa)]
    pre = nt.PRE_NORMALIZE
    for k, extra, min_hits in ((21, [], 1), (15, ["-m", "120"], 120)):
        model = KM.Index(3)
        for i, g in enumerate((a, b, c)):
            for rec in (g.tobytes(), g[:100].tobytes()):
                model.add(KM.record_values(rec, k, BYTES, pre), 1 << i)
        rows, hits, _ = KM.screen(reads, model, k, BYTES, pre)
        want = "".join(KM.cli_line(n, row, h) + "\n" for n, row, h in zip(names, rows, hits)) + KM.cli_summary(rows, hits, min_hits)
        r = subprocess.run([exe, "-k", str(k), *extra, *refs, str(fq)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (k, extra)
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 2
    assert subprocess.run([exe, str(fq)], capture_output=True, timeout=60).returncode == 2
