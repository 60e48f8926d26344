"""Per-record MinHash sketches (include/needletail_amd_record_minhash.h, needletail_amd.RecordMinHash) on a real MI355X.

Truth for every record: tests/_record_minhash_model.py - tests/_minhash_model.sketch of the k-mers the oracle's literal iterators emit
for that record alone.  Every comparison is `np.array_equal` on the offsets, the hashes, the counts and n_windows; there is no tolerance
anywhere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import record_minhashing as RM  # noqa: E402
import _minhash_model as M  # noqa: E402
import _record_minhash_model as R  # noqa: E402
import _sketch_model as S  # noqa: E402
from _count_helpers import CUTOFF, PATH_PRES, pack, random_records, upload  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BYTES, BITS, BITS_CANON = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS, nt.PATH_BITS_CANONICAL
KS = (1, 5, 21, 32)
KINDS = [dict(num=1), dict(num=16), dict(num=1000), dict(scaled=1), dict(scaled=7), dict(scaled=1000)]
ERR_BAD_K, ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 1, 2, 5, 6
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK = 64 << 20   # kChunkBases of ntk_chunks.hpp
M64 = (1 << 64) - 1


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


def run(rmh, dev, n_bytes, off, pre, **kw):
    rmh.run_device(dev, n_bytes, dev_offsets(off), len(off) - 1, pre, **kw)
    return rmh.sketches()


def assert_csr(got, want, what):
    for name, g, w in zip(("offsets", "n_windows", "hashes", "counts"), got, want):
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = int(np.nonzero(g != w)[0][0])
            raise AssertionError((what, name, f"first difference at {bad}", int(g[bad]), int(w[bad])))


def random_bases(rng, n) -> bytes:
    return ACGT[rng.integers(0, 4, n)].tobytes()


def sketched(ctx, records, k, path, pre, kind, **create):
    """(csr, stats) of one run over the packed records."""
    buf, off = pack(records), R.offsets(records)
    with nt.RecordMinHash(k, path, ctx=ctx, **kind, **create) as rmh:
        got = run(rmh, upload(buf), len(buf), off, pre)
        return got, rmh.stats()


# ---- 1. random records across kinds ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,pre", PATH_PRES)
def test_random_records_match_the_model(ctx, path, pre):
    """160 records (empty, shorter than k, with N, U and IUPAC letters, low-complexity) x k x {num 1, 16, 1000, scaled 1, 7, 1000}."""
    recs = random_records(0x4D48)
    buf, off = pack(recs), R.offsets(recs)
    dev = upload(buf)
    for k in KS:
        values = [R.record_values(r, k, path, pre) for r in recs]
        for kind in KINDS:
            with nt.RecordMinHash(k, path, ctx=ctx, **kind) as rmh:
                want = R.csr(values, **kind)
                assert_csr(run(rmh, dev, len(buf), off, pre), want, (path, pre, k, kind))
                st = rmh.stats()
                assert st["n_records"] == len(recs) and st["n_entries"] == want[2].size and st["n_windows"] == int(want[1].sum()), st
                assert (st["k"], st["path"], st["num"], st["scaled"]) == (k, path, kind.get("num", 0), kind.get("scaled", 0))
                assert st["buffer_entries"] == RM.BUFFER_DEFAULT and st["n_rounds"] >= 1 and st["device_bytes"] > 0
                if k == 21 and kind == KINDS[1]:   # the packer's route: the same records through ntk_batch_append, its offsets
                    rmh.run_records(recs, pre)
                    assert_csr(rmh.sketches(), want, ("records", path, pre))


# ---- 2. against KmerMinHash -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [dict(num=16), dict(scaled=7)], ids=["num16", "scaled7"])
def test_eight_records_equal_kmer_minhash_on_each_alone(ctx, kind):
    recs = [r for r in random_records(0x4D48) if len(r) > 60][:8]
    assert len(recs) == 8
    for k, path, pre in ((21, BYTES, nt.PRE_NORMALIZE), (32, BITS, nt.PRE_NONE), (5, BITS_CANON, nt.PRE_NORMALIZE_IUPAC)):
        (offsets, windows, hashes, counts), _ = sketched(ctx, recs, k, path, pre, kind)
        with nt.KmerMinHash(k, path, ctx=ctx, **kind) as mh:
            for r, rec in enumerate(recs):
                mh.reset()
                mh.add_records([rec], pre)
                h, c = mh.hashes()
                lo, hi = int(offsets[r]), int(offsets[r + 1])
                assert np.array_equal(hashes[lo:hi], h) and np.array_equal(counts[lo:hi], c), (k, path, r)
                assert int(windows[r]) == mh.stats()["n_windows"]


# ---- 3. the all-pass seam ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,path,pre", [(1, BITS, nt.PRE_NONE), (21, BYTES, nt.PRE_NORMALIZE), (32, BITS_CANON, nt.PRE_NONE)])
def test_records_on_both_sides_of_the_all_pass_length(ctx, k, path, pre):
    """num = 16: records of ALLPASS * 16 + d candidate windows, d = -1, 0, +1, +64 - all-pass and guessed records in one batch."""
    rng = np.random.default_rng(0xA11 + k)
    num = 16
    recs = [random_bases(rng, RM.ALLPASS * num + d + k - 1) for _ in range(6) for d in (-1, 0, 1, 64)]
    got, st = sketched(ctx, recs, k, path, pre, dict(num=num))
    want = R.sketches(recs, k, path, pre, num=num)
    assert want[1].tolist() == [RM.ALLPASS * num + d for _ in range(6) for d in (-1, 0, 1, 64)]
    assert_csr(got, want, (k, path))
    assert st["n_redone"] == 0


# ---- 4. retry ---------------------------------------------------------------------------------------------------------------------------

def test_repetitive_records_are_retried_until_exact(ctx):
    """num = 64 and three records of more than ALLPASS * 64 + 1000 windows in one batch: period 50 (fewer than 64 distinct k-mers), poly-A
    (one hash, its count the record's windows) and random (accepted at once)."""
    k, num = 21, 64
    rng = np.random.default_rng(0x3E7)
    L = RM.ALLPASS * num + 1500 + k
    periodic = (random_bases(rng, 50) * (L // 50 + 1))[:L]
    recs = [periodic, b"A" * L, random_bases(rng, L)]
    got, st = sketched(ctx, recs, k, BYTES, nt.PRE_NORMALIZE, dict(num=num))
    want = R.sketches(recs, k, BYTES, nt.PRE_NORMALIZE, num=num)
    sizes = np.diff(want[0]).tolist()
    assert sizes[0] < num and sizes[1] == 1 and sizes[2] == num and int(want[3][int(want[0][1])]) == L - k + 1
    assert_csr(got, want, "retry")
    assert st["n_retried_records"] >= 2 and st["n_rounds"] >= 2, st
    alone, st1 = sketched(ctx, recs[2:], k, BYTES, nt.PRE_NORMALIZE, dict(num=num))
    assert st1["n_rounds"] == 1 and st1["n_retried_records"] == 0
    assert np.array_equal(alone[2], got[2][int(got[0][2]):]) and np.array_equal(alone[3], got[3][int(got[0][2]):])


# ---- 5. buffer overflow -----------------------------------------------------------------------------------------------------------------

def test_a_full_buffer_redoes_the_launch_and_drops_nothing(ctx):
    rng = np.random.default_rng(0x0F)
    recs = [random_bases(rng, 500) for _ in range(40)]
    got, st = sketched(ctx, recs, 21, BYTES, nt.PRE_NORMALIZE, dict(scaled=1), buffer_entries=RM.BUFFER_MIN)
    assert_csr(got, R.sketches(recs, 21, BYTES, nt.PRE_NORMALIZE, scaled=1), "overflow")
    assert st["n_redone"] > 0 and st["buffer_entries"] == RM.BUFFER_MIN, st


# ---- 6. extreme hashes ------------------------------------------------------------------------------------------------------------------

def _unmix(h: int) -> int:
    """The inverse of fmix64."""
    inv = lambda c: pow(c, -1, 1 << 64)
    h ^= h >> 33
    h = h * inv(0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    h = h * inv(0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    return h


def _kmer_of(value: int, k: int = 32) -> bytes:
    return bytes(b"ACGT"[(value >> (2 * (k - 1 - i))) & 3] for i in range(k))


@pytest.mark.parametrize("kind", [dict(num=1), dict(scaled=1)], ids=["num1", "scaled1"])
def test_hashes_0_and_all_ones_are_kept(ctx, kind):
    keys = [_unmix(0) ^ M.XOR, _unmix(M64) ^ M.XOR]
    assert S.hash_keys(np.array(keys, dtype=np.uint64)).tolist() == [0, M64]
    rng = np.random.default_rng(6)
    recs = [_kmer_of(keys[0]), random_bases(rng, 40), _kmer_of(keys[1])]
    got, _ = sketched(ctx, recs, 32, BITS, nt.PRE_NONE, kind)
    assert_csr(got, R.sketches(recs, 32, BITS, nt.PRE_NONE, **kind), kind)
    offsets, windows, hashes, counts = got
    assert int(hashes[0]) == 0 and int(hashes[-1]) == M64 and int(counts[0]) == int(counts[-1]) == 1
    assert windows.tolist() == [1, 9, 1] and int(offsets[1]) == 1 and int(offsets[3] - offsets[2]) == 1


# ---- 7. the chunk seam ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seam_batch():
    """64 Mi + 8192 bytes of N on the device; the tests write records around the seam and put the N back."""
    n = CHUNK + 8192
    t = torch.full((n + 64,), ord("N"), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t, n


@pytest.mark.parametrize("k,path,pre", [(21, BYTES, nt.PRE_NORMALIZE), (32, BITS, nt.PRE_NONE)])
def test_records_around_the_chunk_seam(ctx, seam_batch, k, path, pre):
    """A 4 kb record ending at the seam, one starting at it, and one straddling it with 1, k - 1, k, 16 and 33 bases before it; the N
    around them emit nothing, so the model sees the record between two empty ones."""
    dev, n = seam_batch
    rng = np.random.default_rng(0x5EA + k)
    rec = random_bases(rng, 4096)
    values = [R.record_values(r, k, path, pre) for r in (b"", rec, b"")]
    wants = {name: R.csr(values, **kind) for name, kind in (("num", dict(num=64)), ("scaled", dict(scaled=7)))}
    starts = [CHUNK - 4097, CHUNK] + [CHUNK - d for d in (1, k - 1, k, 16, 33)]
    with nt.RecordMinHash(k, path, num=64, ctx=ctx) as by_num, nt.RecordMinHash(k, path, scaled=7, ctx=ctx) as by_scaled:
        for start in starts:
            piece = torch.from_numpy(np.frombuffer(rec + b"\n", dtype=np.uint8).copy()).cuda()
            dev[start:start + 4097] = piece
            torch.cuda.synchronize()
            off = np.array([0, start, start + 4097, n], dtype=np.uint64)
            for name, rmh in (("num", by_num), ("scaled", by_scaled)):
                assert_csr(run(rmh, dev, n, off, pre), wants[name], (name, k, start - CHUNK))
            dev[start:start + 4097] = ord("N")
        torch.cuda.synchronize()
        assert by_num.stats()["n_rounds"] >= 2   # the N records hold nothing at any threshold


# ---- 8. many short records --------------------------------------------------------------------------------------------------------------

def test_twenty_thousand_short_records(ctx):
    """20 000 x 150 bp, num = 1000: every sketch is the record's whole set of distinct k-mers; shuffled, the rows follow the records."""
    k, num, pre = 21, 1000, nt.PRE_NORMALIZE
    rng = np.random.default_rng(0x20000)
    bases = ACGT[rng.integers(0, 4, (20_000, 150))]
    recs = [row.tobytes() for row in bases]
    # the oracle once, over the packed batch: a window never spans a break byte, so record r's k-mers are the batch's 130 r .. 130 r + 129
    values = R.record_values(pack(recs)[:-1], k, BYTES, pre).reshape(20_000, 130)
    assert np.array_equal(values[7], R.record_values(recs[7], k, BYTES, pre))
    order = rng.permutation(20_000)
    with nt.RecordMinHash(k, BYTES, num=num, ctx=ctx) as rmh:
        for rows in (np.arange(20_000), order):
            batch = [recs[i] for i in rows]
            buf = pack(batch)
            want = R.csr(list(values[rows]), num=num)
            assert_csr(run(rmh, upload(buf), len(buf), R.offsets(batch), pre), want, "short records")
            assert np.array_equal(np.diff(want[0]), [np.unique(v).size for v in values[rows]])
        assert rmh.stats()["n_rounds"] == 1


# ---- 9. quality masking -----------------------------------------------------------------------------------------------------------------

def test_quality_stream_masks_as_the_sketch_does(ctx):
    recs = random_records(0x9A1)
    buf, off = pack(recs), R.offsets(recs)
    rng = np.random.default_rng(0x9A2)
    qual = rng.integers(33, 75, len(buf)).astype(np.uint8)
    quals = [qual[int(off[i]): int(off[i + 1]) - 1] for i in range(len(recs))]
    dev, dq = upload(buf), upload(qual.tobytes(), fill=0xFF)
    for k, path, pre in ((21, BYTES, nt.PRE_NORMALIZE), (11, BITS_CANON, nt.PRE_NONE)):
        for kind in (dict(num=16), dict(scaled=3)):
            want = R.sketches(recs, k, path, pre, quals=quals, cutoff=CUTOFF, **kind)
            plain = R.sketches(recs, k, path, pre, **kind)
            assert not np.array_equal(want[1], plain[1])
            with nt.RecordMinHash(k, path, ctx=ctx, **kind) as rmh:
                assert_csr(run(rmh, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=CUTOFF), want, ("quality", k, kind))
                assert_csr(run(rmh, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=0), plain, ("cutoff 0", k, kind))
                assert_csr(run(rmh, dev, len(buf), off, pre), plain, ("no stream", k, kind))


# ---- 10. handle reuse -------------------------------------------------------------------------------------------------------------------

def test_each_read_returns_its_own_run(ctx):
    rng = np.random.default_rng(0x10)
    large = [random_bases(rng, int(n)) for n in rng.integers(0, 3000, 300)]
    small = [random_bases(rng, 100), b"", random_bases(rng, 30)]
    k, pre = 21, nt.PRE_NORMALIZE
    for kind in (dict(num=16), dict(scaled=2)):
        with nt.RecordMinHash(k, BYTES, ctx=ctx, **kind) as rmh:
            assert rmh.stats()["n_rounds"] == 0 and rmh.sketches()[0].tolist() == [0]
            for batch in (large, small):
                rmh.run_records(batch, pre)
                assert_csr(rmh.sketches(), R.sketches(batch, k, BYTES, pre, **kind), ("reuse", kind, len(batch)))
            rmh.trim()
            assert rmh.stats()["device_bytes"] == 0 and rmh.stats()["n_records"] == 0 and rmh.sketches()[2].size == 0
            rmh.run_records(large[::-1], pre)
            assert_csr(rmh.sketches(), R.sketches(large[::-1], k, BYTES, pre, **kind), ("after trim", kind))
            rmh.run_records([], pre)
            assert rmh.stats()["n_records"] == 0 and rmh.sketches()[0].tolist() == [0]


# ---- 11. errors -------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_change_nothing(ctx):
    lib = RM.lib()
    h = C.c_void_p()
    create = lambda *a: lib.ntk_record_minhash_create(ctx._h, *a, C.byref(h))
    assert create(33, BYTES, 16, 0, 0) == ERR_BAD_K and create(0, BYTES, 16, 0, 0) == ERR_BAD_K and create(64, BITS, 16, 0, 0) == ERR_BAD_K
    assert create(21, 3, 16, 0, 0) == ERR_BAD_ARG
    assert create(21, BYTES, 16, 7, 0) == ERR_BAD_ARG and create(21, BYTES, 0, 0, 0) == ERR_BAD_ARG
    assert create(21, BYTES, RM.MAX_NUM + 1, 0, 0) == ERR_BAD_ARG
    assert create(21, BYTES, 16, 0, RM.BUFFER_MIN - 1) == ERR_BAD_ARG and create(21, BYTES, 16, 0, RM.BUFFER_MAX + 1) == ERR_BAD_ARG
    assert not h.value
    assert lib.ntk_record_minhash_create(None, 21, BYTES, 16, 0, 0, C.byref(h)) == ERR_BAD_ARG
    assert lib.ntk_record_minhash_create(ctx._h, 21, BYTES, 16, 0, 0, None) == ERR_BAD_ARG

    rng = np.random.default_rng(0x11)
    recs = [random_bases(rng, 300) for _ in range(5)]
    buf, off = pack(recs), R.offsets(recs)
    dev, d_off = upload(buf), dev_offsets(off)
    want = R.sketches(recs, 21, BYTES, nt.PRE_NORMALIZE, num=16)
    with nt.RecordMinHash(21, BYTES, num=16, ctx=ctx) as rmh:
        assert_csr(run(rmh, dev, len(buf), off, nt.PRE_NORMALIZE), want, "before")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        call = lambda p, seq=ptr(dev), qual=None, n=len(buf), o=ptr(d_off), nr=5: lib.ntk_record_minhash_run_device(
            rmh._h, seq, qual, n, o, nr, C.byref(p) if p is not None else None)
        P = nt._lib.Params
        good = P(21, BYTES, nt.PRE_NORMALIZE, 0)
        assert call(None) == ERR_BAD_ARG
        assert call(P(20, BYTES, nt.PRE_NORMALIZE, 0)) == ERR_BAD_ARG and call(P(21, BITS, nt.PRE_NORMALIZE, 0)) == ERR_BAD_ARG
        assert call(P(21, BYTES, nt.PRE_NORMALIZE, 5)) == ERR_BAD_ARG and call(P(21, BYTES, nt.PRE_NORMALIZE, 1 << 16)) == ERR_BAD_ARG
        assert call(P(21, BYTES, 4, 0)) == ERR_BAD_ARG
        assert call(P(21, BYTES, nt.PRE_NONE, 0)) == ERR_UNSUPPORTED and call(P(21, BYTES, nt.PRE_STRIP_RETURNS, 0)) == ERR_UNSUPPORTED
        assert call(good, seq=C.c_void_p(dev.data_ptr() + 1)) == ERR_BAD_ARG and call(good, seq=None) == ERR_BAD_ARG
        assert call(good, qual=C.c_void_p(dev.data_ptr() + 8)) == ERR_BAD_ARG
        assert call(good, o=None) == ERR_BAD_ARG and call(good, o=C.c_void_p(d_off.data_ptr() + 4)) == ERR_BAD_ARG
        assert call(good, nr=1 << 32) == ERR_BAD_ARG
        assert lib.ntk_record_minhash_run_device(None, ptr(dev), None, len(buf), ptr(d_off), 5, C.byref(good)) == ERR_BAD_ARG
        assert_csr(rmh.sketches(), want, "after the refused calls")   # the held result stayed

        # read: a capacity one too small answers the size and writes nothing
        total = int(want[0][-1])
        n = C.c_uint64(0)
        offsets, windows = np.full(6, 77, dtype=np.uint64), np.full(5, 77, dtype=np.uint64)
        hashes, counts = np.full(total, 77, dtype=np.uint64), np.full(total, 77, dtype=np.uint64)
        read = lambda cap: lib.ntk_record_minhash_read(rmh._h, offsets.ctypes.data, windows.ctypes.data, hashes.ctypes.data, counts.ctypes.data,
                                                       cap, C.byref(n))
        assert read(total - 1) == ERR_CAPACITY and n.value == total
        assert all((a == 77).all() for a in (offsets, windows, hashes, counts))
        n.value = 0
        assert lib.ntk_record_minhash_read(rmh._h, None, None, None, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == total
        assert lib.ntk_record_minhash_read(rmh._h, offsets.ctypes.data, None, None, None, 1, C.byref(n)) == ERR_BAD_ARG
        assert lib.ntk_record_minhash_read(rmh._h, offsets.ctypes.data, None, hashes.ctypes.data, counts.ctypes.data, total, None) == ERR_BAD_ARG
        assert read(total) == 0 and n.value == total
        assert_csr((offsets, windows, hashes, counts), want, "read")
        assert lib.ntk_record_minhash_stats(rmh._h, None) == ERR_BAD_ARG and lib.ntk_record_minhash_trim(None) == ERR_BAD_ARG
        lib.ntk_record_minhash_destroy(None)

        # an offset beyond n_bytes reads as n_bytes; an empty batch is NTK_OK and holds empty sketches
        beyond = off.copy()
        beyond[-1] = len(buf) + 1000
        assert_csr(run(rmh, dev, len(buf), beyond, nt.PRE_NORMALIZE), want, "offset beyond the batch")
        assert call(good, n=0) == 0
        assert [a.tolist() for a in rmh.sketches()] == [[0] * 6, [0] * 5, [], []]
        assert call(good, nr=0) == 0 and rmh.stats()["n_records"] == 0
        assert_csr(run(rmh, dev, len(buf), off, nt.PRE_NORMALIZE), want, "after everything")


# ---- 12. into the set -------------------------------------------------------------------------------------------------------------------

def test_record_sketches_go_into_a_set(ctx):
    """32 mutated copies of one 20 kb genome, num = 256: the set's Jaccard matrix is the model's compare, pair by pair."""
    rng = np.random.default_rng(0x12)
    genome = ACGT[rng.integers(0, 4, 20_000)]
    recs = []
    for i in range(32):
        g = genome.copy()
        hit = rng.random(g.size) < 0.002 * i
        g[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        recs.append(g.tobytes())
    k, num, pre = 21, 256, nt.PRE_NORMALIZE
    with nt.RecordMinHash(k, BYTES, num=num, ctx=ctx) as rmh, nt.MinHashSet(True, ctx) as s:
        rmh.run_records(recs, pre)
        offsets, _, hashes, counts = rmh.sketches()
        assert_csr(rmh.sketches(), R.sketches(recs, k, BYTES, pre, num=num), "genomes")
        assert s.add_record_sketches(rmh) == range(0, 32) and len(s) == 32
        assert (s.k, s.path, s.num, s.scaled) == (k, BYTES, num, 0)
        part = lambda a, r: a[int(offsets[r]):int(offsets[r + 1])]
        assert all(np.array_equal(s.sketch(r)[0], part(hashes, r)) and np.array_equal(s.sketch(r)[1], part(counts, r)) for r in (0, 31))
        want = np.zeros((32, 32))
        for a in range(32):
            for b in range(32):
                c = M.compare(part(hashes, a), part(counts, a), part(hashes, b), part(counts, b), num)
                want[a, b] = c["n_shared"] / c["n_union"]
        assert np.array_equal(s.jaccard_matrix(), want) and want[0, 0] == 1.0 and 0.0 < want[0, 31] < want[0, 1] < 1.0
        assert s.add_record_sketches(rmh) == range(32, 64)
        with nt.RecordMinHash(20, BYTES, num=num, ctx=ctx) as other_k, nt.RecordMinHash(k, BYTES, scaled=5, ctx=ctx) as other_kind:
            for bad in (other_k, other_kind):
                with pytest.raises(nt.NtkError) as e:
                    s.add_record_sketches(bad)
                assert e.value.status == ERR_BAD_ARG
        assert len(s) == 64


# ---- 13. the example --------------------------------------------------------------------------------------------------------------------

def test_sketch_records_example(ctx):
    exe = os.path.join(ROOT, "examples", "sketch_records")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    fasta = os.path.join(GOLDEN, "28S.fasta")
    records = list(nt.parse_fastx_file(fasta))
    names = [re.split(r"[ \t]", r.id)[0] for r in records]
    k, pre = 21, nt.PRE_NORMALIZE
    for args, kind in ((["-n", "200"], dict(num=200)), (["-s", "4"], dict(scaled=4))):
        with nt.RecordMinHash(k, BYTES, ctx=ctx, **kind) as rmh, nt.MinHashSet(False, ctx) as s:
            rmh.run_records([r.raw_seq for r in records], pre)
            offsets, windows, _, _ = rmh.sketches()
            s.add_record_sketches(rmh)
            lines = [f"{names[r]}\t{int(windows[r])}\t{int(offsets[r + 1] - offsets[r])}" for r in range(len(records))]
            matrix = [[float(f"{v:.6f}") for v in row] for row in s.mash_distance_matrix().tolist()]
        assert int(windows.sum()) > 1000
        r = subprocess.run([exe, "-k", str(k), *args, fasta], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == lines
        r = subprocess.run([exe, "-k", str(k), *args, "-m", fasta], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert out[:len(lines)] == lines
        assert [[float(x) for x in line.split("\t")] for line in out[len(lines):]] == matrix
    assert subprocess.run([exe, "-k", "21", fasta], capture_output=True, timeout=60).returncode == 2   # neither -n nor -s
