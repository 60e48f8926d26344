"""The device count table (include/needletail_amd_count.h, needletail_amd.KmerTable) on a real MI355X.

"The oracle's counts" below: the oracle's literal iterators (bit_kmers_arrays / canonical_kmers_arrays) -> packed values ->
numpy.unique(return_counts=True) (tests/_count_helpers.py).  On inputs too large for that, the table is held against the reduce face
on the same bytes (n_total, ACC_SUM, ACC_HIST), which the suite already checks against the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import counting  # noqa: E402
from _count_helpers import (CUTOFF, M64, PATH_PRES, assert_items, device_items, oracle_items, pack, random_records,  # noqa: E402
                            upload)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (1, 2, 4, 11, 21, 31, 32)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def check_against_reduce(ctx, table, dev, n_bytes, k, path, pre, n_bins=16384):
    """Σ counts = n_total, Σ key·count = ACC_SUM, counts folded by the leading six bases = ACC_HIST, spectrum sums."""
    ctx.accum_reset()
    ctx.reduce_device(dev, n_bytes, k, path, pre)
    r = ctx.accum_read()
    st = table.stats()
    assert st["n_dropped"] == 0 and st["n_total"] == r["n_total"], (st, r["n_total"])
    keys, counts = device_items(table)
    assert keys.numel() == st["n_distinct"]
    assert int(counts.sum()) == r["n_total"]
    assert int((keys * counts).sum()) & M64 == r["sum"]
    if keys.numel() > 1:
        u = keys ^ (-(1 << 63))   # unsigned order as signed
        assert bool((u[1:] > u[:-1]).all()), "keys not ascending"
    shift = 2 * k - 12 if k >= 6 else 0
    hist = torch.zeros(4096, dtype=torch.int64, device="cuda")
    hist.scatter_add_(0, (keys >> shift) & 4095, counts)
    assert np.array_equal(hist.cpu().numpy().astype(np.uint64), r["hist"])
    h = table.spectrum(n_bins)
    assert h[0] == 0 and int(h.sum()) == st["n_distinct"]
    if h[-1] == 0:
        assert int((np.arange(n_bins, dtype=np.uint64) * h).sum()) == st["n_total"]
    del keys, counts, hist
    return r


# ---- exact against the oracle ----------------------------------------------------------------------------------------------------

def test_random_records_match_the_oracle(ctx):
    recs = random_records(0xC0017)
    buf = pack(recs)
    dev = upload(buf)
    for path, pre in PATH_PRES:
        for k in KS:
            with nt.KmerTable(k, path, len(buf), ctx) as t:
                t.count_device(dev, len(buf), pre)
                assert_items(t, oracle_items(buf, k, path, pre), (path, pre, k))
                # the packer route: the same records through ntk_batch_append
                t.reset()
                t.count_records(recs, pre)
                assert_items(t, oracle_items(buf, k, path, pre), ("records", path, pre, k))


def test_quality_stream_matches_the_oracle(ctx):
    buf = pack(random_records(0xC0018))
    rng = np.random.default_rng(5)
    qual = rng.integers(33, 75, len(buf)).astype(np.uint8)
    a = np.frombuffer(buf, dtype=np.uint8)
    masked = np.where((qual < CUTOFF) & (a != ord("\n")), ord("N"), a).astype(np.uint8).tobytes()   # QualitySequence::quality_mask
    dev, dq = upload(buf), upload(qual.tobytes(), fill=0xFF)
    for path, pre in PATH_PRES:
        for k in KS:
            with nt.KmerTable(k, path, len(buf), ctx) as t:
                t.count_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=CUTOFF)
                assert_items(t, oracle_items(masked, k, path, pre), ("quality", path, pre, k))


def _records(name):
    return [r.raw_seq for r in nt.parse_fastx_file(os.path.join(GOLDEN, name))]


def test_golden_28s_and_prjna271013(ctx):
    recs = _records("28S.fasta")
    with nt.KmerTable(4, nt.PATH_BITS_CANONICAL, 256, ctx) as t:
        t.count_records(recs, nt.PRE_STRIP_RETURNS)
        assert t.stats()["n_distinct"] == 136 and len(t.items()[0]) == 136
        assert t.lookup("AAAA") == 8108 and t.lookup(b"TTTT") == 8108
    with nt.KmerTable(4, nt.PATH_BYTES_CANONICAL, 256, ctx) as t:  # the README chain: normalize(false), k = 4
        t.count_records(recs, nt.PRE_NORMALIZE)
        assert t.lookup("AAAA") == 8108 and t.stats()["n_total"] == 736277
        assert int(t.items()[1].sum()) == 736277
    for path, pre in ((nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE), (nt.PATH_BITS_CANONICAL, nt.PRE_STRIP_RETURNS)):
        with nt.KmerTable(31, path, 800_000, ctx) as t:
            t.count_records(recs, pre)
            keys, counts = t.items()
            assert int(counts.sum()) == 718007, path
            if path == nt.PATH_BITS_CANONICAL:
                assert int((keys * counts).sum(dtype=np.uint64)) == 0xd59bc15e9cebae61
    # Σ key·count = the reduce face's ACC_SUM on the same bytes
    recs = _records("PRJNA271013_head.fq")
    with nt.KmerTable(21, nt.PATH_BYTES_CANONICAL, 300_000, ctx) as t:
        b = nt.Batch(ctx, sum(len(r) for r in recs) + len(recs), len(recs))
        for r in recs:
            assert b.append(r, nt.PRE_NORMALIZE)
        seq, _ = b.buffers()
        buf = seq.tobytes()
        b.release()
        dev = upload(buf)
        t.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        keys, counts = t.items()
        assert int(counts.sum()) == 209965
        r = check_against_reduce(ctx, t, dev, len(buf), 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE)
        assert int((keys * counts).sum(dtype=np.uint64)) == r["sum"]
        assert_items(t, oracle_items(buf, 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE), "PRJNA271013")


# ---- large inputs against the reduce face ----------------------------------------------------------------------------------------

def test_config2_batch_agrees_with_the_reduce_face(ctx):
    """BASELINE configs[1]: 10M x 150 bp, k = 21, ~1.3 G nearly all-distinct keys in a 2^31-slot table."""
    n_reads, L, k = 10_000_000, 150, 21
    nbytes = n_reads * (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
    with nt.KmerTable(k, nt.PATH_BYTES_CANONICAL, 1_400_000_000, ctx) as t:
        assert t.stats()["slots"] == 1 << 31
        t.count_device(dev, nbytes, nt.PRE_NORMALIZE)
        check_against_reduce(ctx, t, dev, nbytes, k, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE)


def test_chunk_boundaries_are_counted_once(ctx):
    """A batch of more than 64 MiB (the table's chunk) whose records straddle the chunk boundaries, at halos of 0, 16 and 32 bytes."""
    n_reads, L = 500_000, 150
    nbytes = n_reads * (L + 1)
    assert nbytes > (64 << 20) and (64 << 20) % (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0007, 0, n_reads, L, 2, dev)
    for path, pre, k in ((nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 21), (nt.PATH_BITS, nt.PRE_STRIP_RETURNS, 17),
                         (nt.PATH_BITS_CANONICAL, nt.PRE_NONE, 32), (nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE, 1)):
        with nt.KmerTable(k, path, nbytes, ctx) as t:
            t.count_device(dev, nbytes, pre)
            check_against_reduce(ctx, t, dev, nbytes, k, path, pre)


def _genome_reads(seed, genome_len, n_reads, L=150):
    """Reads sampled error-free from a seeded random genome, both strands, packed with one break byte each."""
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, genome_len)]
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    out = np.empty((n_reads, L + 1), dtype=np.uint8)
    out[:, L] = ord("\n")
    step = 200_000
    for lo in range(0, n_reads, step):
        hi = min(n_reads, lo + step)
        starts = rng.integers(0, genome_len - L + 1, hi - lo)
        reads = genome[starts[:, None] + np.arange(L)]
        flip = rng.random(hi - lo) < 0.5
        reads[flip] = comp[reads[flip][:, ::-1]]
        out[lo:hi, :L] = reads
    return out.reshape(-1)


def test_genome_sampled_reads_spectrum(ctx):
    """~300x error-free coverage of a 1 Mb genome: on a subsample, items() and spectrum() equal the oracle's; on the full set the
    spectrum sums and the reduce face agree."""
    k, path, pre = 21, nt.PATH_BITS_CANONICAL, nt.PRE_STRIP_RETURNS
    buf = _genome_reads(0x6E0E, 1_000_000, 2_000_000)
    sub = buf[: 20_000 * 151].tobytes()
    with nt.KmerTable(k, path, 2_100_000, ctx) as t:
        t.count_device(upload(sub), len(sub), pre)
        want = oracle_items(sub, k, path, pre)
        assert_items(t, want, "subsample")
        n_bins = int(want[1].max()) + 2
        h = t.spectrum(n_bins)
        assert np.array_equal(h, np.bincount(want[1], minlength=n_bins).astype(np.uint64))
        clamped = t.spectrum(3)
        assert list(clamped) == [0, int((want[1] == 1).sum()), int((want[1] >= 2).sum())]
        t.reset()
        dev = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        t.count_device(dev, buf.size, pre)
        check_against_reduce(ctx, t, dev, buf.size, k, path, pre)
        assert t.stats()["n_distinct"] <= 2_000_000


# ---- determinism and state ---------------------------------------------------------------------------------------------------

def test_determinism_and_reset(ctx):
    buf = pack(random_records(0xC0019, 400))
    dev = upload(buf)
    k, path, pre = 11, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE
    with nt.KmerTable(k, path, len(buf), ctx) as t:
        t.count_device(dev, len(buf), pre)
        one = t.items()
        # two calls (a record-aligned cut at a 16-byte boundary) equal one
        cut = next(i + 1 for i in range(len(buf) // 2, len(buf)) if buf[i:i + 1] == b"\n" and (i + 1) % 16 == 0)
        t.reset()
        assert t.stats()["n_total"] == 0 and len(t.items()[0]) == 0 and t.spectrum(4).sum() == 0
        t.count_device(dev, cut, pre)
        t.count_device(dev.data_ptr() + cut, len(buf) - cut, pre)
        two = t.items()
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
        # another launch geometry of the materialising scan, another run: identical arrays
        t.reset()
        ctx.set_launch(7, 0)
        try:
            t.count_device(dev, len(buf), pre)
        finally:
            ctx.set_launch(0, 0)
        three = t.items()
        assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1])
        with nt.KmerTable(k, path, len(buf), ctx) as u:
            u.count_device(dev, len(buf), pre)
            four = u.items()
        assert np.array_equal(one[0], four[0]) and np.array_equal(one[1], four[1])


# ---- error cases -------------------------------------------------------------------------------------------------------------

def test_error_cases(ctx):
    lib = counting.lib()
    buf = pack(random_records(0xC001A, 60))
    dev = upload(buf)
    # a tiny table drops occurrences and says so; the read side refuses it
    with nt.KmerTable(21, nt.PATH_BITS_CANONICAL, 3, ctx) as t:
        t.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        st = t.stats()
        assert st["slots"] == 4 and st["n_dropped"] > 0 and st["n_distinct"] == 4
        n = C.c_uint64(7)
        assert lib.ntk_kmer_table_extract_device(t._h, 1, None, None, 0, C.byref(n)) == 5
        h = np.zeros(8, dtype=np.uint64)
        assert lib.ntk_kmer_table_spectrum(t._h, h.ctypes.data, 8) == 5
        q = torch.zeros(4, dtype=torch.int64, device="cuda")
        assert lib.ntk_kmer_table_lookup_device(t._h, C.c_void_p(q.data_ptr()), 4, C.c_void_p(q.data_ptr())) == 5
        with pytest.raises(nt.NtkError) as e:
            t.items()
        assert e.value.status == 5
    with nt.KmerTable(5, nt.PATH_BITS, len(buf), ctx) as t:
        t.count_device(dev, len(buf), nt.PRE_NONE)
        want = oracle_items(buf, 5, nt.PATH_BITS, nt.PRE_NONE)
        # a small cap: NTK_ERR_CAPACITY and the number needed
        keys = torch.empty(4, dtype=torch.int64, device="cuda")
        n = C.c_uint64(0)
        assert lib.ntk_kmer_table_extract_device(t._h, 1, C.c_void_p(keys.data_ptr()), C.c_void_p(keys.data_ptr()), 4, C.byref(n)) == 5
        assert n.value == len(want[0])
        # min_count filters (0 reads as 1)
        for mc in (0, 1, 2, 5, 1000):
            ks, cs = t.items(mc)
            sel = want[1] >= max(mc, 1)
            assert np.array_equal(ks, want[0][sel]) and np.array_equal(cs, want[1][sel].astype(np.uint64)), mc
        # lookups: packed values as given, bytes, absent keys
        got = t.lookup(want[0][:50])
        assert np.array_equal(got, want[1][:50].astype(np.uint64))
        assert t.lookup(b"AAAAA") == int(dict(zip(want[0].tolist(), want[1].tolist())).get(0, 0))
        assert t.lookup(1 << 40) == 0
    # k = 32, all ones on the forward path: the side word, at its sorted place everywhere
    recs = [b"T" * 40, b"ACGT" * 10, b"T" * 32]
    b2 = pack(recs)
    with nt.KmerTable(32, nt.PATH_BITS, 64, ctx) as t:
        t.count_records(recs, nt.PRE_STRIP_RETURNS)
        want = oracle_items(b2, 32, nt.PATH_BITS, nt.PRE_STRIP_RETURNS)
        assert want[0][-1] == np.uint64(M64) and want[1][-1] == 10
        assert_items(t, want, "all ones")
        assert t.lookup(b"T" * 32) == 10 and t.lookup(M64) == 10
        h = t.spectrum(16)
        assert np.array_equal(h, np.bincount(want[1], minlength=16).astype(np.uint64))
        ks, cs = t.items(10)
        assert list(ks) == [M64] and list(cs) == [10]
    # the canonical table never sees all ones (TTT...T is AAA...A)
    with nt.KmerTable(32, nt.PATH_BITS_CANONICAL, 64, ctx) as t:
        t.count_records(recs, nt.PRE_STRIP_RETURNS)
        assert t.lookup(b"T" * 32) == 10 and t.lookup(b"A" * 32) == 10 and t.items()[0][0] == 0
    # argument checks
    with nt.KmerTable(21, nt.PATH_BYTES_CANONICAL, 1000, ctx) as t:
        for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):   # un-normalised byte-path input
            with pytest.raises(nt.NtkError) as e:
                t.count_device(dev, len(buf), pre)
            assert e.value.status == 6
        p = NL.Params(21, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE, 0)   # path mismatch
        assert lib.ntk_kmer_table_count_device(t._h, C.c_void_p(dev.data_ptr()), None, len(buf), C.byref(p)) == 2
        for k, flags in ((19, 0), (21, 11), (21, NL.FLAG_RESET)):   # k mismatch, window bits, reset flag
            p = NL.Params(k, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, flags)
            assert lib.ntk_kmer_table_count_device(t._h, C.c_void_p(dev.data_ptr()), None, len(buf), C.byref(p)) == 2
        p = NL.Params(21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 0)
        assert lib.ntk_kmer_table_count_device(t._h, C.c_void_p(dev.data_ptr() + 8), None, len(buf) - 8, C.byref(p)) == 2
        assert t.stats()["n_total"] == 0
    for k in (0, 33):
        with pytest.raises(nt.NtkError) as e:
            nt.KmerTable(k, nt.PATH_BITS, 100, ctx)
        assert e.value.status == 1


def test_count_kmers_example_prints_the_table(ctx):
    exe = os.path.join(ROOT, "examples", "count_kmers")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    fa = os.path.join(GOLDEN, "28S.fasta")
    recs = _records("28S.fasta")
    for k, path_arg, path, pre in ((4, "bytes", nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE), (21, "canonical", nt.PATH_BITS_CANONICAL,
                                                                                              nt.PRE_STRIP_RETURNS)):
        r = subprocess.run([exe, "-k", str(k), "-p", path_arg, "-m", "2", fa], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        with nt.KmerTable(k, path, 800_000, ctx) as t:
            t.count_records(recs, pre)
            keys, counts = t.items(2)
            want = [f"{nt.bitmer_to_bytes(int(kk), k).decode()}\t{int(c)}" for kk, c in zip(keys, counts)]
            assert r.stdout.splitlines() == want
            r = subprocess.run([exe, "-k", str(k), "-p", path_arg, "-s", "64", fa], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            h = t.spectrum(64)
            assert r.stdout.splitlines() == [f"{c}\t{int(h[c])}" for c in range(1, 64)]
    r = subprocess.run([exe, "-k", "4", fa], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AAAA\t8108" in r.stdout.splitlines()
