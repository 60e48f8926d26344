"""The wide count table (include/needletail_amd_wide_count.h, needletail_amd.WideKmerTable, k = 33..63) on a real MI355X.

"The oracle's items" below: the oracle's literal iterator canonical_kmers_arrays (positions and flags) -> the {hi, lo} words of each
chosen strand -> numpy.unique(axis=0, return_counts=True).  On inputs too large for that, the table is held against the reduce face
on the same bytes (n_total and ACC_HIST, the leading six bases), which the suite already checks against the oracle.  Keys aimed at one
home slot come from the host model tests/_wide_count_model.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import wide_counting  # noqa: E402
import _wide_count_model as W  # noqa: E402
from _count_helpers import CUTOFF, pack, quality_masked, random_records, upload  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (33, 34, 40, 51, 62, 63)
PRES = (nt.PRE_NORMALIZE, nt.PRE_NORMALIZE_IUPAC)
BYTES = nt.PATH_BYTES_CANONICAL
ERR_BAD_K, ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 1, 2, 5, 6

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c + 32] = _i


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def _window_words(codes, starts, k):
    hi = np.zeros(len(starts), dtype=np.uint64)
    lo = np.zeros(len(starts), dtype=np.uint64)
    for i in range(k - 32):
        hi = (hi << np.uint64(2)) | codes[starts + i].astype(np.uint64)
    for i in range(k - 32, k):
        lo = (lo << np.uint64(2)) | codes[starts + i].astype(np.uint64)
    return hi, lo


def oracle_items(buf: bytes, k: int):
    """(keys [n, 2] of [hi, lo] rows ascending, counts) of every canonical k-mer the batch emits on the byte path after normalize.
    Each maximal run of base bytes (ACGTacgtUu) is a sequence of its own; the runs are laid side by side with an N where the other
    bytes were, so one iterator call covers them all."""
    a = np.frombuffer(buf, dtype=np.uint8)
    isu = (a == ord("U")) | (a == ord("u"))
    base = (_CODE[a] != 255) | isu
    runs = np.where(base, a, ord("N")).astype(np.uint8)
    runs[isu] = ord("T")
    norm = O.normalize(runs.tobytes())[0]
    n = len(norm)
    rc = O.reverse_complement(norm)
    pos, flg = O.canonical_kmers_arrays(norm, rc, k)
    pos = pos.astype(np.int64)
    if pos.size == 0:
        return np.zeros((0, 2), np.uint64), np.zeros(0, np.int64)
    fw, rv = _CODE[np.frombuffer(norm, dtype=np.uint8)], _CODE[np.frombuffer(rc, dtype=np.uint8)]
    fh, fl = _window_words(fw, np.where(flg == 1, 0, pos), k)
    rh, rl = _window_words(rv, np.where(flg == 1, n - pos - k, 0), k)
    rows = np.stack([np.where(flg == 1, rh, fh), np.where(flg == 1, rl, fl)], axis=1)
    return np.unique(rows, axis=0, return_counts=True)


def assert_items(table, want, what):
    keys, counts = table.items()
    assert keys.shape == want[0].shape and np.array_equal(keys, want[0]), what
    assert np.array_equal(counts, want[1].astype(np.uint64)), what
    st = table.stats()
    assert st["n_distinct"] == len(want[0]) and st["n_total"] == int(want[1].sum()) and st["n_dropped"] == 0, (what, st)


def device_items(table, min_count=1):
    """(keys [n, 2], counts) as device tensors (for tables too large for the host)."""
    lib = wide_counting.lib()
    n = C.c_uint64(0)
    rc = lib.ntk_wide_table_extract_device(table._h, min_count, None, None, 0, C.byref(n))
    assert rc in (0, ERR_CAPACITY), rc
    keys = torch.empty(max(2 * n.value, 2), dtype=torch.int64, device="cuda")
    counts = torch.empty(max(n.value, 1), dtype=torch.int64, device="cuda")
    NL.check(lib.ntk_wide_table_extract_device(table._h, min_count, C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()),
                                               n.value, C.byref(n)), "extract")
    return keys[: 2 * n.value].view(-1, 2), counts[: n.value]


def _strictly_ascending(keys):
    """keys: a device [n, 2] int64 tensor of [hi, lo] rows."""
    if keys.shape[0] < 2:
        return True
    hi, lo = keys[:, 0], keys[:, 1] ^ (-(1 << 63))   # unsigned order of lo as signed
    return bool(((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1]))).all())


def check_against_reduce(ctx, table, dev, n_bytes, k, pre, split_at=()):
    """Σ counts = n_total, counts folded by the leading six bases = ACC_HIST, keys strictly ascending, the spectrum sums to
    n_distinct.  split_at: record-aligned, 16-byte-aligned cut points of the reduce face's calls."""
    ctx.accum_reset()
    cuts = [0, *split_at, n_bytes]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ctx.reduce_device(dev.data_ptr() + a, b - a, k, BYTES, pre)
    r = ctx.accum_read()
    st = table.stats()
    assert st["n_dropped"] == 0 and st["n_total"] == r["n_total"], (st, r["n_total"])
    keys, counts = device_items(table)
    assert keys.shape[0] == st["n_distinct"]
    assert int(counts.sum()) == r["n_total"]
    assert _strictly_ascending(keys), "keys not strictly ascending"
    hist = torch.zeros(4096, dtype=torch.int64, device="cuda")
    hist.scatter_add_(0, (keys[:, 0] >> (2 * k - 64 - 12)) & 4095, counts)   # the leading six bases are in hi (k >= 38)
    assert np.array_equal(hist.cpu().numpy().astype(np.uint64), r["hist"])
    h = table.spectrum(16384)
    assert h[0] == 0 and int(h.sum()) == st["n_distinct"]
    del keys, counts, hist
    return r


def both_strands(keys, k):
    rh, rl = W.revcomp(keys[:, 0], keys[:, 1], k)
    return np.stack([rh, rl], axis=1)


# ---- 1. exact against the oracle -------------------------------------------------------------------------------------------------

def test_random_records_match_the_oracle(ctx):
    recs = random_records(0xD0017, 200)
    buf = pack(recs)
    dev = upload(buf)
    rng = np.random.default_rng(3)
    for k in KS:
        want = oracle_items(buf, k)
        assert len(want[0]) > 1000
        for pre in PRES:
            with nt.WideKmerTable(k, BYTES, len(buf), ctx) as t:
                t.count_device(dev, len(buf), pre)
                assert_items(t, want, (pre, k))
                if pre == nt.PRE_NORMALIZE:
                    # lookups: every key on both strands, absent keys, bits above 2k
                    assert np.array_equal(t.lookup(want[0]), want[1].astype(np.uint64)), k
                    assert np.array_equal(t.lookup(both_strands(want[0], k)), want[1].astype(np.uint64)), k
                    absent = np.stack([rng.integers(0, 1 << (2 * k - 64), 500, dtype=np.uint64),
                                       rng.integers(0, 1 << 63, 500, dtype=np.uint64)], axis=1)
                    known = {(int(a), int(b)) for a, b in want[0]} | {(int(a), int(b)) for a, b in both_strands(want[0], k)}
                    absent = np.array([r for r in absent if (int(r[0]), int(r[1])) not in known], dtype=np.uint64)
                    assert not t.lookup(absent).any()
                    over = want[0][:20].copy()
                    over[:, 0] |= np.uint64(1 << (2 * k - 64))
                    assert not t.lookup(over).any()
                    s = wide_counting.decode(want[0][:3], k)
                    for kmer, c in zip(s, want[1][:3]):
                        assert t.lookup(kmer) == c and t.lookup(O.reverse_complement(kmer).decode()) == c
                        assert t.lookup(kmer.lower()) == c
                else:
                    # the packer route: the same records through ntk_batch_append
                    t.reset()
                    t.count_records(recs, pre)
                    assert_items(t, want, ("records", pre, k))


def test_quality_stream_matches_the_oracle(ctx):
    buf = pack(random_records(0xD0018, 200))
    rng = np.random.default_rng(6)
    qual = rng.integers(33, 80, len(buf)).astype(np.uint8)
    masked = quality_masked(buf, qual)
    dev, dq = upload(buf), upload(qual.tobytes(), fill=0xFF)
    for k in (40, 63):
        with nt.WideKmerTable(k, BYTES, len(buf), ctx) as t:
            t.count_device(dev, len(buf), nt.PRE_NORMALIZE, d_qual=dq, quality_cutoff=CUTOFF)
            assert_items(t, oracle_items(masked, k), ("quality", k))
            t.reset()   # cutoff 0 or no stream: no mask
            t.count_device(dev, len(buf), nt.PRE_NORMALIZE, d_qual=dq, quality_cutoff=0)
            t.count_device(dev, len(buf), nt.PRE_NORMALIZE_IUPAC)
            want = oracle_items(buf, k)
            assert_items(t, (want[0], want[1] * 2), ("no mask", k))


def _records(name):
    return [r.raw_seq for r in nt.parse_fastx_file(os.path.join(GOLDEN, name))]


def _packed(ctx, recs):
    b = nt.Batch(ctx, sum(len(r) for r in recs) + len(recs), len(recs))
    for r in recs:
        assert b.append(r, nt.PRE_NORMALIZE)
    seq, _ = b.buffers()
    buf = seq.tobytes()
    b.release()
    return buf


def test_golden_files_and_the_cli(ctx):
    exe = os.path.join(ROOT, "examples", "count_kmers")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    for name in ("28S.fasta", "PRJNA271013_head.fq"):
        recs = _records(name)
        buf = _packed(ctx, recs)
        for k in (51, 63):
            want = oracle_items(buf, k)
            with nt.WideKmerTable(k, BYTES, len(buf), ctx) as t:
                t.count_records(recs, nt.PRE_NORMALIZE)
                assert_items(t, want, (name, k))
                keys, counts = t.items(2)
                sel = want[1] >= 2
                assert np.array_equal(keys, want[0][sel]) and np.array_equal(counts, want[1][sel].astype(np.uint64))
                path = os.path.join(GOLDEN, name)
                r = subprocess.run([exe, "-k", str(k), "-m", "2", path], capture_output=True, text=True, timeout=120)
                assert r.returncode == 0, r.stderr
                lines = [f"{s.decode()}\t{int(c)}" for s, c in zip(wide_counting.decode(keys, k), counts)]
                assert r.stdout.splitlines() == lines, (name, k)
                r = subprocess.run([exe, "-k", str(k), "-s", "64", path], capture_output=True, text=True, timeout=120)
                assert r.returncode == 0, r.stderr
                h = t.spectrum(64)
                assert r.stdout.splitlines() == [f"{c}\t{int(h[c])}" for c in range(1, 64)]
    fa = os.path.join(GOLDEN, "28S.fasta")
    for args in (["-k", "33", "-p", "bits"], ["-k", "40", "-p", "canonical"], ["-k", "64"]):
        r = subprocess.run([exe, *args, fa], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "count_kmers" in r.stderr, args


# ---- 4. a large batch against the reduce face ------------------------------------------------------------------------------------

def test_synthetic_reads_agree_with_the_reduce_face(ctx):
    """1 M x 150 bp synthetic reads (with N), ~100 M nearly all-distinct keys at k = 51 in a 2^28-slot table."""
    n_reads, L = 1_000_000, 150
    nbytes = n_reads * (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
    for k in (51, 63):
        with nt.WideKmerTable(k, BYTES, n_reads * (L - k + 1), ctx) as t:
            assert t.stats()["slots"] <= 1 << 28
            t.count_device(dev, nbytes, nt.PRE_NORMALIZE)
            check_against_reduce(ctx, t, dev, nbytes, k, nt.PRE_NORMALIZE)
    del dev
    torch.cuda.empty_cache()


# ---- 5. two-word races -------------------------------------------------------------------------------------------------------------

def _race(ctx, k, hi, lo, reps, seed):
    slots = 1 << 13
    buf = W.records_for(hi, lo, reps, k, seed=seed)
    with nt.WideKmerTable(k, BYTES, 3 << 11, ctx) as t:
        assert t.stats()["slots"] == slots
        t.count_device(upload(buf), len(buf), nt.PRE_NORMALIZE)
        order = np.lexsort((lo, hi))
        want = (np.stack([hi, lo], axis=1)[order], np.full(hi.size, reps, dtype=np.int64))
        assert_items(t, want, ("race", k))
        keys, _ = t.items()
        assert np.unique(keys, axis=0).shape[0] == keys.shape[0], "a key twice in extract"
        assert np.array_equal(oracle_items(buf, k)[0], want[0])


def test_keys_sharing_one_hi_word_and_home_slot_race_exactly(ctx):
    for k, h in ((63, 100), (51, 8000), (33, 0)):
        hi, lo = W.keys_sharing_hi(h, 1 << 13, k, 1 & ((1 << (2 * k - 64)) - 1), 400)
        assert (W.home(hi, lo, 1 << 13) == h).all()
        _race(ctx, k, hi, lo, 40, seed=k)


def test_keys_sharing_one_lo_word_and_home_slot_race_exactly(ctx):
    k = 63
    for h, word in ((5, 0x0123456789ABCDEF), (8191, 0)):
        hi, lo = W.keys_sharing_lo(h, 1 << 13, k, word, 400)
        assert (W.home(hi, lo, 1 << 13) == h).all()
        _race(ctx, k, hi, lo, 40, seed=h)


# ---- 6. the probe bound ------------------------------------------------------------------------------------------------------------

def test_probe_bound_wraps_and_drops(ctx):
    k, slots = 63, 1 << 14
    h = slots - 100
    hi, lo = W.keys_sharing_hi(h, slots, k, 7, W.PROBE_MAX + 1)
    counts = 1 + np.arange(W.PROBE_MAX) % 3
    buf = W.records_for(hi[:-1], lo[:-1], counts, k, seed=9)
    lib = wide_counting.lib()
    with nt.WideKmerTable(k, BYTES, 3 << 12, ctx) as t:
        assert t.stats()["slots"] == slots
        t.count_device(upload(buf), len(buf), nt.PRE_NORMALIZE)
        order = np.lexsort((lo[:-1], hi[:-1]))
        assert_items(t, (np.stack([hi[:-1], lo[:-1]], axis=1)[order], counts[order]), "4096 keys of one home slot")
        # the 4097th key, in a later call: dropped by exactly its count, and the read side refuses the table
        extra = W.records_for(hi[-1:], lo[-1:], [5], k, seed=10)
        t.count_device(upload(extra), len(extra), nt.PRE_NORMALIZE)
        st = t.stats()
        assert (st["n_distinct"], st["n_total"], st["n_dropped"]) == (W.PROBE_MAX, int(counts.sum()), 5), st
        n = C.c_uint64(7)
        assert lib.ntk_wide_table_extract_device(t._h, 1, None, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == 0
        h16 = np.zeros(16, dtype=np.uint64)
        assert lib.ntk_wide_table_spectrum(t._h, h16.ctypes.data, 16) == ERR_CAPACITY
        q = torch.zeros(4, dtype=torch.int64, device="cuda")
        assert lib.ntk_wide_table_lookup_device(t._h, C.c_void_p(q.data_ptr()), 2, C.c_void_p(q.data_ptr())) == ERR_CAPACITY
        with pytest.raises(nt.NtkError) as e:
            t.items()
        assert e.value.status == ERR_CAPACITY
    # a tiny table fills every slot (bound = slots = 4)
    buf = pack(random_records(0xD001A, 30))
    with nt.WideKmerTable(40, BYTES, 3, ctx) as t:
        t.count_device(upload(buf), len(buf), nt.PRE_NORMALIZE)
        st = t.stats()
        assert st["slots"] == 4 and st["n_distinct"] == 4 and st["n_dropped"] > 0
        assert st["n_total"] + st["n_dropped"] == int(oracle_items(buf, 40)[1].sum())


# ---- 7. kernel seams -----------------------------------------------------------------------------------------------------------------

def test_kernel_seams_item_by_item(ctx):
    """A break (record end, N, masked quality) at every offset 0..k before and after every lane-run seam (64 bytes) of a batch that
    spans several 256-lane tiles; then readable padding of A past an n_bytes that is not a multiple of 16."""
    rng = np.random.default_rng(0x5EA)
    span = 2 * W.THREADS * W.LANE_RUN + 3 * W.LANE_RUN + 5
    for k in (33, 63):
        with nt.WideKmerTable(k, BYTES, span, ctx) as t:
            for d in range(-k, k + 1):
                a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, span)].copy()
                at = np.arange(W.LANE_RUN, span, W.LANE_RUN) + d
                at = at[(at >= 0) & (at < span)]
                qual = np.full(span, 60, dtype=np.uint8)
                kind = (d + k) % 3
                if kind == 0:
                    a[at] = ord("\n")
                elif kind == 1:
                    a[at] = ord("N")
                else:
                    qual[at] = 10
                buf = a.tobytes()
                t.reset()
                t.count_device(upload(buf), len(buf), nt.PRE_NORMALIZE, d_qual=upload(qual.tobytes()), quality_cutoff=CUTOFF)
                assert_items(t, oracle_items(quality_masked(buf, qual), k), ("seam", k, d))
            # padding past n_bytes: A up to the readable end, n_bytes % 16 != 0
            for n_bytes in (span - 16 * 3 - 1, 100, k, k - 1, 1):
                buf = bytes(a[:n_bytes])
                dev = upload(buf, fill=ord("A"))
                t.reset()
                t.count_device(dev, n_bytes, nt.PRE_NORMALIZE)
                want = oracle_items(buf, k)
                if n_bytes < k:
                    assert t.stats()["n_total"] == 0 and len(t.items()[0]) == 0
                else:
                    assert_items(t, want, ("padding", k, n_bytes))


# ---- 8. more than 2^32 bytes in one call ------------------------------------------------------------------------------------------

def _genome_reads(dev, seed, genome_len, n_reads, L):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genome = acgt[torch.randint(0, 4, (genome_len,), generator=g, device="cuda")]
    view = dev[: n_reads * (L + 1)].view(n_reads, L + 1)
    view[:, L] = ord("\n")
    off = torch.arange(L, device="cuda")
    for lo in range(0, n_reads, 1_000_000):
        hi = min(n_reads, lo + 1_000_000)
        starts = torch.randint(0, genome_len - L + 1, (hi - lo,), generator=g, device="cuda")
        view[lo:hi, :L] = genome[starts[:, None] + off]


def test_more_than_2_32_bytes_in_one_call(ctx):
    """Reads sampled from a 1 Mb genome, 4.3 GB in one count call; the reduce face in record-aligned calls of < 2^32 bytes."""
    L, k = 150, 51
    n_reads = (1 << 32) // (L + 1) + 50_000
    nbytes = n_reads * (L + 1)
    assert nbytes > 1 << 32
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    _genome_reads(dev, 0x6E0F, 1_000_000, n_reads, L)
    torch.cuda.synchronize()
    cut = (n_reads // 2) // 16 * 16 * (L + 1)   # a record boundary and a multiple of 16
    with nt.WideKmerTable(k, BYTES, 2_000_000, ctx) as t:
        t.count_device(dev, nbytes, nt.PRE_NORMALIZE)
        r = check_against_reduce(ctx, t, dev, nbytes, k, nt.PRE_NORMALIZE, split_at=(cut,))
        assert r["n_total"] == n_reads * (L - k + 1)
        assert t.stats()["n_distinct"] <= 2_000_000
    del dev
    torch.cuda.empty_cache()


# ---- 9. determinism and state --------------------------------------------------------------------------------------------------------

def test_determinism_and_state(ctx):
    recs = random_records(0xD0019, 300)
    buf = pack(recs)
    k = 45
    want = oracle_items(buf, k)
    lib = wide_counting.lib()
    with nt.WideKmerTable(k, BYTES, len(buf), ctx) as t:
        t.count_device(upload(buf), len(buf), nt.PRE_NORMALIZE)
        one = t.items()
        rev = pack(recs[::-1])
        t.reset()
        st = t.stats()
        assert (st["n_distinct"], st["n_total"], st["n_dropped"]) == (0, 0, 0)
        assert t.items()[0].shape == (0, 2) and not t.spectrum(4).any() and not t.lookup(want[0][:10]).any()
        t.count_device(upload(rev), len(rev), nt.PRE_NORMALIZE)
        two = t.items()
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
        assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[1].astype(np.uint64))
        # counts accumulate across calls; a record-aligned cut at a 16-byte boundary
        cut = next(i + 1 for i in range(len(buf) // 2, len(buf)) if buf[i:i + 1] == b"\n" and (i + 1) % 16 == 0)
        dev = upload(buf)
        t.count_device(dev, cut, nt.PRE_NORMALIZE)
        t.count_device(dev.data_ptr() + cut, len(buf) - cut, nt.PRE_NORMALIZE)
        assert_items(t, (want[0], want[1] * 2), "accumulated")
        # extract: cap too small -> NTK_ERR_CAPACITY and the number needed; min_count (0 reads as 1)
        need = len(want[0])
        dk = torch.zeros(2 * need, dtype=torch.int64, device="cuda")
        dc = torch.zeros(need, dtype=torch.int64, device="cuda")
        n = C.c_uint64(0)
        args = (C.c_void_p(dk.data_ptr()), C.c_void_p(dc.data_ptr()))
        assert lib.ntk_wide_table_extract_device(t._h, 1, *args, need - 1, C.byref(n)) == ERR_CAPACITY and n.value == need
        assert not dk.any()
        assert lib.ntk_wide_table_extract_device(t._h, 1, *args, need, C.byref(n)) == 0 and n.value == need
        assert np.array_equal(dk.cpu().numpy().view(np.uint64).reshape(-1, 2), want[0])
        for mc in (0, 1, 2, 3, 4, 6, 1000):
            ks, cs = t.items(mc)
            sel = want[1] * 2 >= max(mc, 1)
            assert np.array_equal(ks, want[0][sel]) and np.array_equal(cs, (want[1][sel] * 2).astype(np.uint64)), mc
        # the spectrum and its clamp
        n_bins = int(want[1].max()) * 2 + 2
        assert np.array_equal(t.spectrum(n_bins), np.bincount(want[1] * 2, minlength=n_bins).astype(np.uint64))
        assert list(t.spectrum(2)) == [0, need]
        assert list(t.spectrum(3)) == [0, 0, need]
        with pytest.raises(nt.NtkError):
            t.spectrum(1)
        with pytest.raises(nt.NtkError):
            t.spectrum(16385)
        # a second table on the same bytes: identical arrays
        with nt.WideKmerTable(k, BYTES, len(buf), ctx) as u:
            u.count_device(dev, len(buf), nt.PRE_NORMALIZE_IUPAC)
            three = u.items()
        assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1])


# ---- 10. error cases -----------------------------------------------------------------------------------------------------------------

def test_error_cases(ctx):
    lib = wide_counting.lib()
    for k, path, cap, status in ((32, BYTES, 100, ERR_BAD_K), (64, BYTES, 100, ERR_BAD_K), (0, BYTES, 100, ERR_BAD_K),
                                 (255, BYTES, 100, ERR_BAD_K), (40, nt.PATH_BITS, 100, ERR_BAD_K),
                                 (40, nt.PATH_BITS_CANONICAL, 100, ERR_BAD_K), (40, 3, 100, ERR_BAD_ARG), (40, BYTES, 0, ERR_BAD_ARG),
                                 (40, BYTES, (3 << 38) + 1, ERR_BAD_ARG)):
        with pytest.raises(nt.NtkError) as e:
            nt.WideKmerTable(k, path, cap, ctx)
        assert e.value.status == status, (k, path, cap)
    buf = pack(random_records(0xD001B, 40))
    dev, dq = upload(buf), upload(bytes(len(buf)))
    with nt.WideKmerTable(40, BYTES, 1000, ctx) as t:
        def call(p, seq=dev.data_ptr(), qual=None, n=len(buf)):
            return lib.ntk_wide_table_count_device(t._h, C.c_void_p(seq), None if qual is None else C.c_void_p(qual), n, C.byref(p))
        for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):   # un-normalised byte input
            with pytest.raises(nt.NtkError) as e:
                t.count_device(dev, len(buf), pre)
            assert e.value.status == ERR_UNSUPPORTED
        assert call(NL.Params(40, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE, 0)) == ERR_BAD_ARG   # path mismatch
        for k, flags in ((41, 0), (40, 11), (40, NL.FLAG_RESET), (40, 1 << 20)):   # k mismatch, window bits, reset flag, high bits
            assert call(NL.Params(k, BYTES, nt.PRE_NORMALIZE, flags)) == ERR_BAD_ARG, (k, flags)
        assert call(NL.Params(40, BYTES, 4, 0)) == ERR_BAD_ARG   # no such pre
        p = NL.Params(40, BYTES, nt.PRE_NORMALIZE, NL.flags(0, CUTOFF))
        assert call(p, seq=dev.data_ptr() + 8, n=len(buf) - 8) == ERR_BAD_ARG     # misaligned d_seq
        assert call(p, qual=dq.data_ptr() + 4) == ERR_BAD_ARG                      # misaligned d_qual
        assert lib.ntk_wide_table_count_device(t._h, None, None, len(buf), C.byref(p)) == ERR_BAD_ARG
        assert call(p, n=0) == 0
        assert t.stats()["n_total"] == 0
        with pytest.raises(ValueError):
            t.lookup("ACGT")
        assert t.lookup("A" * 40) == 0
