"""The device count table (include/needletail_amd_count.h) at its edges on a real MI355X: the sizing promise at 75 % load, the probe
bound and the wrap past the last slot, chunk seams, the spectrum clamp and extract bounds, counts past 2^32, and a second device.

Every reference is either the oracle's literal iterators (tests/_count_helpers.py) or a multiset of keys the test built itself.  The
host model of the table (tests/_count_model.py) only aims: it picks keys with a chosen home slot and records that cross a chunk seam
at a chosen byte; no expected value goes through the table's hashing, probing, extract or sort."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import counting  # noqa: E402
import _count_model as M  # noqa: E402
from _count_helpers import (CUTOFF, M64, PATH_PRES, assert_items, device_items, oracle_items, pack, quality_masked,  # noqa: E402
                            random_records, upload)

pytestmark = pytest.mark.gpu

ERR_BAD_ARG, ERR_CAPACITY = 2, 5
SIGN = -(1 << 63)          # x ^ SIGN orders int64 bit patterns as unsigned
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def count(t, buf: bytes, pre=nt.PRE_NONE):
    dev = upload(buf)
    t.count_device(dev, len(buf), pre)
    t.ctx.synchronize()


def lookup_device(t, q):
    out = torch.empty_like(q)
    torch.cuda.synchronize()
    NL.check(counting.lib().ntk_kmer_table_lookup_device(t._h, C.c_void_p(q.data_ptr()), q.numel(), C.c_void_p(out.data_ptr())),
             "lookup")
    return out


def read_side_status(t):
    """(status, *n) of an extract size query (cap 0), the status of spectrum and of lookup."""
    lib = counting.lib()
    n = C.c_uint64(0)
    h = np.zeros(4, dtype=np.uint64)
    q = torch.zeros(1, dtype=torch.int64, device=f"cuda:{t.ctx.device}")
    out = torch.zeros_like(q)
    torch.cuda.synchronize()
    rc = lib.ntk_kmer_table_extract_device(t._h, 1, None, None, 0, C.byref(n))
    return (rc, n.value, lib.ntk_kmer_table_spectrum(t._h, h.ctypes.data, 4),
            lib.ntk_kmer_table_lookup_device(t._h, C.c_void_p(q.data_ptr()), 1, C.c_void_p(out.data_ptr())))


INCOMPLETE = (ERR_CAPACITY, 0, ERR_CAPACITY, ERR_CAPACITY)   # n_dropped > 0: the read side refuses, extract's *n = 0


def assert_exact(t, keys, counts, what):
    """items(), stats() and lookup() of every key equal the multiset the test inserted."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.broadcast_to(np.asarray(counts, dtype=np.uint64), keys.shape)
    order = np.argsort(keys, kind="stable")
    assert_items(t, (keys[order], counts[order]), what)
    assert np.array_equal(t.lookup(keys), counts), what


def is_canonical(path):
    return path != nt.PATH_BITS


# ---- (a) sizing and the capacity promise -------------------------------------------------------------------------------------

def test_sizing_follows_the_capacity_rule(ctx):
    caps = [1, 2, 3, 4, 6, 7, 12, 13] + [(3 << j) + d for j in (2, 5, 11, 20) for d in (0, 1)]
    for cap in caps:
        with nt.KmerTable(21, nt.PATH_BITS_CANONICAL, cap, ctx) as t:
            assert t.stats()["slots"] == M.slots_for(cap), cap
    for cap in (0, (3 << 38) + 1, M64):
        with pytest.raises(nt.NtkError) as e:
            nt.KmerTable(21, nt.PATH_BITS_CANONICAL, cap, ctx)
        assert e.value.status == ERR_BAD_ARG, cap


def test_capacity_keys_fit_at_75_percent_load(ctx):
    """3 * 2^26 random 64-bit keys in a table made for that many: 2^28 slots at 0.75 load, nothing dropped, every key exact."""
    cap = 3 << 26
    g = torch.Generator(device="cuda")
    g.manual_seed(0x75)
    keys = torch.randint(0, 256, (cap * 8,), generator=g, dtype=torch.uint8, device="cuda").view(torch.int64)
    recs = torch.full((cap * 33 + 64,), ord("\n"), dtype=torch.uint8, device="cuda")
    view = recs[: cap * 33].view(cap, 33)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    step = 1 << 24
    for lo in range(0, cap, step):
        part = keys[lo:lo + step]
        for i in range(32):
            view[lo:lo + step, i] = acgt[(part >> (62 - 2 * i)) & 3]
    torch.cuda.synchronize()
    with nt.KmerTable(32, nt.PATH_BITS, cap, ctx) as t:
        assert t.stats()["slots"] == 1 << 28
        t.count_device(recs, cap * 33, nt.PRE_NONE)
        st = t.stats()
        del view, recs
        uk, uc = torch.unique(keys ^ SIGN, sorted=True, return_counts=True)
        assert st["n_dropped"] == 0 and st["n_total"] == cap and st["n_distinct"] == uk.numel(), st
        gk, gc = device_items(t)
        assert torch.equal(gk, uk ^ SIGN) and torch.equal(gc, uc)
        del gk, gc
        absent = torch.randint(0, 256, (cap * 8,), generator=g, dtype=torch.uint8, device="cuda").view(torch.int64)
        for q in (keys, absent):
            got = lookup_device(t, q)
            u = q ^ SIGN
            idx = torch.searchsorted(uk, u).clamp_(max=uk.numel() - 1)
            want = torch.where(uk[idx] == u, uc[idx], torch.zeros_like(u))
            assert torch.equal(got, want)
            del got, u, idx, want
        del absent
    del keys, uk, uc
    torch.cuda.empty_cache()


# ---- (b) probe bound, drops and wrap-around ----------------------------------------------------------------------------------

PROBE_CASES = [(nt.PATH_BITS, 32), (nt.PATH_BITS, 16), (nt.PATH_BITS_CANONICAL, 32), (nt.PATH_BITS_CANONICAL, 16)]


@pytest.mark.parametrize("path,k", PROBE_CASES)
def test_probe_bound_wraps_and_drops(ctx, path, k):
    """4096 keys with home slots - 7 of 8192: the chain wraps through slot 0 and fills the probe bound.  The last key, inserted on
    its own, sits at chain position 4095; a 4097th is dropped, exactly its count, and the read side refuses the table."""
    slots, c = 8192, 3
    h = slots - 7
    keys = M.keys_with_home(h, slots, k, M.PROBE_MAX + 2, is_canonical(path))
    chain, extra, absent = keys[:M.PROBE_MAX], keys[M.PROBE_MAX:M.PROBE_MAX + 1], keys[M.PROBE_MAX + 1:]
    with nt.KmerTable(k, path, 6144, ctx) as t:
        assert t.stats()["slots"] == slots and M.probe_bound(slots) == M.PROBE_MAX
        count(t, M.records_for(chain[:-1], c, k))
        count(t, M.records_for(chain[-1:], c, k))   # chain position 4095: slot (h + 4095) & (slots - 1)
        assert_exact(t, chain, c, ("chain", path, k))
        assert t.lookup(absent)[0] == 0             # walks 4096 full slots, never an EMPTY one
        assert read_side_status(t) == (ERR_CAPACITY, M.PROBE_MAX, 0, 0)
        count(t, M.records_for(extra, c, k))
        st = t.stats()
        assert st["n_distinct"] == M.PROBE_MAX and st["n_dropped"] == c, st
        assert st["n_total"] == M.PROBE_MAX * c and st["n_total"] + st["n_dropped"] == (M.PROBE_MAX + 1) * c, st
        assert read_side_status(t) == INCOMPLETE
        t.reset()
        count(t, M.records_for(chain, c, k))        # the whole chain in one launch
        assert_exact(t, chain, c, ("after reset", path, k))
        assert t.lookup(absent)[0] == 0


@pytest.mark.parametrize("path,k", [(nt.PATH_BITS, 32), (nt.PATH_BITS_CANONICAL, 16)])
def test_keys_homed_inside_a_cluster(ctx, path, k):
    """A cluster of 3000 keys at home h, then keys whose homes lie inside it and just past it: all exact.  Absent keys whose homes
    lie in the cluster read 0."""
    slots, h, canon = 8192, 1000, is_canonical(path)
    cluster = M.keys_with_home(h, slots, k, 3000, canon)
    late = [M.keys_with_home(h, slots, k, 3003, canon)[3000:]]
    absent = []
    for d in (1, 1499, 2999, 3000, 3001, 3100):
        ks = M.keys_with_home(h + d, slots, k, 4, canon)
        late.append(ks[:3])
        absent.append(ks[3])
    absent.append(M.keys_with_home(h + 1500, slots, k, 1, canon)[0])
    late = np.concatenate(late)
    with nt.KmerTable(k, path, 6144, ctx) as t:
        count(t, M.records_for(cluster, 2, k))
        late_counts = np.arange(1, late.size + 1)
        count(t, M.records_for(late, late_counts, k))
        assert_exact(t, np.concatenate([cluster, late]), np.concatenate([np.full(cluster.size, 2), late_counts]), ("cluster", path, k))
        assert not t.lookup(np.array(absent, dtype=np.uint64)).any()


@pytest.mark.parametrize("path,k", [(nt.PATH_BITS, 32), (nt.PATH_BITS_CANONICAL, 13)])
def test_small_table_fills_every_slot(ctx, path, k):
    """Capacity 6: 8 slots, probe bound 8.  8 keys fill it (all with one home: the chain wraps; or any 8), exact; an absent key walks
    the whole table and reads 0; a 9th key is dropped, exactly its count."""
    canon = is_canonical(path)
    with nt.KmerTable(k, path, 6, ctx) as t:
        assert t.stats()["slots"] == 8
        for keys in (M.keys_with_home(5, 8, k, 9, canon), M.keys_with_home(0, 1, k, 9, canon)):
            t.reset()
            counts = np.arange(1, 9)
            count(t, M.records_for(keys[:8], counts, k))
            assert_exact(t, keys[:8], counts, ("full", path, k))
            assert t.lookup(keys[8:])[0] == 0
            count(t, M.records_for(keys[8:], 7, k))
            st = t.stats()
            assert (st["n_distinct"], st["n_total"], st["n_dropped"]) == (8, 36, 7), st
            assert read_side_status(t) == INCOMPLETE


@pytest.mark.parametrize("path,k", [(nt.PATH_BITS, 32), (nt.PATH_BITS_CANONICAL, 21)])
def test_colliding_keys_race_for_slots(ctx, path, k):
    """Thousands of occurrences of twelve keys with two neighbouring homes (the chain wraps) in one launch: lanes race for the same
    EMPTY slots ("already this key" against "claimed by another") and add to the same counts."""
    slots, canon = 8192, is_canonical(path)
    keys = np.concatenate([M.keys_with_home(slots - 2, slots, k, 6, canon), M.keys_with_home(slots - 1, slots, k, 6, canon)])
    counts = 2000 + 37 * np.arange(keys.size)
    with nt.KmerTable(k, path, 6144, ctx) as t:
        count(t, M.records_for(keys, counts, k, seed=3))
        assert_exact(t, keys, counts, ("race", path, k))


# ---- (c) chunk seams, exact against the oracle -------------------------------------------------------------------------------

SEAMS = (M.CHUNK, 2 * M.CHUNK, 3 * M.CHUNK)
SEAM_KS = (1, 2, 16, 17, 18, 21, 31, 32)   # halos 0, 16 (17 fits it exactly, 18 is one over) and 32


def _bases(rng, n, noise=0.06):
    """n bytes of record: bases with some lower case, U / u and N."""
    r = ACGT[rng.integers(0, 4, n)].copy()
    m = rng.random(n) < noise
    r[m] = np.frombuffer(b"acgtUuN", dtype=np.uint8)[rng.integers(0, 7, int(m.sum()))]
    return r.tobytes()


class SeamBuffer:
    """One device batch (and quality stream) of break bytes, reused for every layout: small regions of records are written where a
    layout puts them; the oracle only has to read the regions."""

    def __init__(self, n_max):
        self.dev = torch.full((n_max + 64,), ord("\n"), dtype=torch.uint8, device="cuda")
        self.qual = torch.full_like(self.dev, 0xFF)
        self.rng = np.random.default_rng(0x5EA)

    def lay(self, placed):
        """placed: (start, bytes) regions, ascending, each ending in a break byte or at the input's end.  Returns the regions and
        their quality bytes, concatenated."""
        self.dev.fill_(ord("\n"))
        self.qual.fill_(0xFF)
        regions, quals, end = [], [], 0
        for start, reg in placed:
            assert start >= end + 1
            q = self.rng.integers(33, 75, len(reg)).astype(np.uint8)
            self.dev[start:start + len(reg)] = torch.from_numpy(np.frombuffer(reg, dtype=np.uint8).copy()).cuda()
            self.qual[start:start + len(reg)] = torch.from_numpy(q).cuda()
            regions.append(reg if reg.endswith(b"\n") else reg + b"\n")
            quals.append(np.append(q, 0xFF) if not reg.endswith(b"\n") else q)
            end = start + len(reg)
        torch.cuda.synchronize()
        return b"".join(regions), np.concatenate(quals)


def _around(seed, rec, offset, seam):
    """Random records, then `rec` so that `seam` falls on its byte `offset` (offset len(rec): on its break byte), then random
    records.  Returns (start, bytes)."""
    before, after = pack(random_records(seed, 5)), pack(random_records(seed + 1, 5))
    return seam - len(before) - offset, before + rec + b"\n" + after


class Tables:
    def __init__(self, ctx):
        self.ctx, self.t = ctx, {}

    def __call__(self, k, path):
        if (k, path) not in self.t:
            self.t[k, path] = nt.KmerTable(k, path, 1 << 15, self.ctx)
        t = self.t[k, path]
        t.reset()
        return t

    def close(self):
        for t in self.t.values():
            t.close()


def _check_layout(tables, buf, n_bytes, ref, ref_qual, ks, what, quality=True):
    masked = quality_masked(ref, ref_qual)
    for path, pre in PATH_PRES:
        for k in ks:
            t = tables(k, path)
            t.count_device(buf.dev, n_bytes, pre)
            assert_items(t, oracle_items(ref, k, path, pre), (what, path, pre, k))
            if quality:
                t = tables(k, path)
                t.count_device(buf.dev, n_bytes, pre, d_qual=buf.qual, quality_cutoff=CUTOFF)
                assert_items(t, oracle_items(masked, k, path, pre), (what, "quality", path, pre, k))


def test_chunk_seams_item_by_item(ctx):
    """Seams at 64, 128 and 192 MiB, each falling on byte 0..33 of a record (every k's halo, the exact fit of k = 17 and one byte
    over it), on the break byte after a record of exactly k bases, on that record's last base, and on the first base of a record of
    exactly k bases after a break: items equal the oracle's on every path and pre-step, with and without a quality stream."""
    n_bytes = SEAMS[-1] + 8192
    buf, tables = SeamBuffer(n_bytes), Tables(ctx)
    rng = np.random.default_rng(0x5EAB)
    try:
        offsets = list(range(34))
        for g in range(0, len(offsets), len(SEAMS)):
            placed = [_around(1000 * g + 10 * i, _bases(rng, int(rng.integers(40, 64))), o, s)
                      for i, (o, s) in enumerate(zip(offsets[g:g + len(SEAMS)], SEAMS))]
            ref, q = buf.lay(placed)
            _check_layout(tables, buf, n_bytes, ref, q, SEAM_KS, ("offsets", offsets[g:g + len(SEAMS)]))
        for k in SEAM_KS:
            placed = [_around(7000 + k, _bases(rng, k, 0), k, SEAMS[0]),        # ends at seam - 1: the seam is on its break byte
                      _around(7100 + k, _bases(rng, k, 0), k - 1, SEAMS[1]),    # ends at the seam
                      _around(7200 + k, _bases(rng, k, 0), 0, SEAMS[2])]        # starts at the seam, after a break byte
            ref, q = buf.lay(placed)
            _check_layout(tables, buf, n_bytes, ref, q, (k,), ("k-base records", k))
    finally:
        tables.close()


def test_input_ending_just_past_a_chunk_start(ctx):
    """n_bytes = 64 MiB + d, d in {0, 1, 15, 16, 17, 33}: the second chunk is shorter than a halo or the last record's tail.  The
    last record's break byte is the input's last byte, or the record runs to the last byte with no break byte after it."""
    buf, tables = SeamBuffer(M.CHUNK + 64), Tables(ctx)
    rng = np.random.default_rng(0xE0F)
    try:
        for d in (0, 1, 15, 16, 17, 33):
            n_bytes = M.CHUNK + d
            for tail in (b"\n", b""):
                reg = pack(random_records(d, 5)) + _bases(rng, 50) + tail
                ref, q = buf.lay([(n_bytes - len(reg), reg)])
                _check_layout(tables, buf, n_bytes, ref, q, SEAM_KS, ("end", d, tail), quality=False)
    finally:
        tables.close()


def test_scratch_grows_between_unsynchronised_calls(ctx):
    """A 1 MB call, then at once a 196 MB call on the same table (its scratch grows while the first call may still run): the same
    items as one call on a fresh table over both inputs."""
    small = pack(random_records(0xC0020, 5000))
    small += b"\n" * (-len(small) % 16)
    n_small, n_reads, L = len(small), 1_300_000, 150
    n_big = n_reads * (L + 1)
    dev = torch.full((n_small + n_big + 1024,), ord("\n"), dtype=torch.uint8, device="cuda")
    dev[:n_small] = torch.from_numpy(np.frombuffer(small, dtype=np.uint8).copy()).cuda()
    ctx.synth_reads_device(0x5EED0008, 0, n_reads, L, 2, dev.data_ptr() + n_small)
    torch.cuda.synchronize()
    ctx.synchronize()
    for path, pre, k in ((nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE, 11), (nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 21)):
        with nt.KmerTable(k, path, n_small + n_big, ctx) as a, nt.KmerTable(k, path, n_small + n_big, ctx) as b:
            a.count_device(dev, n_small, pre)
            a.count_device(dev.data_ptr() + n_small, n_big, pre)
            b.count_device(dev, n_small + n_big, pre)
            sa, sb = a.stats(), b.stats()
            assert sa["n_dropped"] == 0 and sa == sb, (sa, sb)
            ka, ca = device_items(a)
            kb, cb = device_items(b)
            assert torch.equal(ka, kb) and torch.equal(ca, cb), (path, k)
            del ka, ca, kb, cb
        with nt.KmerTable(k, path, n_small, ctx) as s:   # the small part alone, against the oracle
            s.count_device(dev, n_small, pre)
            assert_items(s, oracle_items(small, k, path, pre), ("small", path, k))
    del dev
    torch.cuda.empty_cache()


# ---- (d) spectrum and extract edges, with designed counts --------------------------------------------------------------------

SPECTRUM_BINS = (2, 3, 64, 16384)
DESIGNED = sorted({c for n in SPECTRUM_BINS for c in (n - 2, n - 1, n, 3 * n)} - {0} | {1})


def _want_spectrum(counts, n_bins):
    h = np.zeros(n_bins, dtype=np.uint64)
    for c in counts:
        h[min(int(c), n_bins - 1)] += 1
    return h


@pytest.mark.parametrize("ones", [0, 62, 63, 64, 16382, 16383, 16384])
def test_spectrum_clamp_and_extract_bounds(ctx, ones):
    """Keys counted exactly n_bins - 2, n_bins - 1, n_bins and 3 n_bins times (and once), the all-ones side word (k = 32, forward)
    below, at and above the clamp bin: spectrum, extract at each min_count edge and extract's cap edge."""
    k = 32
    keys = M.keys_with_home(0, 1, k, len(DESIGNED))
    counts = np.array(DESIGNED, dtype=np.uint64)
    buf = M.records_for(keys, counts, k) + (b"T" * k + b"\n") * ones
    all_keys = np.append(keys, np.uint64(M64)) if ones else keys
    all_counts = np.append(counts, np.uint64(ones)) if ones else counts
    lib = counting.lib()
    with nt.KmerTable(k, nt.PATH_BITS, 64, ctx) as t:
        count(t, buf)
        assert_exact(t, all_keys, all_counts, ("designed", ones))
        assert t.lookup(M64) == ones
        for n_bins in sorted(set(SPECTRUM_BINS) | {4, 5, 62, 63, 65, 16383}):
            assert np.array_equal(t.spectrum(n_bins), _want_spectrum(all_counts, n_bins)), n_bins
        h = np.zeros(16385, dtype=np.uint64)
        for n_bins in (0, 1, 16385):
            assert lib.ntk_kmer_table_spectrum(t._h, h.ctypes.data, n_bins) == ERR_BAD_ARG, n_bins
        order = np.argsort(all_keys)
        sk, sc = all_keys[order], all_counts[order]
        for mc in (0, 1, 2, 62, 63, 64, 65, 16383, 16384, 16385, M64):
            sel = sc >= max(mc, 1)
            got = t.items(mc)
            assert np.array_equal(got[0], sk[sel]) and np.array_equal(got[1], sc[sel]), mc
        need = len(all_keys)
        dk = torch.zeros(need, dtype=torch.int64, device="cuda")
        dc = torch.zeros_like(dk)
        n = C.c_uint64(0)
        args = (C.c_void_p(dk.data_ptr()), C.c_void_p(dc.data_ptr()))
        assert lib.ntk_kmer_table_extract_device(t._h, 1, *args, need - 1, C.byref(n)) == ERR_CAPACITY and n.value == need
        assert not dk.any()
        assert lib.ntk_kmer_table_extract_device(t._h, 1, *args, need, C.byref(n)) == 0 and n.value == need
        assert np.array_equal(dk.cpu().numpy().view(np.uint64), sk) and np.array_equal(dc.cpu().numpy().view(np.uint64), sc)


def test_empty_and_reset_tables_read_as_zeros(ctx):
    k = 32
    keys = M.keys_with_home(0, 1, k, 3)
    probe = np.append(keys, [np.uint64(0), np.uint64(M64)])
    with nt.KmerTable(k, nt.PATH_BITS, 64, ctx) as t:
        for filled in (False, True):
            if filled:
                count(t, M.records_for(keys, [1, 2, 3], k) + (b"T" * k + b"\n") * 5)
                assert t.stats()["n_distinct"] == 4
                t.reset()
            st = t.stats()
            assert (st["n_distinct"], st["n_total"], st["n_dropped"]) == (0, 0, 0), st
            assert len(t.items()[0]) == 0 and len(t.items(0)[0]) == 0
            for n_bins in (2, 64, 16384):
                assert not t.spectrum(n_bins).any()
            assert not t.lookup(probe).any()


# ---- (e) 64-bit counts and the hot key ---------------------------------------------------------------------------------------

HOT_LEN = 1 << 30
# Every occurrence of a table key is one per-lane atomic add to its slot: calls of 2^30 - 20 occurrences of one key, enough to
# carry the slot's count past 2^32 (profiles/count/README.md, workload (c), has the rate).
HOT_CALLS = 5


def _hot_run(ctx, base, k, path, calls):
    dev = torch.full((HOT_LEN + 64,), ord("\n"), dtype=torch.uint8, device="cuda")
    dev[:HOT_LEN] = base
    torch.cuda.synchronize()
    n = calls * (HOT_LEN - k + 1)
    with nt.KmerTable(k, path, 16, ctx) as t:
        for _ in range(calls):
            t.count_device(dev, HOT_LEN + 1, nt.PRE_NONE)
        st = t.stats()
        assert (st["n_distinct"], st["n_total"], st["n_dropped"]) == (1, n, 0), st
        key = M64 if base == ord("T") and path == nt.PATH_BITS else 0
        keys, counts = t.items()
        assert list(keys) == [key] and list(counts) == [n]
        assert t.lookup(key) == n and t.lookup(b"T" * k) == n
        assert list(t.spectrum(16384)[-1:]) == [1] and t.spectrum(16384).sum() == 1 and list(t.spectrum(2)) == [0, 1]
        assert len(t.items(n)[0]) == 1 and len(t.items(n + 1)[0]) == 0
    del dev
    torch.cuda.empty_cache()
    return n


def test_side_word_counts_past_2_32(ctx):
    """TTT...T forward at k = 32 is the side word's key; 5 (2^30 - 31) occurrences > 2^32."""
    assert _hot_run(ctx, ord("T"), 32, nt.PATH_BITS, 5) > 1 << 32


def test_hot_table_slot_counts_past_2_32(ctx):
    """One record of 2^30 A at k = 21 on the canonical bits path: every lane adds to one table slot, HOT_CALLS times."""
    assert _hot_run(ctx, ord("A"), 21, nt.PATH_BITS_CANONICAL, HOT_CALLS) > 1 << 32


# ---- (f) two devices ---------------------------------------------------------------------------------------------------------

def test_tables_on_two_devices(ctx):
    n_dev = torch.cuda.device_count()
    if n_dev < 2:
        pytest.skip("one visible device")
    last = n_dev - 1
    buf = pack(random_records(0xC0021))
    k, path, pre = 21, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE
    want = oracle_items(buf, k, path, pre)
    d0, dn = upload(buf), upload(buf, device=f"cuda:{last}")
    with nt.Context(last) as cn, nt.KmerTable(k, path, len(buf), ctx) as a, nt.KmerTable(k, path, len(buf), cn) as b:
        b.count_device(dn, len(buf), pre)
        assert_items(b, want, "last device")
        for _ in range(2):   # interleaved, no synchronisation in between
            a.count_device(d0, len(buf), pre)
            b.count_device(dn, len(buf), pre)
        assert_items(a, (want[0], want[1] * 2), "device 0")
        assert_items(b, (want[0], want[1] * 3), "last device, interleaved")
