"""MinHash sketches (include/needletail_amd_minhash.h, needletail_amd.KmerMinHash) on a real MI355X.

Truth for the hashes and their counts: the host model tests/_minhash_model.py applied to the oracle's literal iterators - `oracle_values`
(tests/_count_helpers.py) for k <= 32, the {hi, lo} words of canonical_kmers_arrays (the wide count tests' oracle_items) for k >= 33.
Hashes and counts are compared with array_equal, n_windows exactly.  Every case asserts the sizes that make it mean something."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import minhashing  # noqa: E402
import _count_model as CM  # noqa: E402
import _minhash_model as M  # noqa: E402
from _count_helpers import CUTOFF, PATH_PRES, oracle_values, pack, quality_masked, random_records, upload  # noqa: E402
from test_gpu_wide_count import oracle_items as wide_oracle_items  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (1, 3, 7, 16, 21, 31, 32)
WIDE_KS = (33, 34, 40, 51, 62, 63)
NUMS = (1, 16, 500, 10 ** 6)
SCALEDS = (1, 7, 1000)
KINDS = [dict(num=n) for n in NUMS] + [dict(scaled=s) for s in SCALEDS]
BYTES = nt.PATH_BYTES_CANONICAL
ERR_BAD_K, ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 1, 2, 5, 6
FILTER_THREADS = 256   # kFilterThreads of ntk_minhash.hip (tests/test_minhash_abi.py ties the two)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def oracle_keys(buf: bytes, k: int, path: int, pre: int) -> np.ndarray:
    """Every key the batch emits, with repeats: narrow values, or [hi, lo] rows at k >= 33."""
    if k <= 32:
        return oracle_values(buf, k, path, pre)
    keys, counts = wide_oracle_items(buf, k)
    return np.repeat(keys, counts, axis=0)


def kind_of(mh) -> dict:
    return dict(num=mh.num) if mh.num else dict(scaled=mh.scaled)


def assert_minhash(mh, keys, what, windows=None):
    """The handle's hashes, counts and stats are the model's on this multiset of keys."""
    kind = kind_of(mh)
    want = M.sketch(keys, **kind)
    h, c = mh.hashes()
    assert h.dtype == np.uint64 and c.dtype == np.uint64
    assert np.array_equal(h, want[0]), (what, h.size, want[0].size)
    assert np.array_equal(c, want[1]), (what, int((c != want[1]).sum()))
    st = mh.stats()
    assert st["n_windows"] == (len(keys) if windows is None else windows), (what, st)
    assert st["n_kept"] == h.size and st["threshold"] == M.threshold(want[0], **kind), (what, st)
    assert (st["k"], st["path"], st["num"], st["scaled"]) == (mh.k, mh.path, mh.num, mh.scaled)
    return st, want


# ---- 1. and 2. exact against the model on the oracle's k-mers ---------------------------------------------------------------------------

def _qualities(seed, n):
    """A quality stream that masks about 1 % of the bases at CUTOFF: enough windows survive, at every k, for the bottom-s cut and the
    scaled threshold to be met on masked data (a uniform 33..75 leaves no window of 63 bases)."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.01, rng.integers(33, CUTOFF, n), rng.integers(CUTOFF, 75, n)).astype(np.uint8)


def _assert_mask_bites(masked_keys, keys):
    """The masked batch loses windows, and keeps more distinct keys than the largest finite num and some hash under scaled = 1000."""
    distinct = np.unique(masked_keys, axis=0).shape[0]
    assert distinct > max(n for n in NUMS if n < 10 ** 6) and 0 < masked_keys.shape[0] < keys.shape[0]
    assert len(M.sketch(masked_keys, scaled=max(SCALEDS))[0]) >= 3


@functools.lru_cache(maxsize=None)
def _narrow_batch():
    recs = random_records(0x3A0017)
    buf = pack(recs)
    qual = _qualities(7, len(buf))
    return recs, buf, qual, quality_masked(buf, qual)


def test_random_records_match_the_model(ctx):
    recs, buf, qual, masked = _narrow_batch()
    dev, dq = upload(buf), upload(qual.tobytes(), fill=0xFF)
    for path, pre in PATH_PRES:
        for k in KS:
            keys = oracle_keys(buf, k, path, pre)
            distinct = np.unique(keys).size
            assert keys.size > 10_000 and (500 < distinct < 10 ** 6 or k <= 3)
            masked_keys = oracle_keys(masked, k, path, pre) if k in (7, 21, 32) else None
            for kind in KINDS:
                with nt.KmerMinHash(k, path, ctx=ctx, **kind) as mh:
                    mh.add_device(dev, len(buf), pre)
                    st, want = assert_minhash(mh, keys, (path, pre, k, kind))
                    if kind.get("num"):
                        assert st["n_kept"] == min(kind["num"], distinct)
                    if kind.get("scaled") == 1:
                        assert st["n_kept"] == distinct and int(want[1].sum()) == keys.size
                    if kind.get("scaled") == 1000 and k >= 16:
                        assert st["n_kept"] >= 8, (k, st)
                    if k in (7, 21, 32):
                        # the packer route: the same records through ntk_batch_append
                        mh.reset()
                        mh.add_records(recs, pre)
                        assert_minhash(mh, keys, ("records", path, pre, k, kind))
                        # a quality stream and a cutoff mask bases as the tables do
                        mh.reset()
                        mh.add_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=CUTOFF)
                        assert_minhash(mh, masked_keys, ("quality", path, pre, k, kind))
                        _assert_mask_bites(masked_keys, keys)


def test_random_records_match_the_model_wide(ctx):
    recs = random_records(0x3B0017, 200)
    buf = pack(recs)
    dev = upload(buf)
    qual = _qualities(8, len(buf))
    dq, masked = upload(qual.tobytes(), fill=0xFF), quality_masked(buf, qual)
    for k in WIDE_KS:
        keys = oracle_keys(buf, k, BYTES, nt.PRE_NORMALIZE)
        distinct = np.unique(keys, axis=0).shape[0]
        assert keys.shape[0] > 10_000 and distinct > 8000
        masked_keys = oracle_keys(masked, k, BYTES, nt.PRE_NORMALIZE) if k in (40, 63) else None
        for pre in (nt.PRE_NORMALIZE, nt.PRE_NORMALIZE_IUPAC):
            for kind in KINDS:
                with nt.KmerMinHash(k, BYTES, ctx=ctx, **kind) as mh:
                    mh.add_device(dev, len(buf), pre)
                    st, _ = assert_minhash(mh, keys, (pre, k, kind))
                    if kind.get("num"):
                        assert st["n_kept"] == min(kind["num"], distinct)
                    if kind.get("scaled") == 1000:
                        assert st["n_kept"] >= 8, (k, st)
                    if pre == nt.PRE_NORMALIZE and k in (40, 63):
                        mh.reset()
                        mh.add_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=CUTOFF)
                        assert_minhash(mh, masked_keys, ("quality", k, kind))
                        _assert_mask_bites(masked_keys, keys)
                        mh.reset()   # cutoff 0: no mask
                        mh.add_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=0)
                        assert_minhash(mh, keys, ("no mask", k, kind))


# ---- 3. overflow and redo at the smallest shape -------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 51])
@pytest.mark.parametrize("buffer_entries", [64, 256])
def test_overflow_and_redo(ctx, k, buffer_entries):
    """A buffer far smaller than the number of passing hashes: launches are discarded and redone, the buffer is merged many times, and
    every count is still exact."""
    recs, buf, _, _ = _narrow_batch()
    dev = upload(buf)
    keys = oracle_keys(buf, k, BYTES, nt.PRE_NORMALIZE)
    distinct = np.unique(keys, axis=0).shape[0]
    assert distinct > 5000
    for kind in (dict(scaled=1), dict(num=8), dict(num=500)):
        with nt.KmerMinHash(k, BYTES, ctx=ctx, buffer_entries=buffer_entries, **kind) as mh:
            mh.add_device(dev, len(buf), nt.PRE_NORMALIZE)
            st, want = assert_minhash(mh, keys, (k, buffer_entries, kind))
            assert st["n_redone"] > 0 and st["n_merges"] > 1, st
            assert st["buffer_entries"] == buffer_entries
            assert st["n_kept"] == (distinct if "scaled" in kind else kind["num"])
            # again on top: the counts double, and the second pass of a bottom-s sketch starts with a tight threshold
            mh.add_device(dev, len(buf), nt.PRE_NORMALIZE)
            h, c = mh.hashes()
            assert np.array_equal(h, want[0]) and np.array_equal(c, 2 * want[1])
    with nt.KmerMinHash(k, BYTES, num=8, ctx=ctx) as mh:
        assert mh.stats()["buffer_entries"] == M.BUFFER_DEFAULT


@pytest.mark.parametrize("k", [21, 51])
def test_one_handle_grows_across_calls_and_starts_over(ctx, k):
    """One handle, three batches of about 200, 20 000 and 200 bases: the kept set, the runs, the merge's arrays and rocPRIM's temporary
    storage, sized by the first batch, are all replaced by larger ones in the second call and used again, too large, by the third.  The
    sketch is the model's on everything added so far after every call, and the last batch's alone after a reset."""
    rng = np.random.default_rng(0x3C00 + k)
    bufs = [pack([bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))]) for n in (200, 20_000, 200)]
    keys = [oracle_keys(buf, k, BYTES, nt.PRE_NORMALIZE) for buf in bufs]
    assert [len(v) for v in keys] == [200 - k + 1, 20_000 - k + 1, 200 - k + 1]
    for kind in (dict(scaled=2), dict(num=64)):
        with nt.KmerMinHash(k, BYTES, ctx=ctx, **kind) as mh:
            for i, buf in enumerate(bufs):
                mh.add_device(upload(buf), len(buf), nt.PRE_NORMALIZE)
                st, _ = assert_minhash(mh, np.concatenate(keys[: i + 1]), (k, kind, "call", i))
                if "scaled" in kind:   # every batch has hashes under a fixed threshold (a bottom-s threshold may let none of a batch in)
                    assert st["n_merges"] >= i + 1
            if "scaled" in kind:
                assert st["n_kept"] > 20 * (200 - k + 1)   # far more than the first call's arrays held
            mh.reset()
            mh.add_device(upload(bufs[2]), len(bufs[2]), nt.PRE_NORMALIZE)
            assert_minhash(mh, keys[2], (k, kind, "after reset"))


# ---- 4. a tie at the threshold ------------------------------------------------------------------------------------------------------

def test_a_tie_at_the_threshold(ctx):
    """Keys whose hashes are 0..19, the key ~0 (T^32) and the key whose hash is ~0, at k = 32 on the forward bit path.  With num = 10
    the threshold is the hash 9 after the first batch; a second batch repeats the 10th and 11th smallest hashes 40 times each: the
    repeats of the 10th are at the threshold and must count (the test is h <= tau), the 11th stays out."""
    k, path, pre = 32, nt.PATH_BITS, nt.PRE_NONE
    hashes = np.concatenate([np.arange(20, dtype=np.uint64), np.array([M.ALL], dtype=np.uint64)])
    keys = CM.fmix64_inv(hashes) ^ np.uint64(M.XOR)
    assert int(keys[0]) == M.XOR and np.array_equal(M.sketch(keys, scaled=1)[0], hashes)
    keys = np.concatenate([keys, np.array([M.ALL], dtype=np.uint64)])   # TTT...T
    t_hash = int(M.sketch(keys[-1:], scaled=1)[0][0])
    assert 19 < t_hash < M.ALL and np.unique(keys).size == 22
    counts = np.random.default_rng(4).integers(1, 6, keys.size)
    first = CM.records_for(keys, counts, k, seed=1)
    second = CM.records_for(keys[9:11], [40, 40], k, seed=2)
    d1, d2 = upload(first), upload(second)
    m1, m2 = oracle_keys(first, k, path, pre), oracle_keys(second, k, path, pre)
    assert m1.size == int(counts.sum()) > 64 and m2.size == 80
    with nt.KmerMinHash(k, path, num=10, ctx=ctx, buffer_entries=64) as mh:
        mh.add_device(d1, len(first), pre)
        st, want = assert_minhash(mh, m1, "first")
        assert st["threshold"] == 9 and st["n_kept"] == 10 and want[1].tolist() == counts[:10].tolist()
        mh.add_device(d2, len(second), pre)
        st, want = assert_minhash(mh, np.concatenate([m1, m2]), "both")
        assert st["threshold"] == 9 and want[0].tolist() == list(range(10)) and int(want[1][9]) == int(counts[9]) + 40
    with nt.KmerMinHash(k, path, scaled=1, ctx=ctx, buffer_entries=64) as mh:
        mh.add_device(d1, len(first), pre)
        mh.add_device(d2, len(second), pre)
        st, want = assert_minhash(mh, np.concatenate([m1, m2]), "scaled")
        h, c = mh.hashes()
        assert h.size == 22 and int(h[-1]) == M.ALL and int(h[0]) == 0 and int(c[10]) == int(counts[10]) + 40
        assert st["threshold"] == M.ALL


# ---- 5. a function of the key multiset: order, splits, repeats ----------------------------------------------------------------------

def _cuts(buf: bytes, pieces: int):
    """Record-aligned, 16-byte-aligned cut points that split buf into about `pieces` calls."""
    ends = [i + 1 for i in range(len(buf)) if buf[i:i + 1] == b"\n" and (i + 1) % 16 == 0]
    want = [len(buf) * j // pieces for j in range(1, pieces)]
    cuts = sorted({min(ends, key=lambda e: abs(e - w)) for w in want})
    return [0, *cuts, len(buf)]


@pytest.mark.parametrize("k,path,pre", [(11, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE), (21, BYTES, nt.PRE_NORMALIZE),
                                        (45, BYTES, nt.PRE_NORMALIZE)])
def test_order_split_and_repeat_invariance(ctx, k, path, pre):
    recs = random_records(0x3A0019, 400)
    buf = pack(recs)
    dev = upload(buf)
    keys = oracle_keys(buf, k, path, pre)
    order = np.random.default_rng(3).permutation(len(recs))
    shuffled = pack([recs[i] for i in order])
    ds = upload(shuffled)
    cuts = _cuts(buf, 3)
    assert len(cuts) == 4
    for kind in (dict(num=200), dict(scaled=50)):
        for buffer_entries in (0, 1024):   # 1024: the splits and the repeats meet the redo rule as well
            with nt.KmerMinHash(k, path, ctx=ctx, buffer_entries=buffer_entries, **kind) as mh:
                mh.add_device(dev, len(buf), pre)
                st, want = assert_minhash(mh, keys, "one call")
                assert st["n_kept"] >= 200
                mh.reset()
                st = mh.stats()
                assert st["n_kept"] == 0 and st["n_windows"] == 0 and st["n_merges"] == 0 and st["n_redone"] == 0
                mh.add_device(ds, len(shuffled), pre)
                assert_minhash(mh, keys, "shuffled")
                mh.reset()
                for a, b in zip(cuts[:-1], cuts[1:]):
                    mh.add_device(dev.data_ptr() + a, b - a, pre)
                assert_minhash(mh, keys, "three calls")
                mh.add_device(dev, len(buf), pre)   # the same batch again: the hashes stay, the counts double
                h, c = mh.hashes()
                assert np.array_equal(h, want[0]) and np.array_equal(c, 2 * want[1])
                assert mh.stats()["n_windows"] == 2 * len(keys)


# ---- 6. merge -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 51])
def test_merge(ctx, k):
    lib = minhashing.lib()
    ra, rb = random_records(0x3A001A, 300), random_records(0x3A001B, 200)
    a, b = pack(ra), pack(rb + ra[:50])   # the halves share records: counts of equal hashes add
    pre = nt.PRE_NORMALIZE
    ka, kb = oracle_keys(a, k, BYTES, pre), oracle_keys(b, k, BYTES, pre)
    both = np.concatenate([ka, kb])
    da, db = upload(a), upload(b)
    for kind in (dict(num=300), dict(scaled=20)):
        with nt.KmerMinHash(k, BYTES, ctx=ctx, **kind) as sa, nt.KmerMinHash(k, BYTES, ctx=ctx, **kind) as sb:
            sa.add_device(da, len(a), pre)
            sb.add_device(db, len(b), pre)
            ha, ca = sa.hashes()
            want_b = M.sketch(kb, **kind)
            shared = np.intersect1d(ha, want_b[0]).size
            assert shared > 20 and shared < ha.size
            sb.merge(sa)                                   # a sketch object
            st, want = assert_minhash(sb, both, ("A into B", kind))
            assert np.array_equal(M.merge((ha, ca), want_b, **kind)[0], want[0])
            sb.reset()
            sb.merge(ha, ca, n_windows=len(ka))            # bare arrays into an empty handle: how a sketch travels
            assert_minhash(sb, ka, ("into an empty handle", kind))
            sb.merge(ha, None, n_windows=5)                # counts = None: every count 1
            h, c = sb.hashes()
            assert np.array_equal(h, ha) and np.array_equal(c, ca + np.uint64(1)) and sb.stats()["n_windows"] == len(ka) + 5
            sb.merge(ha[:0], None, n_windows=7)            # nothing but windows
            assert sb.stats()["n_windows"] == len(ka) + 12 and np.array_equal(sb.hashes()[1], ca + np.uint64(1))
            # ascending order is enforced; wrong types and lengths; n_windows is required with bare arrays
            for bad in (ha[::-1].copy(), np.concatenate([ha[:5], ha[4:9]])):
                with pytest.raises(nt.NtkError) as e:
                    sb.merge(bad, None, n_windows=1)
                assert e.value.status == ERR_BAD_ARG
            for bad, cnt in ((ha.astype(np.int64), None), (ha, ca[:-1]), (ha.reshape(1, -1), None)):
                with pytest.raises(nt.NtkError) as e:
                    sb.merge(bad, cnt, n_windows=1)
                assert e.value.status == ERR_BAD_ARG
            with pytest.raises(TypeError):
                sb.merge(ha, ca)
            assert lib.ntk_minhash_merge(sb._h, None, None, 3, 0) == ERR_BAD_ARG
            assert lib.ntk_minhash_merge(None, ha.ctypes.data, None, 3, 0) == ERR_BAD_ARG
            # k and path mismatches are refused in Python
            with nt.KmerMinHash(k - 1, BYTES, ctx=ctx, **kind) as other, pytest.raises(nt.NtkError):
                sb.merge(other)
            if k <= 32:
                with nt.KmerMinHash(k, nt.PATH_BITS_CANONICAL, ctx=ctx, **kind) as other, pytest.raises(nt.NtkError):
                    sb.merge(other)
            assert sb.stats()["n_windows"] == len(ka) + 12 and np.array_equal(sb.hashes()[1], ca + np.uint64(1))   # unchanged
            # the comparison of the two handles is the model's on their sketches
            sb.reset()
            sb.add_device(db, len(b), pre)
            num = kind.get("num", 0)
            want_cmp = M.compare(ha, ca, *want_b, num, M.max_hash(kind["scaled"]) if "scaled" in kind else M.ALL)
            got = sa.compare(sb)
            assert all(got[key] == want_cmp[key] for key in ("n_a", "n_b", "n_shared", "n_union")) and got["n_shared"] > 0
            j = want_cmp["n_shared"] / want_cmp["n_union"]
            assert sa.jaccard(sb) == j and 0 < j < 1 and sa.jaccard(sa) == 1.0 and sa.mash_distance(sa) == 0.0
            assert sa.mash_distance(sb) == max(0.0, -math.log(2.0 * j / (1.0 + j)) / k) > 0
            assert sa.containment(sb) == want_cmp["n_shared"] / want_cmp["n_a"]
            assert sa.cosine(sb) == pytest.approx(want_cmp["dot"] / np.sqrt(want_cmp["norm2_a"] * want_cmp["norm2_b"]), rel=1e-12)
            assert sa.cosine(sa) == pytest.approx(1.0, rel=1e-12)


# ---- 7. and 8. seams ---------------------------------------------------------------------------------------------------------------

def test_chunk_boundaries_are_taken_once(ctx):
    """A batch of more than 64 MiB (the chunk) whose records straddle the chunk boundary: n_windows is the reduce face's n_total, and
    the sketch is that of the same batch added in two record-aligned pieces that each fit one chunk."""
    n_reads, L = 500_000, 150
    nbytes = n_reads * (L + 1)
    assert nbytes > M.CHUNK and M.CHUNK % (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0007, 0, n_reads, L, 2, dev)
    cut = (n_reads // 2) // 16 * 16 * (L + 1)   # a record boundary and a multiple of 16
    assert cut < M.CHUNK and nbytes - cut < M.CHUNK
    for path, pre, k in ((BYTES, nt.PRE_NORMALIZE, 21), (nt.PATH_BITS, nt.PRE_STRIP_RETURNS, 32)):
        ctx.accum_reset()
        ctx.reduce_device(dev, nbytes, k, path, pre)
        n_total = ctx.accum_read()["n_total"]
        for kind in (dict(num=1000), dict(scaled=100_000)):
            with nt.KmerMinHash(k, path, ctx=ctx, **kind) as mh:
                mh.add_device(dev, nbytes, pre)
                (h, c), st = mh.hashes(), mh.stats()
                assert st["n_windows"] == n_total, (k, st, n_total)
                assert h.size == 1000 if "num" in kind else h.size >= 100, (k, kind, h.size)
                assert np.all(h[1:] > h[:-1]) and c.min() >= 1 and st["n_redone"] == 0
                mh.reset()
                mh.add_device(dev, cut, pre)
                mh.add_device(dev.data_ptr() + cut, nbytes - cut, pre)
                h2, c2 = mh.hashes()
                assert np.array_equal(h2, h) and np.array_equal(c2, c) and mh.stats()["n_windows"] == n_total, (k, kind)
    del dev
    torch.cuda.empty_cache()


def test_wide_kernel_seams(ctx):
    """A break (record end, N, masked quality) at every offset -k..k around every lane-run seam (64 bytes) of a batch that spans
    three blocks of the wide filter kernel; then readable padding of A past an n_bytes that is not a multiple of 16."""
    rng = np.random.default_rng(0x3EB)
    span = 2 * FILTER_THREADS * M.LANE_RUN + 3 * M.LANE_RUN + 5
    for k in (33, 63):
        with nt.KmerMinHash(k, BYTES, scaled=1, ctx=ctx) as mh:
            for d in range(-k, k + 1):
                a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, span)].copy()
                at = np.arange(M.LANE_RUN, span, M.LANE_RUN) + d
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
                mh.reset()
                dev, dq = upload(buf), upload(qual.tobytes())
                mh.add_device(dev, len(buf), nt.PRE_NORMALIZE, d_qual=dq, quality_cutoff=CUTOFF)
                keys = oracle_keys(quality_masked(buf, qual), k, BYTES, nt.PRE_NORMALIZE)
                assert keys.shape[0] > 0
                assert_minhash(mh, keys, ("seam", k, d))
            for n_bytes in (span - 16 * 3 - 1, 100, k, k - 1, 1):
                buf = bytes(a[:n_bytes])
                mh.reset()
                dev = upload(buf, fill=ord("A"))
                mh.add_device(dev, n_bytes, nt.PRE_NORMALIZE)
                assert_minhash(mh, oracle_keys(buf, k, BYTES, nt.PRE_NORMALIZE), ("padding", k, n_bytes))


# ---- 9. nothing to add ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,path,pre", [(21, nt.PATH_BITS_CANONICAL, nt.PRE_NONE), (21, BYTES, nt.PRE_NORMALIZE), (51, BYTES, nt.PRE_NORMALIZE)])
def test_inputs_without_a_window(ctx, k, path, pre):
    lib = minhashing.lib()
    for kind, threshold in ((dict(num=16), M.ALL), (dict(scaled=1000), M.ALL // 1000)):
        with nt.KmerMinHash(k, path, ctx=ctx, **kind) as mh:
            p = NL.Params(k, path, pre, 0)
            assert lib.ntk_minhash_add_device(mh._h, None, None, 0, C.byref(p)) == 0           # empty input
            bufs = (b"ACGTACGTAC", b"A" * (k - 1), b"\n" * 1000, b"N" * 300 + b"\n" + b"-" * 77, (b"A" * (k - 1) + b"\n") * 50)
            devs = [upload(buf, fill=ord("A")) for buf in bufs]
            for buf, dev in zip(bufs, devs):
                mh.add_device(dev, len(buf), pre)
            st = mh.stats()
            assert st["n_kept"] == 0 and st["n_windows"] == 0 and st["threshold"] == threshold and st["n_redone"] == 0
            h, c = mh.hashes()
            assert h.size == 0 and c.size == 0
            n = C.c_uint64(99)
            assert lib.ntk_minhash_read(mh._h, None, None, 0, C.byref(n)) == 0 and n.value == 0


# ---- 10. one key many times ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,path,pre", [(21, nt.PATH_BITS_CANONICAL, nt.PRE_NONE), (51, BYTES, nt.PRE_NORMALIZE)])
def test_one_key_2_20_times(ctx, k, path, pre):
    """One record of 2^20 A: every window is the key AAA...A, and each of them is appended (the documented hot-key cost).  With a
    4096-entry buffer the launch is redone in 256 pieces; the one hash comes back with its full count."""
    n = 1 << 20
    dev = torch.full((n + 1024,), ord("\n"), dtype=torch.uint8, device="cuda")
    dev[:n] = ord("A")
    torch.cuda.synchronize()
    key = np.zeros(1, np.uint64) if k <= 32 else np.zeros((1, 2), np.uint64)
    a_hash = int(M.sketch(key, scaled=1)[0][0])
    with nt.KmerMinHash(k, path, scaled=1, ctx=ctx, buffer_entries=4096) as mh:
        mh.add_device(dev, n + 1, pre)
        (h, c), st = mh.hashes(), mh.stats()
        assert h.tolist() == [a_hash] and c.tolist() == [n - k + 1]
        assert st["n_windows"] == n - k + 1 and st["n_redone"] == 1 and st["n_merges"] >= 256
    # after random records, bottom-4: kept or not as the model says, with its full count if kept
    buf = pack(random_records(0x3A001D, 60))
    keys = oracle_keys(buf, k, path, pre)
    db = upload(buf)
    with nt.KmerMinHash(k, path, num=4, ctx=ctx, buffer_entries=4096) as mh:
        mh.add_device(db, len(buf), pre)
        mh.add_device(dev, n + 1, pre)
        st, want = assert_minhash(mh, np.concatenate([keys, np.repeat(key, n - k + 1, axis=0)]), "after records")
        assert st["n_kept"] == 4 and keys.shape[0] > 4096
    with nt.KmerMinHash(k, path, num=4, ctx=ctx, buffer_entries=4096) as mh:   # alone it is kept, whatever its hash
        mh.add_device(dev, n + 1, pre)
        h, c = mh.hashes()
        assert h.tolist() == [a_hash] and c.tolist() == [n - k + 1] and mh.stats()["threshold"] == M.ALL
    del dev
    torch.cuda.empty_cache()


# ---- 11. error rules -------------------------------------------------------------------------------------------------------------------

def test_error_cases(ctx):
    lib = minhashing.lib()
    for k, path, status in ((0, BYTES, ERR_BAD_K), (64, BYTES, ERR_BAD_K), (255, BYTES, ERR_BAD_K), (0, nt.PATH_BITS, ERR_BAD_K),
                            (33, nt.PATH_BITS, ERR_BAD_K), (40, nt.PATH_BITS_CANONICAL, ERR_BAD_K), (64, nt.PATH_BITS, ERR_BAD_K),
                            (21, 3, ERR_BAD_ARG), (40, 3, ERR_BAD_ARG)):
        with pytest.raises(nt.NtkError) as e:
            nt.KmerMinHash(k, path, num=100, ctx=ctx)
        assert e.value.status == status, (k, path)
    for kwargs in (dict(), dict(num=5, scaled=5), dict(num=(1 << 20) + 1), dict(num=5, buffer_entries=63),
                   dict(scaled=5, buffer_entries=(1 << 28) + 1), dict(num=5, buffer_entries=1)):
        with pytest.raises(nt.NtkError) as e:
            nt.KmerMinHash(21, BYTES, ctx=ctx, **kwargs)
        assert e.value.status == ERR_BAD_ARG, kwargs
    nt.KmerMinHash(21, BYTES, num=1 << 20, ctx=ctx, buffer_entries=64).close()   # the ends of the ranges exist
    h = C.c_void_p()
    assert lib.ntk_minhash_create(None, 21, BYTES, 10, 0, 0, C.byref(h)) == ERR_BAD_ARG
    assert lib.ntk_minhash_create(ctx._h, 21, BYTES, 10, 0, 0, None) == ERR_BAD_ARG
    assert lib.ntk_minhash_reset(None) == ERR_BAD_ARG
    lib.ntk_minhash_destroy(None)
    for k in (32, 33, 63):   # the ends of both routes exist
        nt.KmerMinHash(k, BYTES, scaled=10, ctx=ctx).close()
    buf = pack(random_records(0x3A001C, 40))
    dev, dq = upload(buf), upload(bytes(len(buf)))
    for k in (21, 40):
        with nt.KmerMinHash(k, BYTES, num=50, ctx=ctx) as mh:
            def call(p, seq=dev.data_ptr(), qual=None, n=len(buf)):
                return lib.ntk_minhash_add_device(mh._h, C.c_void_p(seq), None if qual is None else C.c_void_p(qual), n, C.byref(p))
            for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):   # un-normalised byte-path input
                with pytest.raises(nt.NtkError) as e:
                    mh.add_device(dev, len(buf), pre)
                assert e.value.status == ERR_UNSUPPORTED
            assert call(NL.Params(k, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE, 0)) == ERR_BAD_ARG   # path mismatch
            for kk, flags in ((k + 1, 0), (k, 11), (k, NL.FLAG_RESET), (k, 1 << 20)):   # k mismatch, window bits, reset flag, high bits
                assert call(NL.Params(kk, BYTES, nt.PRE_NORMALIZE, flags)) == ERR_BAD_ARG, (kk, flags)
            assert call(NL.Params(k, BYTES, 4, 0)) == ERR_BAD_ARG   # no such pre
            p = NL.Params(k, BYTES, nt.PRE_NORMALIZE, NL.flags(0, CUTOFF))
            assert call(p, seq=dev.data_ptr() + 8, n=len(buf) - 8) == ERR_BAD_ARG     # misaligned d_seq
            assert call(p, qual=dq.data_ptr() + 4) == ERR_BAD_ARG                      # misaligned d_qual
            assert lib.ntk_minhash_add_device(mh._h, None, None, len(buf), C.byref(p)) == ERR_BAD_ARG
            assert lib.ntk_minhash_add_device(mh._h, C.c_void_p(dev.data_ptr()), None, len(buf), None) == ERR_BAD_ARG
            assert lib.ntk_minhash_add_device(None, C.c_void_p(dev.data_ptr()), None, len(buf), C.byref(p)) == ERR_BAD_ARG
            assert call(p, n=0) == 0
            st = mh.stats()
            assert st["n_windows"] == 0 and st["n_kept"] == 0
            assert lib.ntk_minhash_stats(mh._h, None) == ERR_BAD_ARG and lib.ntk_minhash_stats(None, C.byref(minhashing.Stats())) == ERR_BAD_ARG
            # read: a small cap answers the size and writes nothing
            mh.add_device(dev, len(buf), nt.PRE_NORMALIZE)
            n = C.c_uint64(0)
            hh, cc = np.full(50, 7, dtype=np.uint64), np.full(50, 7, dtype=np.uint64)
            assert lib.ntk_minhash_read(mh._h, None, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == 50
            n = C.c_uint64(0)
            assert lib.ntk_minhash_read(mh._h, hh.ctypes.data, cc.ctypes.data, 49, C.byref(n)) == ERR_CAPACITY and n.value == 50
            assert (hh == 7).all() and (cc == 7).all()
            assert lib.ntk_minhash_read(mh._h, hh.ctypes.data, cc.ctypes.data, 50, None) == ERR_BAD_ARG
            assert lib.ntk_minhash_read(mh._h, None, cc.ctypes.data, 50, C.byref(n)) == ERR_BAD_ARG
            assert lib.ntk_minhash_read(None, hh.ctypes.data, cc.ctypes.data, 50, C.byref(n)) == ERR_BAD_ARG
            assert lib.ntk_minhash_read(mh._h, hh.ctypes.data, cc.ctypes.data, 50, C.byref(n)) == 0 and n.value == 50
            assert np.array_equal(hh, mh.hashes()[0]) and np.all(hh[1:] > hh[:-1]) and cc.min() >= 1
    with nt.KmerMinHash(21, nt.PATH_BITS, scaled=10, ctx=ctx) as mh:   # the bit paths take un-normalised input, as the table does
        mh.add_device(dev, len(buf), nt.PRE_NONE)
        assert mh.stats()["n_windows"] > 0
        with nt.KmerMinHash(21, nt.PATH_BITS, num=10, ctx=ctx) as other, pytest.raises(nt.NtkError):
            mh.compare(other)   # a bottom-s sketch against a scaled one


# ---- 12. the example --------------------------------------------------------------------------------------------------------------------

def _records(name):
    return [r.raw_seq for r in nt.parse_fastx_file(os.path.join(GOLDEN, name))]


def test_minhash_sketch_example(ctx):
    exe = os.path.join(ROOT, "examples", "minhash_sketch")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    names = ("28S.fasta", "28S.fasta", "PRJNA271013_head.fq")
    files = [os.path.join(GOLDEN, n) for n in names]
    for args, kind in ((["-k", "21", "-n", "1000"], dict(num=1000)), (["-k", "21", "-s", "10"], dict(scaled=10))):
        r = subprocess.run([exe, *args, *files], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == 6
        sketches = []
        for name, path, line in zip(names, files, lines[:3]):
            with nt.KmerMinHash(21, BYTES, ctx=ctx, **kind) as mh:
                mh.add_records(_records(name), nt.PRE_NORMALIZE)
                st = mh.stats()
                sketches.append(mh.hashes())
            assert line.split("\t") == [path, str(st["n_windows"]), str(st["n_kept"])] and st["n_kept"] > 100
        matrix = [[float(x) for x in line.split("\t")] for line in lines[3:]]
        assert matrix[0][1] == matrix[1][0] == 1.0 and all(matrix[i][i] == 1.0 for i in range(3))
        max_hash = M.max_hash(kind["scaled"]) if "scaled" in kind else M.ALL
        for i in range(3):
            for j in range(3):
                c = minhashing.compare(*sketches[i], *sketches[j], kind.get("num", 0), max_hash)
                assert matrix[i][j] == float(f"{c['n_shared'] / c['n_union']:.6f}"), (i, j)
    assert subprocess.run([exe, "-k", "21", files[0]], capture_output=True, timeout=60).returncode == 2   # neither -n nor -s
