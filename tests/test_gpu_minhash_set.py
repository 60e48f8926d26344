"""The device-resident set of MinHash sketches and its all-pairs comparison (include/needletail_amd_minhash_set.h,
needletail_amd.MinHashSet) on a real MI355X.

Truth: minhashing.compare, the host loop of the MinHash library (pinned to tests/_minhash_model.py by tests/test_minhash_abi.py), called
pair by pair; the model itself where a test says so.  Integers are compared with array_equal; the doubles bit for bit wherever every
partial sum is an integer below 2^53 (counts below 2^20, at most 2049 entries), and within rel 1e-12 with counts up to 2^64 - 1."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import minhash_sets, minhashing  # noqa: E402
import _mhset_model as SM  # noqa: E402
import _minhash_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STAGE = 2048          # kStage of ntk_minhash_set.hip (tests/test_minhash_set_abi.py ties the two)
PAIR_THREADS = 256    # kPairThreads of ntk_minhash_set.hip (likewise): four walked sketches per block
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2048, STAGE - 1, STAGE, STAGE + 1)
NUMS = (0, 1, 10, 500, 10 ** 6)
ERR_BAD_ARG, ERR_CAPACITY = 2, 5
INTS, DOUBLES, VECTORS = ("n_shared", "n_union"), ("dot", "norm2_a", "norm2_b"), ("n_a", "n_b")
u64 = functools.partial(np.array, dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def host_block(rows, cols, num, max_hash, abundance=True):
    return SM.block(rows, cols, num, max_hash, abundance, compare=minhashing.compare)


def assert_block(got, want, what, exact=True):
    for name in INTS + VECTORS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)
    for name in DOUBLES:
        if exact:
            assert np.array_equal(got[name], want[name]), (what, name)
        else:
            np.testing.assert_allclose(got[name], want[name], rtol=1e-12, atol=0, err_msg=f"{what} {name}")


def filled(ctx, sketches, abundance=True, block_pairs=0):
    s = nt.MinHashSet(abundance, ctx, block_pairs)
    for i, (h, c) in enumerate(sketches):
        assert s.add((h, c if abundance else None)) == i
    return s


def draw(rng, pool, n, top=1 << 20):
    h = np.sort(rng.choice(pool, n, replace=False))
    return h, rng.integers(1, top, n, dtype=np.uint64)


# ---- 1. the block against the host compare -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def forty():
    """40 sketches from one pool of 5000 hashes (0 and 2^64 - 1 among them), so that many hashes are shared: every length of LENGTHS,
    identical pairs, a subset, a prefix, and two interleaved halves."""
    rng = np.random.default_rng(0x5E7)
    pool = np.unique(np.concatenate([rng.integers(0, 1 << 64, 5000, dtype=np.uint64), u64([0, M.ALL])]))
    sk = [draw(rng, pool, n) for n in LENGTHS]
    long = sk[LENGTHS.index(STAGE + 1)]
    sk.append((long[0].copy(), long[1].copy()))                                  # identical, counts too
    sk.append((sk[12][0].copy(), rng.integers(1, 1 << 20, 1000, dtype=np.uint64)))   # identical hashes, other counts
    keep = np.sort(rng.choice(long[0].size, 700, replace=False))
    sk.append((long[0][keep], long[1][keep]))                                    # a subset of the longest
    sk.append((sk[12][0][:300], sk[12][1][:300]))                                # a prefix
    sk += [(long[0][::2], long[1][::2]), (long[0][1::2], long[1][1::2])]         # interleaved and disjoint
    while len(sk) < 40:
        sk.append(draw(rng, pool, int(rng.integers(1, 1500))))
    return pool, sk


@pytest.mark.parametrize("abundance", [True, False])
@pytest.mark.parametrize("cut", ["all", "half", "thousandth", "zero"])
def test_block_matches_the_host_compare(ctx, abundance, cut):
    pool, sk = forty()
    assert len(sk) == 40 and sorted(h.size for h, _ in sk[:len(LENGTHS)]) == sorted(LENGTHS)
    max_hash = {"all": M.ALL, "half": int(pool[pool.size // 2]), "thousandth": int(pool[pool.size // 1000]), "zero": 0}[cut]
    with filled(ctx, sk, abundance) as s:
        assert len(s) == 40 and s.stats()["n_entries"] == sum(h.size for h, _ in sk) and s.stats()["abundance"] == int(abundance)
        for num in NUMS:
            got, want = s.compare(num=num, max_hash=max_hash), host_block(sk, sk, num, max_hash, abundance)
            assert_block(got, want, (abundance, cut, num))
            if cut == "all" and num == 0:
                assert want["n_shared"][16, 17] == STAGE + 1 and want["n_shared"][21, 22] == 0 and want["n_union"][21, 22] == STAGE + 1
                assert (want["n_shared"] > 100).sum() > 100, "the pool makes the sketches overlap"
            if not abundance:
                assert np.array_equal(got["dot"], got["n_shared"].astype(np.float64))
        assert s.stats()["n_launches"] == 2 * len(NUMS) and s.stats()["n_uploads"] == 1


# ---- 2. large counts ---------------------------------------------------------------------------------------------------------------

def test_large_counts_sum_in_double(ctx):
    rng = np.random.default_rng(0x5E8)
    pool = np.unique(rng.integers(0, 1 << 64, 3000, dtype=np.uint64))
    sk = [draw(rng, pool, n, top=1 << 64) for n in (1, 64, 65, 500, 1000, 2047, 2048, 2048, 1500, 130)]
    sk.append((sk[7][0].copy(), np.full(2048, M.ALL, dtype=np.uint64)))
    with filled(ctx, sk) as s:
        for num in (0, 700):
            got, want = s.compare(num=num), host_block(sk, sk, num, M.ALL)
            assert want["dot"].max() > 2.0 ** 130 and (want["n_shared"] > 50).sum() > 30
            assert_block(got, want, num, exact=False)


# ---- 3. the num-th member of the union ---------------------------------------------------------------------------------------------

def test_the_num_th_union_member(ctx):
    """A shared, an A-only and a B-only hash at union position num - 1 (the last one counted) and, with num one smaller, at position num
    (the first one not counted), on both sides of A's first round of 64; against the model."""
    base = np.arange(10, 10 + 2 * 70, 2, dtype=np.uint64)
    cases = []
    for at in (3, 63, 64, 66):
        for a, b in ((base, base[[at]]), (base, base[at + 1:]), (base[:at], base[at:]), (base, base)):
            position = int(np.searchsorted(np.union1d(a, b), base[at]))
            cases += [(a, b, num) for num in (position + 1, position) if num]
    rows = [(a, np.arange(1, a.size + 1, dtype=np.uint64)) for a, _, _ in cases]
    cols = [(b, np.arange(101, b.size + 101, dtype=np.uint64)) for _, b, _ in cases]
    with filled(ctx, rows) as ra, filled(ctx, cols) as cb:
        for i, (a, b, num) in enumerate(cases):
            got = ra.compare(rows=i, cols=i, other=cb, num=num)
            want = M.compare(*rows[i], *cols[i], num, M.ALL)
            assert want["n_union"] == num
            for name in INTS + DOUBLES:
                assert got[name].shape == (1, 1) and got[name][0, 0] == want[name], (i, name, num, got[name], want[name])
            assert got["n_a"][0] == a.size and got["n_b"][0] == b.size


# ---- 4. 0 and 2^64 - 1 are hashes like any other -----------------------------------------------------------------------------------

def test_hash_edge_values(ctx):
    rng = np.random.default_rng(0x5E9)
    inner = np.unique(rng.integers(1, M.ALL, 2200, dtype=np.uint64))   # neither edge value
    hashes = [u64([0]), u64([M.ALL]), u64([0, M.ALL]), u64([1]), u64([M.ALL - 1])]
    for n in (63, 64, 65, STAGE - 1, STAGE, STAGE + 1):
        body = np.sort(rng.choice(inner, n, replace=False))
        # n hashes ending in 2^64 - 1 / starting with 0 / both, and the same sketch without the edge value
        hashes += [np.concatenate([body[:-1], u64([M.ALL])]), body, np.concatenate([u64([0]), body[1:]]),
                   np.concatenate([u64([0]), body[1:-1], u64([M.ALL])]), body[:-1], body[1:]]
    sk = [(h, rng.integers(1, 1 << 20, h.size, dtype=np.uint64)) for h in hashes]
    assert all(np.all(h[1:] > h[:-1]) for h in hashes)
    with filled(ctx, sk) as s:
        for num, max_hash in ((0, M.ALL), (0, M.ALL - 1), (0, 0), (5, M.ALL), (64, M.ALL), (STAGE, M.ALL), (2 * STAGE, M.ALL - 1)):
            want = host_block(sk, sk, num, max_hash)
            assert_block(s.compare(num=num, max_hash=max_hash), want, (num, max_hash))
        # a sketch ending in 2^64 - 1 against the same sketch without it: one hash fewer is shared, nothing is taken for a match
        want = host_block(sk, sk, 0, M.ALL)
        for first in range(5, len(sk), 6):
            n = sk[first][0].size
            assert want["n_shared"][first, first + 4] == n - 1 and want["n_union"][first, first + 4] == n
            assert want["n_shared"][first + 2, first + 5] == n - 1
        assert want["n_shared"][0, 2] == want["n_shared"][1, 2] == 1 and want["n_shared"][0, 1] == 0


# ---- 5. sub-blocks -----------------------------------------------------------------------------------------------------------------

def test_sub_block_seams(ctx):
    """37 rows against 29 columns with a launch per pair, within a row, per row exactly, per row plus one pair, and per 64 pairs; each
    equals the one-launch result, and the launches are counted."""
    rng = np.random.default_rng(0x5EA)
    pool = np.unique(rng.integers(0, 1 << 64, 900, dtype=np.uint64))
    sk = [draw(rng, pool, int(n)) for n in rng.integers(0, 400, 37 + 29)]
    want = host_block(sk[:37], sk[37:], 150, M.ALL)
    for block_pairs in (1073, 1, 7, 29, 30, 64):
        with filled(ctx, sk, block_pairs=block_pairs) as s:
            assert s.stats()["block_pairs"] == block_pairs
            steps = -(-37 * 29 // block_pairs)
            got = s.compare(rows=(0, 37), cols=(37, 66), num=150)
            assert_block(got, want, block_pairs)
            assert s.stats()["n_launches"] == 2 * steps
            got = s.compare(rows=(0, 37), cols=(37, 66), num=150, want=("n_shared", "n_union", "dot", "norm2_a"))   # no second pass
            assert set(got) == {"n_shared", "n_union", "dot", "norm2_a", "n_a", "n_b"}
            for name in got:
                assert np.array_equal(got[name], want[name]), (block_pairs, name)
            assert s.stats()["n_launches"] == 3 * steps
            assert s.stats()["device_bytes"] >= 32 * min(block_pairs, 1073)


# ---- 6. ranges, two sets, the same set -----------------------------------------------------------------------------------------------

def test_ranges_two_sets_and_the_same_set(ctx):
    rng = np.random.default_rng(0x5EB)
    pool = np.unique(rng.integers(0, 1 << 64, 1200, dtype=np.uint64))
    sa = [draw(rng, pool, int(n)) for n in rng.integers(0, 600, 13)]
    sb = [draw(rng, pool, int(n)) for n in rng.integers(0, 600, 9)]
    with filled(ctx, sa) as a, filled(ctx, sb) as b, filled(ctx, sa[:1]) as one:
        for num in (0, 300):
            assert_block(a.compare(rows=(3, 11), cols=(5, 13), num=num), host_block(sa[3:11], sa[5:13], num, M.ALL), "one set, ranges")
            assert_block(a.compare(rows=range(2, 13), cols=slice(4, 7), other=b, num=num), host_block(sa[2:], sb[4:7], num, M.ALL), "two sets")
            assert_block(b.compare(other=a, num=num), host_block(sb, sa, num, M.ALL), "two sets, everything")
            assert_block(one.compare(num=num), host_block(sa[:1], sa[:1], num, M.ALL), "N = 1")
        whole = a.compare()
        n_a = np.array([h.size for h, _ in sa], dtype=np.uint64)
        assert np.array_equal(whole["n_a"], n_a) and np.array_equal(whole["n_b"], n_a)
        assert np.array_equal(np.diag(whole["n_shared"]), n_a) and np.array_equal(np.diag(whole["n_union"]), n_a)
        assert np.array_equal(np.diag(whole["dot"]), np.diag(whole["norm2_a"])) and np.array_equal(whole["norm2_a"], whole["norm2_b"].T)
        assert np.array_equal(whole["n_shared"], whole["n_shared"].T)
        before = a.stats()["n_launches"]
        for rows, cols in (((4, 4), None), (None, (2, 2)), ((0, 0), (0, 0))):
            got = a.compare(rows=rows, cols=cols)
            assert got["n_shared"].size == 0 and got["n_shared"].shape == (0 if rows else 13, 0 if cols else 13)
        assert a.stats()["n_launches"] == before
        # only the vectors: no pair is compared
        lib, out = minhash_sets.lib(), np.zeros(13, dtype=np.uint64)
        assert lib.ntk_mhset_compare(a._h, 0, 13, a._h, 0, 13, 0, int(pool[600]), None, None, None, None, None, out.ctypes.data, None) == 0
        assert np.array_equal(out, [int((h <= pool[600]).sum()) for h, _ in sa]) and a.stats()["n_launches"] == before


# ---- 7. add, read, growth, reset -----------------------------------------------------------------------------------------------------

def test_add_read_round_trip_and_growth(ctx):
    rng = np.random.default_rng(0x5EC)
    pool = np.unique(rng.integers(0, 1 << 64, 6000, dtype=np.uint64))
    sk = [draw(rng, pool, int(n)) for n in rng.choice([0, 1, 5, 64, 300, 1000, 3000], 300)]
    for abundance in (True, False):
        with nt.MinHashSet(abundance, ctx) as s:
            assert len(s) == 0 and s.stats()["n_uploads"] == 0
            grown = set()
            for i, (h, c) in enumerate(sk):
                assert s.add((h, c if abundance else None)) == i
                if i % 60 == 59:   # what was staged since the last compare goes up in one upload
                    assert s.stats()["n_uploads"] == i // 60
                    got = s.compare(rows=(i - 2, i + 1), cols=(0, 3), num=200)
                    assert_block(got, host_block(sk[i - 2:i + 1], sk[:3], 200, M.ALL, abundance), i)
                    assert s.stats()["n_uploads"] == i // 60 + 1
                    grown.add(s.stats()["device_bytes"])
            st = s.stats()
            assert st["n_sketches"] == 300 and st["n_entries"] == sum(h.size for h, _ in sk) > 100000
            assert st["n_uploads"] == 5 and len(grown) >= 3, "the arrays grew, by uploads far fewer than the adds"
            for i, (h, c) in enumerate(sk):
                got = s.sketch(i)
                assert np.array_equal(got[0], h) and np.array_equal(got[1], c if abundance else np.ones(h.size, dtype=np.uint64)), i
            assert s.stats()["n_uploads"] == 5
            n = C.c_uint64(0)   # the size query, and a capacity too small: nothing written
            few = np.zeros(2, dtype=np.uint64)
            assert minhash_sets.lib().ntk_mhset_read(s._h, 299, few.ctypes.data, few.ctypes.data, 2, C.byref(n)) == (ERR_CAPACITY if sk[299][0].size > 2 else 0)
            assert n.value == sk[299][0].size
            s.reset()
            assert len(s) == 0 and s.stats()["n_entries"] == 0
            assert s.add((sk[6][0], None)) == 0 and s.add((sk[7][0], None)) == 1
            plain = [(h, np.ones(h.size, dtype=np.uint64)) for h, _ in sk[6:8]]
            assert_block(s.compare(), host_block(plain, plain, 0, M.ALL), "after reset")
            assert np.array_equal(s.sketch(1)[0], sk[7][0])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------

def test_error_cases(ctx):
    good, other = u64([1, 5, 9]), u64([2, 5, 7, 11])
    lib = minhash_sets.lib()

    def refused(call):
        with pytest.raises(nt.NtkError) as e:
            call()
        assert e.value.status == ERR_BAD_ARG

    def unchanged(s, n):
        st = s.stats()
        assert st["n_sketches"] == n and st["n_entries"] == 3 * n
        for i in range(n):
            assert np.array_equal(s.sketch(i)[0], good)

    with nt.MinHashSet(True, ctx) as s, nt.MinHashSet(False, ctx) as flat:
        assert s.add((good, u64([3, 2, 1]))) == 0 and flat.add((good, None)) == 0
        for bad in (u64([1, 9, 5]), u64([1, 5, 5]), u64([9, 5, 1]), u64([0, 0])):
            refused(lambda: s.add((bad, None)))
            refused(lambda: flat.add((bad, None)))
        refused(lambda: flat.add((good, u64([1, 1, 1]))))                 # counts on a flat set
        refused(lambda: s.add((good, u64([1, 1]))))                       # a count array of the wrong size
        refused(lambda: s.add((good.astype(np.int64), None)))
        refused(lambda: s.add((None, None)))
        index = C.c_uint64(77)
        assert lib.ntk_mhset_add(s._h, None, None, 1 << 32, C.byref(index)) == ERR_BAD_ARG   # the length is checked before the arrays
        assert lib.ntk_mhset_add(s._h, None, None, (1 << 64) - 1, C.byref(index)) == ERR_BAD_ARG
        assert lib.ntk_mhset_add(s._h, None, None, 3, C.byref(index)) == ERR_BAD_ARG and index.value == 77
        assert lib.ntk_mhset_add(None, good.ctypes.data, None, 3, C.byref(index)) == ERR_BAD_ARG
        unchanged(s, 1)
        unchanged(flat, 1)
        assert s.add((good, None)) == 1
        for rows, cols in (((0, 3), None), (None, (1, 3)), ((2, 4), None), ((3, 3), None), (5, None)):
            refused(lambda: s.compare(rows=rows, cols=cols))
        refused(lambda: s.compare(cols=(0, 2), other=flat))
        refused(lambda: s.sketch(2))
        n = C.c_uint64(0)
        assert lib.ntk_mhset_read(s._h, 0, None, None, 3, C.byref(n)) == ERR_BAD_ARG
        assert lib.ntk_mhset_compare(s._h, 0, 1, None, 0, 1, 0, M.ALL, None, None, None, None, None, None, None) == ERR_BAD_ARG
        with nt.Context(0) as ctx2, nt.MinHashSet(True, ctx2) as far:
            far.add((other, None))
            refused(lambda: s.compare(other=far))
            refused(lambda: far.compare(other=s))
            assert far.compare()["n_shared"][0, 0] == 4
        handle = C.c_void_p()
        for abundance, block_pairs in ((2, 0), (0, minhash_sets.BLOCK_MAX + 1), (1, 1 << 63)):
            assert lib.ntk_mhset_create(ctx._h, abundance, block_pairs, C.byref(handle)) == ERR_BAD_ARG and not handle.value
        unchanged(s, 2)
        mixed = s.compare(other=flat)   # a set with counts against one without: those count 1
        assert mixed["n_shared"][0, 0] == 3 and mixed["dot"][0, 0] == 6.0 and mixed["norm2_b"][0, 0] == 3.0

    # the checks of KmerMinHash.compare, at add
    with nt.KmerMinHash(21, nt.PATH_BYTES_CANONICAL, num=100, ctx=ctx) as a, nt.KmerMinHash(19, nt.PATH_BYTES_CANONICAL, num=100, ctx=ctx) as k19, \
            nt.KmerMinHash(21, nt.PATH_BITS_CANONICAL, num=100, ctx=ctx) as bits, nt.KmerMinHash(21, nt.PATH_BYTES_CANONICAL, scaled=10, ctx=ctx) as sc, \
            nt.KmerMinHash(21, nt.PATH_BYTES_CANONICAL, num=50, ctx=ctx) as a50, nt.MinHashSet(True, ctx) as s:
        for mh in (a, a50):   # the refusals look at what a handle is, not at what it holds
            mh.add_records([b"ACGTTGCAAGGCTTAGCATCGATCGGATCTAGCTAGGATCCGATATCGCGATTAGC" * 3], nt.PRE_NORMALIZE)
        assert s.add(a) == 0 and (s.k, s.path, s.num, s.scaled, s.max_hash) == (21, nt.PATH_BYTES_CANONICAL, 100, 0, M.ALL)
        for mh in (k19, bits, sc):
            refused(lambda: s.add(mh))
            refused(lambda: s.search(mh))
        assert len(s) == 1 and s.add(a50) == 1 and s.num == 50


# ---- 9. real sketches ------------------------------------------------------------------------------------------------------------------

_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _samples():
    rng = np.random.default_rng(0x5ED)
    original = [r.raw_seq.replace(b"\n", b"").replace(b"\r", b"") for r in nt.parse_fastx_file(os.path.join(GOLDEN, "28S.fasta"))][:400]
    mutated = []
    for seq in original:
        arr = np.frombuffer(seq, dtype=np.uint8).copy()
        hit = rng.random(arr.size) < 0.01
        arr[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        mutated.append(arr.tobytes())
    revcomp = [seq.translate(_COMPLEMENT)[::-1] for seq in original]
    batches = [[np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3000)].tobytes() for _ in range(60)] for _ in range(2)]
    return [original, mutated, revcomp, batches[0], batches[1], []]


@pytest.mark.parametrize("kind", [dict(num=500), dict(scaled=7)], ids=["num500", "scaled7"])
def test_from_real_sketches(ctx, kind):
    samples = _samples()
    abundance = "scaled" in kind
    handles = [nt.KmerMinHash(21, nt.PATH_BYTES_CANONICAL, ctx=ctx, **kind) for _ in samples]
    try:
        for mh, records in zip(handles, samples):
            mh.add_records(records, nt.PRE_NORMALIZE)
        assert handles[0].stats()["n_kept"] >= 500 and handles[5].stats()["n_kept"] == 0
        with nt.MinHashSet(abundance, ctx) as s:
            for i, mh in enumerate(handles):
                assert s.add(mh) == i
            assert (s.k, s.num, s.scaled) == (21, kind.get("num", 0), kind.get("scaled", 0))
            for i, mh in enumerate(handles):
                h, c = mh.hashes()
                assert np.array_equal(s.sketch(i)[0], h) and (not abundance or np.array_equal(s.sketch(i)[1], c))
            pairwise = lambda method: np.array([[getattr(a, method)(b) for b in handles] for a in handles])
            jac = s.jaccard_matrix()
            assert np.array_equal(jac, pairwise("jaccard")) and np.array_equal(s.containment_matrix(), pairwise("containment"))
            assert np.array_equal(s.mash_distance_matrix(), pairwise("mash_distance")) and np.array_equal(s.mash_distance_matrix(21), s.mash_distance_matrix())
            if abundance:   # a flat set's counts are all 1; the handles' are not
                assert np.array_equal(s.cosine_matrix(), pairwise("cosine"))
            assert jac[0, 2] == jac[2, 0] == 1.0, "a sample and its reverse complement share every canonical k-mer"
            assert 0.2 < jac[0, 1] < 1.0 and jac[0, 3] < 0.01 and jac[5, 5] == 0.0 and np.array_equal(jac, jac.T)
            with nt.MinHashSet(abundance, ctx) as db:   # without the query itself and its reverse complement
                for mh in handles[1:2] + handles[3:]:
                    db.add(mh)
                hits = db.search(handles[0], top=3)
                assert len(hits) == 3 and hits[0] == (0, jac[0, 1]) and hits[0][1] > hits[1][1]
                contained = db.search(handles[0], top=10, containment=True)
                assert len(contained) == 4 and contained[0] == (0, s.containment_matrix()[0, 1])
    finally:
        for mh in handles:
            mh.close()


# ---- 10. the example -------------------------------------------------------------------------------------------------------------------

def test_minhash_matrix_example(ctx, tmp_path):
    exe = os.path.join(ROOT, "examples", "minhash_matrix")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    samples = _samples()[:3]
    files = []
    for i, records in enumerate(samples):
        files.append(str(tmp_path / f"s{i}.fasta"))
        with open(files[-1], "wb") as f:
            for j, seq in enumerate(records[:120]):
                f.write(b">r%d\n%s\n" % (j, seq))
    for args, kind in ((["-k", "21", "-n", "300"], dict(num=300)), (["-k", "21", "-s", "10"], dict(scaled=10))):
        handles = [nt.KmerMinHash(21, nt.PATH_BYTES_CANONICAL, ctx=ctx, **kind) for _ in samples]
        with nt.MinHashSet(False, ctx) as s:
            for mh, records in zip(handles, samples):
                mh.add_records(records[:120], nt.PRE_NORMALIZE)
                s.add(mh)
                mh.close()
            want = {"jaccard": s.jaccard_matrix(), "mash": s.mash_distance_matrix(), "containment": s.containment_matrix()}
        assert 0.0 < want["jaccard"][0, 1] < 1.0 and want["jaccard"][0, 2] == 1.0
        for measure, matrix in want.items():
            r = subprocess.run([exe, *args, "-m", measure, *files], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            got = [[float(x) for x in line.split("\t")] for line in r.stdout.splitlines()]
            assert got == [[float(f"{v:.6f}") for v in row] for row in matrix.tolist()], (measure, kind)
    assert subprocess.run([exe, "-k", "21", files[0]], capture_output=True, timeout=60).returncode == 2          # neither -n nor -s
    assert subprocess.run([exe, "-k", "21", "-n", "10", "-m", "x", files[0]], capture_output=True, timeout=60).returncode == 2
