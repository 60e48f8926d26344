"""Exact k-mer set algebra and joint spectra (include/needletail_amd_kmer_sets.h, needletail_amd.KmerSet) on a real MI355X.

Truth: tests/_kmer_sets_model.py, plain dicts (held to the rule header on the CPU by tests/test_kset_rule.py).  Everything is an integer
and is compared with array_equal.  test_many_tiles_per_block also compares with numpy directly (intersect1d / union1d / setdiff1d)."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import kmer_sets as KS  # noqa: E402
import _kmer_sets_model as KM  # noqa: E402
from _count_helpers import oracle_items, pack, random_records, upload  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TILE = {1: KM.TILE_WORDS, 2: KM.TILE_WORDS // 2}   # kTileOf<KW> of ntk_kmer_sets.hip (tests/test_kmer_sets_abi.py ties the two)
T = TILE[1]
M64 = KM.M64
BYTES = nt.PATH_BYTES_CANONICAL
ERR_BAD_ARG, ERR_CAPACITY = 2, 5
K_OF = {1: 21, 2: 41}   # the k a test set of each key width claims (the library never looks at it)
RULE_NAMES = {KM.MIN: "min", KM.MAX: "max", KM.SUM: "sum", KM.LEFT: "left", KM.RIGHT: "right"}
u64 = functools.partial(np.array, dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def _dev(v):
    v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1)
    if v.size == 0:
        return torch.empty(1, dtype=torch.int64, device="cuda")
    return torch.from_numpy(v.view(np.int64).copy()).cuda()


def make(ctx, keys, counts, kw=None):
    """A KmerSet straight from ascending host arrays (no sort, no validation: the tests decide what goes in)."""
    keys = np.asarray(keys, dtype=np.uint64)
    kw = kw or (2 if keys.ndim == 2 else 1)
    s = nt.KmerSet(_dev(keys), _dev(counts), len(counts), K_OF[kw], BYTES, ctx)
    torch.cuda.synchronize()
    return s


def ops_of(a, b, op, rule):
    if op == KM.INTERSECT:
        return a.intersect(b, RULE_NAMES[rule])
    if op == KM.UNION:
        return a.union(b, RULE_NAMES[rule])
    return a.subtract(b) if op == KM.SUBTRACT else a.counters_subtract(b)


def assert_list(got: "nt.KmerSet", want: dict, what):
    keys, counts = got.items()
    wk, wc = KM.as_list(want, got.key_words)
    assert len(got) == len(want) and keys.shape == wk.shape, (what, len(got), len(want))
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc), what
    assert got.violations() == 0, what


def check_pair(ctx, a_list, b_list, what, bins=(16, 5), ops=KM.OPS):
    """compare and every op of `ops` on the two lists against the model."""
    (ak, ac), (bk, bc) = a_list, b_list
    kw = 2 if np.asarray(ak).ndim == 2 else 1
    da, db = KM.as_dict(ak, ac), KM.as_dict(bk, bc)
    with make(ctx, ak, ac, kw) as a, make(ctx, bk, bc, kw) as b:
        hist, totals = a.compare(b, *bins)
        want_hist, want_totals = KM.compare(da, db, *bins)
        assert hist.dtype == np.uint64 and np.array_equal(hist.reshape(-1), want_hist), (what, "hist")
        assert totals == want_totals, (what, totals, want_totals)
        assert hist[0, 0] == 0
        for op, rule in ops:
            with ops_of(a, b, op, rule) as out:
                assert_list(out, KM.apply(op, rule, da, db), (what, op, rule))


def ramp(n, start=10, step=3):
    return np.arange(start, start + step * n, step, dtype=np.uint64)[:n]


def cnt(n, seed=0):
    return (np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(seed)) % np.uint64(9) + np.uint64(1)


def wide(v):
    """Narrow keys as {hi, lo} rows whose order is the values': a new hi every 50 values."""
    v = np.asarray(v, dtype=np.uint64)
    return np.stack([v // np.uint64(50), v * np.uint64(0x9E3779B1) % np.uint64(1 << 40) + (v % np.uint64(50) << np.uint64(40))], axis=1)


# ---- 1. lengths around the seams ---------------------------------------------------------------------------------------------------

def seam_lengths(t):
    return [(0, 0), (0, 1), (1, 0), (t - 1, 0), (t, 0), (t + 1, 0), (0, t - 1), (0, t), (0, t + 1), (t, t), (2 * t + 1, 3)]


@pytest.mark.parametrize("kw", (1, 2))
def test_lengths_around_the_tile_seams(ctx, kw):
    for n_a, n_b in seam_lengths(TILE[kw]):
        a, b = ramp(n_a, 10, 3), ramp(n_b, 13, 6)   # every second key of B is one of A's (while A lasts)
        if kw == 2:
            a, b = wide(a), wide(b)
        check_pair(ctx, (a, cnt(n_a, 1)), (b, cnt(n_b, 4)), (kw, n_a, n_b))


def test_many_tiles_per_block(ctx):
    """A few hundred thousand entries: more tiles than the launch has blocks, so a block strides over several tiles and flushes the bins
    it gathered over all of them.  Held to the model, and to numpy directly."""
    rng = np.random.default_rng(0xB16)
    pool = np.unique(rng.integers(0, 1 << 64, 400_000, dtype=np.uint64))
    a = np.sort(rng.choice(pool, 180_000, replace=False))
    b = np.sort(rng.choice(pool, 150_000, replace=False))
    ca, cb = rng.integers(1, 300, a.size, dtype=np.uint64), rng.integers(1, 12, b.size, dtype=np.uint64)
    assert (a.size + b.size) // T > 150
    check_pair(ctx, (a, ca), (b, cb), "big", bins=(256, 8), ops=((KM.UNION, KM.SUM), (KM.INTERSECT, KM.MIN), (KM.COUNTERS_SUBTRACT, 0)))
    with make(ctx, a, ca) as sa, make(ctx, b, cb) as sb:
        shared, ia, ib = np.intersect1d(a, b, assume_unique=True, return_indices=True)
        with sa.intersect(sb, "max") as out:
            keys, counts = out.items()
            assert np.array_equal(keys, shared) and np.array_equal(counts, np.maximum(ca[ia], cb[ib]))
        with sa.union(sb, "left") as out:
            keys, counts = out.items()
            assert np.array_equal(keys, np.union1d(a, b))
            assert np.array_equal(counts[np.searchsorted(keys, a)], ca)
        with sa.subtract(sb) as out:
            assert np.array_equal(out.items()[0], np.setdiff1d(a, b, assume_unique=True))
        hist, totals = sa.compare(sb, 128, 128)
        want = np.zeros((128, 128), dtype=np.uint64)
        in_b = np.zeros(a.size, dtype=bool)
        in_b[ia] = True
        full_b = np.zeros(a.size, dtype=np.uint64)
        full_b[ia] = cb[ib]
        np.add.at(want, (np.minimum(ca, 127).astype(np.int64), np.minimum(full_b, 127).astype(np.int64)), 1)
        only_b = np.ones(b.size, dtype=bool)
        only_b[ib] = False
        np.add.at(want, (np.zeros(int(only_b.sum()), dtype=np.int64), np.minimum(cb[only_b], 127).astype(np.int64)), 1)
        assert np.array_equal(hist, want)
        assert totals["n_shared"] == shared.size and totals["sum_a"] == int(ca.sum()) and totals["sum_b_only"] == int(cb[only_b].sum())


# ---- 2. where the seams fall -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", (1, 2))
def test_a_shared_key_across_each_of_the_first_three_seams(ctx, kw):
    """The shared key's A element is the last of tile s - 1 and its B twin the first of tile s (merged positions sT - 1 and sT), for
    s = 1, 2, 3, and one position to either side; then with the lists swapped, where B's unshared element ends the tile."""
    shape = wide if kw == 2 else (lambda v: v)
    for seam in (1, 2, 3):
        for before in (seam * TILE[kw] - 2, seam * TILE[kw] - 1, seam * TILE[kw]):
            # A: `before` small keys, then the shared key; B: the shared key, then larger keys
            top = np.uint64(10 * T)
            a = np.concatenate([np.arange(before, dtype=np.uint64), u64([top])])
            b = np.concatenate([u64([top]), top + np.uint64(5) + np.arange(40, dtype=np.uint64)])
            la, lb = (shape(a), cnt(a.size, 2)), (shape(b), cnt(b.size, 5))
            some = ((KM.UNION, KM.SUM), (KM.INTERSECT, KM.RIGHT), (KM.SUBTRACT, 0), (KM.COUNTERS_SUBTRACT, 0))
            check_pair(ctx, la, lb, (kw, seam, before, "A last"), ops=some)
            check_pair(ctx, lb, la, (kw, seam, before, "swapped"), ops=some)


def test_all_shared_none_shared_and_interleaved(ctx):
    n = 2 * T + 77
    base = ramp(n, 5, 4)
    for what, a, b in (("all shared", base, base), ("none shared", base, base + np.uint64(1)), ("interleaved", base[::2], base[1::2]),
                       ("B below A", base + np.uint64(10 ** 9), base), ("A below B", base, base + np.uint64(10 ** 9))):
        check_pair(ctx, (a, cnt(a.size, 3)), (b, cnt(b.size, 6)), what)
    check_pair(ctx, (wide(base), cnt(n, 3)), (wide(base[::3]), cnt(base[::3].size, 6)), "wide, a third shared")


# ---- 3. key edges ------------------------------------------------------------------------------------------------------------------

def test_key_edges_narrow(ctx):
    mid = ramp(T + 5, 1000, 7)
    zero, top = u64([0]), u64([M64])
    for what, a, b in (("0 in A", np.concatenate([zero, mid]), mid), ("0 in B", mid, np.concatenate([zero, mid])),
                       ("0 in both", np.concatenate([zero, mid]), np.concatenate([zero, mid[::2]])),
                       ("top in A", np.concatenate([mid, top]), mid[::2]), ("top in B", mid[::2], np.concatenate([mid, top])),
                       ("top in both", np.concatenate([mid, top]), np.concatenate([zero, mid[1::2], top])),
                       ("only the edges", np.concatenate([zero, top]), np.concatenate([zero, top])),
                       ("edges apart", zero, top)):
        check_pair(ctx, (a, cnt(a.size, 1)), (b, cnt(b.size, 2)), what)


def test_key_edges_wide(ctx):
    """Wide keys that differ only in lo (equal hi) and only in hi (equal lo), and the edge values of both words."""
    rows = u64([[0, 0], [0, 1], [0, M64], [1, 0], [1, 1], [1, M64], [7, 5], [8, 5], [9, 5], [1 << 63, 0], [M64, 0], [M64, M64 - 1], [M64, M64]])
    rng = np.random.default_rng(0xED6E)
    for _ in range(12):
        pa, pb = np.sort(rng.choice(len(rows), rng.integers(0, len(rows) + 1), replace=False)), \
            np.sort(rng.choice(len(rows), rng.integers(0, len(rows) + 1), replace=False))
        check_pair(ctx, (rows[pa].reshape(-1, 2), cnt(pa.size, 1)), (rows[pb].reshape(-1, 2), cnt(pb.size, 3)), (pa, pb))
    # runs of one hi longer than a tile, and runs of one lo
    n = T + 300
    same_hi = np.stack([np.full(n, 3, dtype=np.uint64), ramp(n, 0, 2)], 1)
    same_lo = np.stack([ramp(n, 0, 2), np.full(n, 9, dtype=np.uint64)], 1)
    check_pair(ctx, (same_hi, cnt(n, 1) * np.uint64(20)), (same_hi[::2], cnt(same_hi[::2].shape[0], 2) * np.uint64(20)), "equal hi", bins=(128, 128))
    check_pair(ctx, (same_lo, cnt(n, 1)), (same_lo[1::3], cnt(same_lo[1::3].shape[0], 2)), "equal lo")
    order = np.lexsort((np.concatenate([same_hi, same_lo])[:, 1], np.concatenate([same_hi, same_lo])[:, 0]))
    mixed = np.unique(np.concatenate([same_hi, same_lo])[order], axis=0)
    check_pair(ctx, (mixed, cnt(mixed.shape[0], 4)), (same_lo, cnt(n, 5)), "mixed")


# ---- 4. counts ---------------------------------------------------------------------------------------------------------------------

def test_sum_saturates_and_counters_subtract_at_the_edge(ctx):
    keys = ramp(8)
    ca = u64([M64, M64 - 1, 1 << 63, 5, 5, 6, 1, M64])
    cb = u64([1, 1, 1 << 63, 5, 4, 7, M64, M64])
    with make(ctx, keys, ca) as a, make(ctx, keys, cb) as b:
        with a.union(b, "sum") as out:
            assert out.items()[1].tolist() == [M64, M64, M64, 10, 9, 13, M64, M64]
        with a.intersect(b, "sum") as out:
            assert out.items()[1].tolist() == [M64, M64, M64, 10, 9, 13, M64, M64]
        with a.counters_subtract(b) as out:   # a == b is dropped, a == b + 1 stays with 1
            k, c = out.items()
            assert k.tolist() == keys[[0, 1, 4]].tolist() and c.tolist() == [M64 - 1, M64 - 2, 1]
    check_pair(ctx, (keys, ca), (keys[2:], cb[2:]), "big counts", bins=(2, 2))


@pytest.mark.parametrize("bins", ((2, 2), (128, 128), (5, 3), (16384 // 2, 2)))
def test_counts_at_below_and_above_the_last_bin(ctx, bins):
    ba, bb = bins
    edge_a, edge_b = [ba - 2, ba - 1, ba, ba + 100], [bb - 2, bb - 1, bb, bb + 100]
    pairs = [(x, y) for x in edge_a for y in edge_b if x > 0 and y > 0] + [(x, 0) for x in edge_a if x > 0] + [(0, y) for y in edge_b if y > 0]
    keys = ramp(len(pairs))
    in_a, in_b = u64([p[0] for p in pairs]) > 0, u64([p[1] for p in pairs]) > 0
    a = (keys[in_a], u64([p[0] for p in pairs])[in_a])
    b = (keys[in_b], u64([p[1] for p in pairs])[in_b])
    check_pair(ctx, a, b, bins, bins=bins, ops=())


def test_a_total_that_wraps(ctx):
    keys = ramp(5)
    ca, cb = u64([M64, M64, 3, M64 - 7, 2]), u64([M64, 9, M64, M64 - 7, M64])
    with make(ctx, keys, ca) as a, make(ctx, keys[1:], cb[1:]) as b:
        _, t = a.compare(b, 2, 2)
        assert t == KM.compare(KM.as_dict(keys, ca), KM.as_dict(keys[1:], cb[1:]), 2, 2)[1]
        assert t["sum_a"] == int(sum(int(c) for c in ca)) % (1 << 64) and int(sum(int(c) for c in ca)) >= 1 << 64
        assert t["sum_max"] == (sum(max(int(x), int(y)) for x, y in zip(ca[1:], cb[1:])) + M64) % (1 << 64)


# ---- 5. every op x rule on random lists --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", (1, 2))
def test_every_op_and_rule_on_random_lists(ctx, kw):
    rng = np.random.default_rng(0x0B5 + kw)
    for n_a, n_b, n_pool in ((3000, 2500, 4000), (5, 4100, 4200), (4500, 1, 5000), (2049, 2047, 2100)):
        if kw == 1:
            pool = np.unique(np.concatenate([rng.integers(0, 1 << 64, n_pool, dtype=np.uint64), u64([0, M64])]))
        else:
            pool = np.unique(np.stack([rng.integers(0, 5, n_pool, dtype=np.uint64), rng.integers(0, 1 << 64, n_pool, dtype=np.uint64)], 1), axis=0)
        ia, ib = np.sort(rng.choice(len(pool), n_a, replace=False)), np.sort(rng.choice(len(pool), n_b, replace=False))
        check_pair(ctx, (pool[ia], rng.integers(1, 40, n_a, dtype=np.uint64)), (pool[ib], rng.integers(1, 40, n_b, dtype=np.uint64)), (kw, n_a, n_b),
                   bins=(32, 32))


# ---- 6. the C calls: capacity, arguments, validate ---------------------------------------------------------------------------------

def _raw_apply(h, op, rule, a, b, out_keys, out_counts, cap):
    n = C.c_uint64(123)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = KS.lib().ntk_kmer_sets_apply_device(h._native(), op, rule, *a._list(), *b._list(), ptr(out_keys), ptr(out_counts), cap, C.byref(n))
    torch.cuda.synchronize()
    return rc, n.value


@pytest.mark.parametrize("kw", (1, 2))
def test_capacity_query_exact_fit_and_one_short(ctx, kw):
    a_keys, b_keys = ramp(3 * T, 10, 2), ramp(2 * T, 11, 3)
    if kw == 2:
        a_keys, b_keys = wide(a_keys), wide(b_keys)
    da, db = KM.as_dict(a_keys, cnt(3 * T, 1)), KM.as_dict(b_keys, cnt(2 * T, 2))
    with make(ctx, a_keys, cnt(3 * T, 1), kw) as a, make(ctx, b_keys, cnt(2 * T, 2), kw) as b:
        for op, rule in ((KM.UNION, KM.SUM), (KM.INTERSECT, KM.MIN), (KM.SUBTRACT, 0), (KM.COUNTERS_SUBTRACT, 0)):
            want_k, want_c = KM.as_list(KM.apply(op, rule, da, db), kw)
            need = want_c.size
            assert need >= T
            assert _raw_apply(a, op, rule, a, b, None, None, 0) == (ERR_CAPACITY, need)
            sentinel = -0x0123456789ABCDEF
            keys = torch.full((kw * need + 8,), sentinel, dtype=torch.int64, device="cuda")
            counts = torch.full((need + 8,), sentinel, dtype=torch.int64, device="cuda")
            assert _raw_apply(a, op, rule, a, b, keys, counts, need - 1) == (ERR_CAPACITY, need)
            assert bool((keys == sentinel).all()) and bool((counts == sentinel).all()), "cap one short writes nothing"
            assert _raw_apply(a, op, rule, a, b, keys, counts, need) == (0, need)
            assert np.array_equal(keys[: kw * need].cpu().numpy().view(np.uint64), want_k.reshape(-1))
            assert np.array_equal(counts[:need].cpu().numpy().view(np.uint64), want_c)
            assert bool((keys[kw * need:] == sentinel).all()) and bool((counts[need:] == sentinel).all()), "nothing past the result"


def _union_sum(a, ca, b, cb):
    keys = np.union1d(a, b)
    counts = np.zeros(keys.size, dtype=np.uint64)
    counts[np.searchsorted(keys, a)] += ca
    counts[np.searchsorted(keys, b)] += cb
    return keys, counts


def test_scratch_regrows_on_one_handle_and_after_release(ctx):
    """One handle joins lists of 100 keys, then lists of more than 1024 tiles (the tile arrays' first size), then - its scratch released -
    lists of 100 again.  Every union is numpy's (the small ones the model's too), and the scratch a grown handle holds is what a fresh one
    allocates for the same call."""
    n_big = 1024 * T // 2 + 1
    assert (2 * n_big + T - 1) // T == 1025
    rng = np.random.default_rng(0xB17)
    lists = []
    for n in (100, n_big):
        pool = np.unique(rng.integers(0, 1 << 63, 3 * n, dtype=np.uint64))
        a, b = np.sort(rng.choice(pool, n, replace=False)), np.sort(rng.choice(pool, n, replace=False))
        lists.append((a, rng.integers(1, 300, n, dtype=np.uint64), b, rng.integers(1, 12, n, dtype=np.uint64)))
    keys = torch.empty(2 * n_big, dtype=torch.int64, device="cuda")
    counts = torch.empty(2 * n_big, dtype=torch.int64, device="cuda")

    def union_on(h, a, ca, b, cb, what):
        want_k, want_c = _union_sum(a, ca, b, cb)
        with make(ctx, a, ca) as sa, make(ctx, b, cb) as sb:
            assert _raw_apply(h, KM.UNION, KM.SUM, sa, sb, keys, counts, 2 * a.size) == (0, want_k.size), what
        assert np.array_equal(keys[: want_k.size].cpu().numpy().view(np.uint64), want_k), what
        assert np.array_equal(counts[: want_k.size].cpu().numpy().view(np.uint64), want_c), what
        return h.stats()["device_bytes"]

    small, big = lists
    model_k, model_c = KM.as_list(KM.apply(KM.UNION, KM.SUM, KM.as_dict(small[0], small[1]), KM.as_dict(small[2], small[3])), 1)
    numpy_k, numpy_c = _union_sum(*small)
    assert np.array_equal(model_k, numpy_k) and np.array_equal(model_c, numpy_c) and 100 < numpy_k.size < 200
    with make(ctx, small[0], small[1]) as h, make(ctx, small[0], small[1]) as fresh:
        bytes_small = union_on(h, *small, "100")
        bytes_big = union_on(h, *big, "big")
        assert bytes_big > bytes_small
        assert union_on(fresh, *big, "big, fresh") == bytes_big
        h.release()
        assert h.stats()["device_bytes"] < bytes_small
        assert union_on(h, *small, "100 after release") == bytes_small


def test_argument_checks(ctx):
    lib = KS.lib()
    keys, counts = ramp(100), cnt(100)
    with make(ctx, keys, counts) as a, make(ctx, keys[::2], counts[::2]) as b:
        out_k, out_c = torch.zeros(256, dtype=torch.int64, device="cuda"), torch.zeros(256, dtype=torch.int64, device="cuda")
        # unknown op / rule, a rule with a subtract op, no rule with union
        for op, rule in ((0, 0), (5, 0), (KM.UNION, 0), (KM.UNION, 6), (KM.INTERSECT, 0), (KM.SUBTRACT, KM.MIN), (KM.COUNTERS_SUBTRACT, KM.SUM)):
            assert _raw_apply(a, op, rule, a, b, out_k, out_c, 256)[0] == ERR_BAD_ARG, (op, rule)
        # an output range that overlaps an input range, or the other output
        assert _raw_apply(a, KM.UNION, KM.SUM, a, b, a.keys, out_c, 100)[0] == ERR_BAD_ARG
        assert _raw_apply(a, KM.UNION, KM.SUM, a, b, out_k, b.counts, 50)[0] == ERR_BAD_ARG
        assert _raw_apply(a, KM.UNION, KM.SUM, a, b, out_k, out_k[100:], 150)[0] == ERR_BAD_ARG
        assert _raw_apply(a, KM.UNION, KM.SUM, a, b, a.keys[99:], out_c, 10)[0] == ERR_BAD_ARG   # the last input word
        # NULL outputs with a capacity, NULL lists with a length
        assert _raw_apply(a, KM.UNION, KM.SUM, a, b, None, out_c, 256)[0] == ERR_BAD_ARG
        n = C.c_uint64(0)
        null = C.c_void_p(None)
        assert lib.ntk_kmer_sets_apply_device(a._native(), KM.UNION, KM.SUM, null, C.c_void_p(a.counts.data_ptr()), 100, *b._list(),
                                              C.c_void_p(out_k.data_ptr()), C.c_void_p(out_c.data_ptr()), 256, C.byref(n)) == ERR_BAD_ARG
        assert lib.ntk_kmer_sets_apply_device(a._native(), KM.UNION, KM.SUM, *a._list(), *b._list(), C.c_void_p(out_k.data_ptr()),
                                              C.c_void_p(out_c.data_ptr()), 256, None) == ERR_BAD_ARG
        # misaligned
        assert lib.ntk_kmer_sets_apply_device(a._native(), KM.UNION, KM.SUM, C.c_void_p(a.keys.data_ptr() + 4), C.c_void_p(a.counts.data_ptr()), 50,
                                              *b._list(), C.c_void_p(out_k.data_ptr()), C.c_void_p(out_c.data_ptr()), 256, C.byref(n)) == ERR_BAD_ARG
        # compare: bins
        t = KS.Totals()
        for ba, bb in ((1, 8), (8, 1), (0, 0), (129, 128), (16385, 1), (8193, 2)):
            assert lib.ntk_kmer_sets_compare_device(a._native(), *a._list(), *b._list(), ba, bb, None, C.byref(t)) == ERR_BAD_ARG, (ba, bb)
        assert lib.ntk_kmer_sets_compare_device(a._native(), *a._list(), *b._list(), 8192, 2, None, None) == 0
        assert lib.ntk_kmer_sets_compare_device(a._native(), null, null, 5, *b._list(), 4, 4, None, C.byref(t)) == ERR_BAD_ARG
        # empty lists are ordinary: NULL arrays with n = 0
        assert lib.ntk_kmer_sets_compare_device(a._native(), null, null, 0, null, null, 0, 4, 4, None, C.byref(t)) == 0 and t.n_a == t.sum_max == 0
        assert lib.ntk_kmer_sets_apply_device(a._native(), KM.UNION, KM.SUM, null, null, 0, null, null, 0, null, null, 0, C.byref(n)) == 0 and n.value == 0
        # key_words
        h = C.c_void_p()
        for kw in (0, 3):
            assert lib.ntk_kmer_sets_create(ctx._h, kw, C.byref(h)) == ERR_BAD_ARG and not h.value
        # the Python face refuses sets of a different k
        with nt.KmerSet(a.keys, a.counts, a.n, 22, BYTES, ctx) as other, pytest.raises(nt.NtkError) as e:
            a.union(other)
        assert e.value.status == ERR_BAD_ARG
        with nt.KmerSet(a.keys, a.counts, a.n, 21, nt.PATH_BITS, ctx) as other, pytest.raises(nt.NtkError):
            a.compare(other)
        st = a.stats()
        assert st["key_words"] == 1 and st["n_launches"] > 0 and st["device_bytes"] > 0
        a.release()
        assert a.stats()["device_bytes"] < st["device_bytes"]
        with a.union(b) as again:   # the scratch comes back
            assert len(again) == 100


@pytest.mark.parametrize("kw", (1, 2))
def test_validate_counts_a_swapped_pair_and_a_duplicate(ctx, kw):
    keys = ramp(3 * T + 10)
    keys[[T - 1, T]] = keys[[T, T - 1]]     # one swapped pair, across a block boundary of 256 and the tile length: 1 violation
    keys[2 * T + 5] = keys[2 * T + 4]       # one duplicate: 1 violation
    shaped = wide(keys) if kw == 2 else keys
    with make(ctx, shaped, cnt(keys.size), kw) as s:
        assert s.violations() == 2
    ok = ramp(3 * T + 10)
    with make(ctx, wide(ok) if kw == 2 else ok, cnt(ok.size), kw) as s:
        assert s.violations() == 0
    for n in (0, 1):
        with make(ctx, (wide(ok) if kw == 2 else ok)[:n], cnt(n), kw) as s:
            assert s.violations() == 0
    if kw == 2:   # equal hi with descending lo, equal lo with descending hi
        with make(ctx, u64([[1, 5], [1, 4], [2, 4], [1, 4]]), cnt(4), 2) as s:
            assert s.violations() == 2
    with pytest.raises(nt.NtkError) as e:
        nt.KmerSet.from_arrays(u64([5, 3, 5]) if kw == 1 else u64([[1, 5], [0, 3], [1, 5]]), cnt(3), K_OF[kw], ctx=ctx)
    assert e.value.status == ERR_BAD_ARG
    with nt.KmerSet.from_arrays(u64([5, 3, 9]) if kw == 1 else u64([[1, 5], [0, 3], [1, 4]]), u64([1, 2, 3]), K_OF[kw], ctx=ctx) as s:
        k, c = s.items()
        assert (k.tolist(), c.tolist()) == (([3, 5, 9], [2, 1, 3]) if kw == 1 else ([[0, 3], [1, 4], [1, 5]], [2, 3, 1]))


# ---- 7. end to end: two count tables -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def two_buffers():
    """Two record sets that share half their records."""
    recs = random_records(0x5E75, 240)
    return pack(recs[:160]), pack(recs[80:])


def _wide_oracle_items(buf, k):
    from test_gpu_wide_count import oracle_items as wide_items
    return wide_items(buf, k)


@pytest.mark.parametrize("k", (21, 41))
def test_two_tables_end_to_end(ctx, k):
    bufs = two_buffers()
    table = nt.KmerTable if k <= 32 else nt.WideKmerTable
    want = [oracle_items(b, k, BYTES, nt.PRE_NORMALIZE) if k <= 32 else _wide_oracle_items(b, k) for b in bufs]
    da, db = (KM.as_dict(keys, counts.astype(np.uint64)) for keys, counts in want)
    assert len(da) > 5000 and len(set(da) & set(db)) > 1000 and len(set(da) - set(db)) > 1000
    tables, devs = [], [upload(buf) for buf in bufs]
    for buf, dev in zip(bufs, devs):
        t = table(k, BYTES, len(buf), ctx)
        t.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        ctx.synchronize()
        tables.append(t)
    with nt.KmerSet.from_table(tables[0]) as a, nt.KmerSet.from_table(tables[1]) as b:
        assert (a.k, a.path, a.key_words) == (k, BYTES, 1 if k <= 32 else 2)
        assert_list(a, da, "A")
        assert_list(b, db, "B")
        hist, totals = a.compare(b)
        want_hist, want_totals = KM.compare(da, db, 256, 8)
        assert hist.shape == (256, 8) and np.array_equal(hist.reshape(-1), want_hist) and totals == want_totals
        for op, rule in KM.OPS:
            with ops_of(a, b, op, rule) as out:
                assert_list(out, KM.apply(op, rule, da, db), (k, op, rule))
        # the numbers read from the totals
        t = want_totals
        assert a.jaccard(b) == t["n_shared"] / (t["n_a"] + t["n_b"] - t["n_shared"])
        assert a.containment(b) == t["n_shared"] / t["n_a"]
        assert a.weighted_jaccard(b) == t["sum_min"] / t["sum_max"]
        assert a.bray_curtis(b) == 1.0 - 2.0 * t["sum_min"] / (t["sum_a"] + t["sum_b"])
        assert KS.merqury_qv(a, b) == KM.qv(t["sum_b_only"], t["sum_b"], k) and math.isfinite(KS.merqury_qv(a, b))
        assert KS.merqury_qv(a, a) == math.inf
        # composition
        with a.intersect(a, "left") as same:
            assert_list(same, da, "intersect(A, A, LEFT)")
        with a.subtract(a) as none:
            assert len(none) == 0 and none.items()[0].shape == ((0,) if k <= 32 else (0, 2))
        both = table(k, BYTES, len(bufs[0]) + len(bufs[1]), ctx)
        for buf, dev in zip(bufs, devs):
            both.count_device(dev, len(buf), nt.PRE_NORMALIZE)
        ctx.synchronize()
        with a.union(b, "sum") as u:
            keys, counts = u.items()
            tk, tc = both.items()
            assert np.array_equal(keys, tk) and np.array_equal(counts, tc), "union(A, B, SUM) is the table that counted both"
        both.close()
    # min_count = 2: the solid k-mers
    solid = {key: c for key, c in da.items() if c >= 2}
    with nt.KmerSet.from_table(tables[0], min_count=2) as a2, nt.KmerSet.from_table(tables[1]) as b:
        assert_list(a2, solid, "min_count=2")
        t2 = KM.compare(solid, db, 2, 2)[1]
        assert KS.completeness(a2, b) == t2["n_shared"] / t2["n_a"]
        with a2.counters_subtract(b) as out:
            assert_list(out, KM.apply(KM.COUNTERS_SUBTRACT, 0, solid, db), "solid csub")
    for t in tables:
        t.close()


# ---- 8. the example --------------------------------------------------------------------------------------------------------------

def _records(name):
    return [r.raw_seq for r in nt.parse_fastx_file(os.path.join(GOLDEN, name))]


def _decode(kmer: str, k: int):
    v = 0
    for ch in kmer:
        v = (v << 2) | "ACGT".index(ch)
    return v


@pytest.mark.parametrize("k,other,op_arg", ((21, "28S.fasta", "intersect:max"), (21, "PRJNA271013_head.fq", "union"),
                                              (41, "PRJNA271013_head.fq", "counters_subtract")))
def test_compare_tables_example(ctx, k, other, op_arg):
    """examples/compare_tables on 28S.fasta against itself and against the FASTQ head: the spectrum, the summary and one list, each
    against the Python route on the same records."""
    exe = os.path.join(ROOT, "examples", "compare_tables")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    fa, other = os.path.join(GOLDEN, "28S.fasta"), os.path.join(GOLDEN, other)
    table = nt.KmerTable if k <= 32 else nt.WideKmerTable
    sets = []
    for path in (fa, other):
        recs = _records(os.path.basename(path))
        with table(k, BYTES, sum(len(r) for r in recs) + 1, ctx) as t:
            t.count_records(recs, nt.PRE_NORMALIZE)
            sets.append(nt.KmerSet.from_table(t))
    a, b = sets
    hist, totals = a.compare(b, 64, 4)
    r = subprocess.run([exe, "-k", str(k), "-a", "64", "-b", "4", fa, other], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got_hist, summary = np.zeros((64, 4), dtype=np.uint64), {}
    for line in r.stdout.splitlines():
        if line.startswith("# "):
            name, value = line[2:].split("\t")
            summary[name] = value
        else:
            x, y, n = map(int, line.split("\t"))
            got_hist[x, y] = n
    assert np.array_equal(got_hist, hist)
    assert {name: int(summary[name]) for name in KM.TOTALS} == totals
    assert float(summary["jaccard"]) == a.jaccard(b) and float(summary["weighted_jaccard"]) == a.weighted_jaccard(b)
    assert float(summary["bray_curtis"]) == a.bray_curtis(b) and float(summary["completeness"]) == KS.completeness(a, b)
    assert float(summary["containment"]) == a.containment(b)
    assert float(summary["qv"]) == pytest.approx(KS.merqury_qv(a, b), rel=1e-12)   # pow and log10 of two maths libraries
    if other == fa:
        assert totals["n_shared"] == totals["n_a"] == totals["n_b"] > 0 and summary["qv"] == "inf" and float(summary["jaccard"]) == 1.0
    else:
        assert 0 < totals["n_shared"] < totals["n_a"] or totals["n_shared"] == 0
    out = {"intersect:max": lambda: a.intersect(b, "max"), "union": lambda: a.union(b, "sum"),
           "counters_subtract": lambda: a.counters_subtract(b)}[op_arg]()
    r = subprocess.run([exe, "-k", str(k), "-o", op_arg, fa, other], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [line.split("\t") for line in r.stdout.splitlines()]
    keys, counts = out.items()
    want_keys = [int(v) for v in keys] if k <= 32 else [(int(hi) << 64) | int(lo) for hi, lo in keys]
    assert len(lines) == len(out) > 0
    assert [_decode(kmer, k) for kmer, _ in lines] == want_keys and [int(c) for _, c in lines] == counts.tolist()
    for s in (out, a, b):
        s.close()
    for bad in (["-o", "subtract:min"], ["-a", "-1"], ["-a", "8193", "-b", "2"], ["-b", "1"]):   # refused before any device work
        r = subprocess.run([exe, *bad, fa, fa], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr, bad
