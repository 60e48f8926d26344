"""Every capped-grid kernel of the k-mer libraries past one step of its grid-stride loop (tests/_grid_steps.py is the inventory).

Each test reads the device's CU count, sizes its input to about 1.25 x items_per_step of its kernel - one whole step and a second, partly
filled one - and asserts that before it runs.  The references are the libraries' host models (and numpy set algebra for the k-mer lists,
tests/_dbg_model.ArrayGraph for the graph); every comparison is array_equal on whole outputs.  Inputs are built vectorised; what is done
per record in Python stays in the tens of thousands of records."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import needletail_amd as nt  # noqa: E402
import _abundance_model as A  # noqa: E402
import _colors_model as KM  # noqa: E402
import _count_model as CM  # noqa: E402
import _dbg_model as DM  # noqa: E402
import _grid_steps as G  # noqa: E402
import _minhash_model as M  # noqa: E402
import _record_minhash_model as R  # noqa: E402
import _trim_model as T  # noqa: E402
import _wide_count_model as WM  # noqa: E402
from _count_helpers import oracle_items  # noqa: E402
from _lib_fuzz import hold_graph, random_masks  # noqa: E402

pytestmark = pytest.mark.gpu

BYTES, BITS = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NL = ord("\n")
K = 21
U = np.uint64


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def step_of(kernel, cu, lib=None) -> int:
    return G.items_per_step(G.rows_of(kernel, lib), cu)


def past_one_step(kernel, items, cu, lib=None, whole=1):
    """The precondition: `items` fill `whole` steps of the kernel's grid and a part of the next."""
    step = step_of(kernel, cu, lib)
    assert whole * step < items < (whole + 1) * step, \
        f"{kernel}: {items} items at {step} per step on {cu} CUs are {items / step:.3f} steps, not between {whole} and {whole + 1}"
    print(f"{kernel}: {items} items at {step} per step on {cu} CUs: {items / step:.3f} steps")
    return step


def dev_u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    t = torch.from_numpy(a.view(np.int64).copy()).cuda() if a.size else torch.empty(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def upload(a: np.ndarray):
    """A batch on the device, padded with break bytes to a multiple of 16 and 64 more."""
    t = torch.full(((a.size + 15) // 16 * 16 + 64,), NL, dtype=torch.uint8, device="cuda")
    t[:a.size] = torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64) if t.dtype == torch.int64 else t.cpu().numpy()


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError((what, f"{bad.size} rows differ, first {int(bad[0])}", got[bad[0]].tolist(), want[bad[0]].tolist()))


# ---- batches, vectorised -----------------------------------------------------------------------------------------------------------------

def sampled_batch(rng, genome, lengths, sub_rate=0.01, n_rate=0.05, periodic=False):
    """(bytes, offsets) of reads of the given lengths cut from `genome` at random places (around its end when `periodic`): substitutions
    at `sub_rate`, one N in a share `n_rate` of the reads, one break byte after each."""
    lengths = np.asarray(lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lengths + 1)])
    rec = np.repeat(np.arange(lengths.size), lengths + 1)
    within = np.arange(off[-1]) - off[:-1][rec]
    starts = rng.integers(0, np.full(lengths.size, genome.size) if periodic else np.maximum(genome.size - lengths, 1))
    buf = genome[(starts[rec] + within) % genome.size].copy()
    sub = rng.random(buf.size) < sub_rate
    buf[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    holed = np.flatnonzero((rng.random(lengths.size) < n_rate) & (lengths > 0))
    buf[off[holed] + rng.integers(0, lengths[holed])] = ord("N")
    buf[off[1:] - 1] = NL
    return buf, off.astype(np.uint64)


def windows_by_record(buf, off, k, path, pre):
    """(ends, values) per record: one walk of the oracle's iterators over the whole batch, cut at the record starts.  A window never
    spans a break byte, so the windows of the batch are the windows of its records."""
    ends, vals = T.windows_of(buf.tobytes(), k, path, pre)
    assert np.all(ends[1:] > ends[:-1])
    cuts = np.searchsorted(ends, off.astype(np.int64))
    return [(ends[a:b] - int(o), vals[a:b]) for a, b, o in zip(cuts[:-1], cuts[1:], off[:-1])]


def mixed_lengths(rng, n):
    """0 .. 400 bases: empty records, records shorter than k, the register path (up to 192 windows) and the streamed one."""
    lengths = rng.integers(0, 401, n)
    lengths[rng.random(n) < 0.03] = 0
    return lengths


@pytest.fixture(scope="module")
def read_batch(cu):
    """1.25 steps of the wave-per-record kernels (4 records per block, 8 blocks per CU): reads of a 30 kb genome, and their k-mers."""
    rng = np.random.default_rng(0x57E9)
    n = 5 * step_of("ra_wave_kernel", cu) // 4
    genome = ACGT[rng.integers(0, 4, 30_000)]
    buf, off = sampled_batch(rng, genome, mixed_lengths(rng, n))
    values = [v for _, v in windows_by_record(buf, off, K, BYTES, nt.PRE_NORMALIZE)]
    sizes = np.array([v.size for v in values])
    lengths = np.diff(off.astype(np.int64)) - 1
    assert int((lengths == 0).sum()) > 50 and int(((lengths > 0) & (lengths < K)).sum()) > 50
    assert int(((sizes > 0) & (sizes <= 192)).sum()) > 1000 and int((sizes > 192).sum()) > 1000
    assert int(((sizes < lengths - K + 1) & (lengths >= K)).sum()) > 100, "records with an N"
    return buf, off, values


def count_table(ctx, buf, k=K, path=BYTES, pre=nt.PRE_NORMALIZE):
    t = nt.KmerTable(k, path, max(int(buf.size), 16), ctx)
    t.count_device(upload(buf), int(buf.size), pre)
    ctx.synchronize()
    return t, oracle_items(buf.tobytes(), k, path, pre)


# ---- abundance ---------------------------------------------------------------------------------------------------------------------------

def test_abundance_records_take_a_second_step(ctx, cu, read_batch):
    """ra_wave_kernel: every wave of the capped grid takes a second record, a part of them; the table is counted from every third
    record, so k-mers are absent, rare and frequent."""
    buf, off, values = read_batch
    n = len(values)
    past_one_step("ra_wave_kernel", n, cu)
    third = np.concatenate([buf[int(off[r]):int(off[r + 1])] for r in range(0, n, 3)])
    t, items = count_table(ctx, third)
    with t, nt.ReadAbundance(t) as ra:
        for mc in (1, 3):
            want = A.rows_from_values(values, items, mc)
            assert int((want[:, 1] < want[:, 0]).sum()) > 1000 and int((want[:, 2] < want[:, 3]).sum()) > 1000
            got = host(ra.run_device(upload(buf), int(buf.size), dev_u64(off), n, nt.PRE_NORMALIZE, min_count=mc))
            same(got, want, ("abundance", mc))


def test_abundance_long_records_take_a_second_step(ctx, cu):
    """ra_block_kernel: n_cu + n_cu / 4 records of 65 537 .. 66 000 windows, each a read around a 3 kb genome whose k-mers the table
    holds at depths that vary, so the median needs its bit rounds; short records between them."""
    rng = np.random.default_rng(0xB10C)
    n_long = cu + cu // 4
    genome = ACGT[rng.integers(0, 4, 3000)]
    lengths = np.zeros(2 * n_long, dtype=np.int64)
    lengths[0::2] = rng.integers(65_537, 66_001, n_long) + K - 1
    lengths[1::2] = rng.integers(0, 120, n_long)
    buf, off = sampled_batch(rng, genome, lengths, sub_rate=0.002, n_rate=0.0, periodic=True)
    values = [v for _, v in windows_by_record(buf, off, K, BYTES, nt.PRE_NORMALIZE)]
    long_ones = sum(v.size > 65_536 for v in values)
    assert long_ones == n_long and max(v.size for v in values) <= 66_000
    past_one_step("ra_block_kernel", long_ones, cu)
    depth, _ = sampled_batch(rng, genome, rng.integers(30, 300, 400), sub_rate=0.0, n_rate=0.0)
    t, items = count_table(ctx, depth)
    want = A.rows_from_values(values, items, 2)
    rows_long = want[0::2]
    assert np.all(rows_long[:, 2] < rows_long[:, 3]) and np.all(rows_long[:, 3] < rows_long[:, 4]), "min < median < max in every long row"
    assert np.unique(rows_long[:, 3]).size > 1
    with t, nt.ReadAbundance(t) as ra:
        got = host(ra.run_device(upload(buf), int(buf.size), dev_u64(off), len(values), nt.PRE_NORMALIZE, min_count=2))
    same(got, want, "long records")


# ---- colors ------------------------------------------------------------------------------------------------------------------------------

def color_index(ctx, k, path, n_colors, keys, seed):
    """An index over `keys` with random masks (none, one, several and all bits), and its model."""
    rng = np.random.default_rng(seed)
    masks = random_masks(rng, keys.size, n_colors)
    model = KM.Index(n_colors)
    kc = nt.KmerColors(k, path, n_colors, 2 * keys.size + 16, ctx)
    kc.add_masks(keys, masks)
    model.add(keys, masks)
    ctx.synchronize()
    return kc, model


def run_screen(kc, dev, n_bytes, off, pre, single=True):
    rows, hits, alone = kc.run_device(dev, n_bytes, dev_u64(off), len(off) - 1, pre, single=single)
    return host(rows), host(hits), None if alone is None else host(alone)


def same_screen(got, want, what):
    for name, g, w in zip(("rows", "hits", "single"), got, want):
        if g is not None:
            same(g, w, (what, name))


@pytest.mark.parametrize("n_colors", [5, 64])
def test_colors_screen_records_take_a_second_step(ctx, cu, read_batch, n_colors):
    """kc_wave_kernel on the abundance batch, against an index of every fourth of its k-mers and as many foreign keys."""
    buf, off, values = read_batch
    past_one_step("kc_wave_kernel", len(values), cu)
    rng = np.random.default_rng(0xC0 + n_colors)
    own = np.unique(np.concatenate(values))[::4]
    keys = np.concatenate([own, rng.integers(0, 1 << 42, own.size, dtype=np.uint64)])
    kc, model = color_index(ctx, K, BYTES, n_colors, keys, 0xC1 + n_colors)
    with kc:
        want = KM.screen_values(values, model)
        assert int((want[0][:, 1] > 0).sum()) > 5000 and int((want[0][:, 1] < want[0][:, 0]).sum()) > 5000
        dev = upload(buf)
        same_screen(run_screen(kc, dev, int(buf.size), off, nt.PRE_NORMALIZE), want, n_colors)
        same_screen(run_screen(kc, dev, int(buf.size), off, nt.PRE_NORMALIZE, single=False), want, (n_colors, "no single"))


def test_colors_one_long_record_takes_a_second_step(ctx, cu):
    """kc_long_kernel: one record of 1.25 steps of valid windows, read around a 5 kb genome, between short reads; with and without the
    single matrix."""
    rng = np.random.default_rng(0x10F6)
    n_colors = 7
    windows = 5 * step_of("kc_long_kernel", cu) // 4
    genome = ACGT[rng.integers(0, 4, 5000)]
    lengths = np.concatenate([rng.integers(0, 200, 20), [windows + K - 1], rng.integers(0, 200, 20)])
    buf, off = sampled_batch(rng, genome, lengths, sub_rate=0.0, n_rate=0.0, periodic=True)
    values = [v for _, v in windows_by_record(buf, off, K, BYTES, nt.PRE_NORMALIZE)]
    assert values[20].size == windows > KM.LONG_RECORD
    past_one_step("kc_long_kernel", values[20].size, cu)
    own = np.unique(values[20])
    kc, model = color_index(ctx, K, BYTES, n_colors, own[::2], 0x10F7)
    with kc:
        want = KM.screen_values(values, model)
        assert 0 < int(want[0][20, 1]) < windows and 0 < int(want[0][20, 2]) < int(want[0][20, 1])
        dev = upload(buf)
        for single in (True, False):
            same_screen(run_screen(kc, dev, int(buf.size), off, nt.PRE_NORMALIZE, single=single), want, ("long", single))


def lowest_bits(m):
    """(lowest set bit, next set bit) of every mask, NONE where there is none."""
    def lowest(x):
        low = x & (~x + U(1))
        # the index of a power of two: its value - 1 has that many ones
        v = low - U(1)
        n = np.zeros(x.size, dtype=np.uint64)
        for s in (32, 16, 8, 4, 2, 1):
            big = (v >> U(s)) != 0
            n += np.where(big, U(s), U(0))
            v = np.where(big, v >> U(s), v)
        n += v   # 0 or 1 left
        return np.where(x == 0, U(KM.NONE), n)
    return lowest(m), lowest(m & (m - U(1)))


def test_colors_best_of_one_window_records(ctx, cu):
    """kc_best_kernel (and kc_wave_kernel over 80 steps): records of exactly k bases, one window each, so every row follows from the
    looked-up mask of its one k-mer - hits are its bits, best its lowest set bit (every hit colour has one hit: ties go to the smallest
    colour) and second the next."""
    rng = np.random.default_rng(0xBE57)
    n_colors, path, pre = 64, BITS, nt.PRE_NONE
    n = 5 * step_of("kc_best_kernel", cu) // 4
    keys = np.unique(rng.integers(0, 1 << 42, 50_000, dtype=np.uint64))
    times = np.full(keys.size, n // keys.size, dtype=np.int64)
    times[: n - int(times.sum())] += 1
    raw = np.frombuffer(CM.records_for(keys, times, K, seed=5), dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * U(K + 1)
    past_one_step("kc_best_kernel", n, cu)
    ends, vals = T.windows_of(raw.tobytes(), K, path, pre)
    assert vals.size == n and np.array_equal(ends, np.arange(n) * (K + 1) + K - 1), "one window per record"
    kc, model = color_index(ctx, K, path, n_colors, keys[::2], 0xBE58)
    with kc:
        m = model.lookup(vals)
        best, second = lowest_bits(m)
        one = (m != 0) & (m & (m - U(1)) == 0)
        want_rows = np.stack([np.ones(n, dtype=np.uint64), (m != 0).astype(np.uint64), one.astype(np.uint64), best, second], axis=1)
        want_hits = (m[:, None] >> np.arange(n_colors, dtype=np.uint64)[None, :]) & U(1)
        sample = rng.integers(0, n, 200)
        for r in sample.tolist():   # the closed form against the model's own rule
            row, hits, _ = KM.screen_masks(m[r:r + 1], n_colors)
            assert np.array_equal(row, want_rows[r]) and np.array_equal(hits, want_hits[r])
        assert int((second != U(KM.NONE)).sum()) > n // 8 and int((m == 0).sum()) > n // 4
        rows, hits, alone = run_screen(kc, upload(raw), int(raw.size), off, pre)
        same(rows, want_rows, "best rows")
        same(hits, want_hits, "best hits")
        same(alone, want_hits * one[:, None].astype(np.uint64), "best single")


def or_by_key(keys, masks):
    """The index by definition, on arrays: (distinct keys ascending, the OR of each one's masks), keys whose OR is 0 left out."""
    order = np.argsort(keys, kind="stable")
    k, m = keys[order], masks[order]
    first = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    ored = np.bitwise_or.reduceat(m, first)
    return k[first][ored != 0], ored[ored != 0]


@pytest.mark.parametrize("which", ["census", "keys", "one step", "one step and a key"])
def test_colors_index_of_many_keys(ctx, cu, which):
    """kc_add_kernel, kc_lookup_kernel and kc_census_kernel past one step: per-key masks (a tenth of the keys twice), every key and as
    many absent ones looked up, n_keys and per_color from stats.  "census": just enough keys for the slots to take a second step of
    the census; "keys": 1.25 steps of keys; the last two: exactly one step of keys and queries, and one more."""
    n_colors = 64
    key_step, slot_step = step_of("kc_add_kernel", cu), step_of("kc_census_kernel", cu)
    n = {"census": 3 * slot_step // 4 + 1000, "keys": 5 * key_step // 4, "one step": key_step, "one step and a key": key_step + 1}[which]
    rng = np.random.default_rng(0x1DE + n % 997)
    distinct = np.unique(rng.integers(0, 1 << 62, n, dtype=np.uint64))
    keys = np.concatenate([distinct, distinct[rng.random(distinct.size) < 0.1]])
    rng.shuffle(keys)
    keys = keys[:n]
    assert keys.size == n and np.unique(keys).size < n
    masks = random_masks(rng, n, n_colors)
    absent = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    if which in ("census", "keys"):
        queries = np.concatenate([keys, absent])
    else:
        queries = np.concatenate([keys[: n // 2], absent])[:n]
    if which == "keys":
        past_one_step("kc_add_kernel", keys.size, cu)
        past_one_step("kc_lookup_kernel", queries.size, cu, whole=2)
    want_keys, want_masks = or_by_key(keys, masks)
    at = np.minimum(np.searchsorted(want_keys, queries), want_keys.size - 1)
    want_lookup = np.where(want_keys[at] == queries, want_masks[at], U(0))
    with nt.KmerColors(K, BITS, n_colors, n, ctx) as kc:
        kc.add_masks(keys, masks)
        st = kc.stats()
        assert st["slots"] > slot_step, f"kc_census_kernel: {st['slots']} slots at {slot_step} per step on {cu} CUs"
        assert st["n_dropped"] == 0 and st["n_keys"] == want_keys.size and st["n_masked_bits"] == 0
        per_color = ((want_masks[:, None] >> np.arange(n_colors, dtype=np.uint64)[None, :]) & U(1)).sum(axis=0)
        assert st["per_color"] == per_color.tolist()
        same(kc.lookup(queries), want_lookup, ("lookup", which))
    # the model's own index on a slice, so that the definition above is the model's
    model = KM.Index(n_colors)
    model.add(keys[:5000], masks[:5000])
    k5, m5 = or_by_key(keys[:5000], masks[:5000])
    assert model.n_keys == k5.size and np.array_equal(model.lookup(k5), m5)


# ---- trim --------------------------------------------------------------------------------------------------------------------------------

def test_trim_records_take_a_second_step(ctx, cu):
    """rt_interval_kernel (1.25 steps) and rt_copy_kernel (2.5 steps): reads of k .. 3k bases of a genome with 2 % substitutions against
    the table of the genome itself, so a read is whole, cut at its first error or dropped; every 2 000th record is one of more than
    kGroup * kGroupRounds plane words, so the group path and the whole-wave path alternate inside a wave's stride.  Both modes, and
    the compaction of each."""
    rng = np.random.default_rng(0x7819)
    k, path, pre = K, BYTES, nt.PRE_NORMALIZE
    n = 5 * step_of("rt_interval_kernel", cu) // 4
    past_one_step("rt_interval_kernel", n, cu)
    past_one_step("rt_copy_kernel", n, cu, whole=2)
    genome = ACGT[rng.integers(0, 4, 60_000)]
    lengths = rng.integers(k, 3 * k + 1, n)
    short = rng.random(n) < 0.02
    lengths[short] = rng.integers(0, k, int(short.sum()))
    long_at = np.arange(700, n, 2000)
    lengths[long_at] = rng.integers(2200, 3000, long_at.size)   # more than 32 words of 64 bases
    buf, off = sampled_batch(rng, genome, lengths, sub_rate=0.02, n_rate=0.02)
    gbuf = np.concatenate([genome, [NL]]).astype(np.uint8)
    t, items = count_table(ctx, gbuf)
    wins = windows_by_record(buf, off, k, path, pre)
    counts = [A.lookup(v, items) for _, v in wins]
    records = [buf[int(off[r]):int(off[r + 1]) - 1].tobytes() for r in range(n)]
    words = (off[1:].astype(np.int64) - 2) // 64 - (off[:-1].astype(np.int64) + k - 1) // 64 + 1
    assert int((words[long_at] > 32).sum()) == long_at.size and int((words > 32).sum()) == long_at.size
    dev, d_off = upload(buf), dev_u64(off)
    aux = rng.integers(33, 127, buf.size).astype(np.uint8)
    d_aux = upload(aux)
    with t, nt.ReadTrimmer(t) as rt:
        for mode in (T.PREFIX, T.LONGEST):
            want = np.zeros((n, 4), dtype=np.uint64)
            for r in range(n):
                want[r] = T.row(int(lengths[r]), k, wins[r][0], counts[r], mode)
            whole, dropped = int((want[:, 1] == lengths).sum()), int(((want[:, 1] == 0) & (lengths >= k)).sum())
            cut = int(((want[:, 1] > 0) & (want[:, 1] < lengths)).sum())
            assert min(whole, dropped, cut) > 1000, (mode, whole, dropped, cut)
            rows = rt.run_device(dev, int(buf.size), d_off, n, pre, mode=mode)
            same(host(rows), want, ("trim rows", mode))
            seq, n_bytes, offsets, source, out_aux = rt.compact_device(dev, int(buf.size), d_off, n, rows, d_aux=d_aux)
            auxs = [aux[int(off[r]):int(off[r + 1]) - 1] for r in range(n)]
            w_seq, w_bytes, w_off, w_src, w_aux = T.compact(records, want, auxs, aux[off[1:].astype(np.int64) - 1])
            assert n_bytes == w_bytes and np.array_equal(host(offsets), w_off) and np.array_equal(host(source), w_src)
            assert np.array_equal(host(seq)[: len(w_seq)], np.frombuffer(w_seq, dtype=np.uint8)), mode
            assert np.array_equal(host(out_aux)[:w_bytes], np.frombuffer(w_aux, dtype=np.uint8)[:w_bytes]), mode


# ---- record_minhash ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [dict(num=16), dict(scaled=7)], ids=["num16", "scaled7"])
def test_record_minhash_records_take_a_second_step(ctx, cu, kind):
    """rmh_windows_kernel: one block per record, 1.25 steps of records; some blocks `continue` over an empty or sub-k record before
    they count the windows of their second one."""
    rng = np.random.default_rng(0x4D49)
    step = step_of("rmh_windows_kernel", cu)
    n = 5 * step // 4
    past_one_step("rmh_windows_kernel", n, cu)
    genome = ACGT[rng.integers(0, 4, 200_000)]
    buf, off = sampled_batch(rng, genome, mixed_lengths(rng, n), sub_rate=0.0, n_rate=0.1)
    values = [v for _, v in windows_by_record(buf, off, K, BYTES, nt.PRE_NORMALIZE)]
    sizes = np.array([v.size for v in values])
    second = np.arange(step, n)
    assert int(((sizes[second - step] == 0) & (sizes[second] > 0)).sum()) > 5, "a block skips its first record and counts its second"
    assert int(((sizes[second - step] > 0) & (sizes[second] == 0)).sum()) > 5
    want = R.csr(values, **kind)
    with nt.RecordMinHash(K, BYTES, ctx=ctx, **kind) as rmh:
        rmh.run_device(upload(buf), int(buf.size), dev_u64(off), n, nt.PRE_NORMALIZE)
        got = rmh.sketches()
        for name, g, w in zip(("offsets", "n_windows", "hashes", "counts"), got, want):
            same(g, w, (kind, name))
        assert rmh.stats()["n_windows"] == int(sizes.sum())


# ---- kmer_sets ---------------------------------------------------------------------------------------------------------------------------

def as_wide(v):
    """Narrow keys below 2^62 as {hi, lo} rows in the same order: the top 32 bits, then the low 30 above 34 bits of noise."""
    v = np.asarray(v, dtype=np.uint64)
    return np.stack([v >> U(30), ((v & U((1 << 30) - 1)) << U(34)) | (CM.fmix64(v) & U((1 << 34) - 1))], axis=1)


def key_set(ctx, keys, counts, kw):
    k = 21 if kw == 1 else 41
    s = nt.KmerSet(dev_u64(as_wide(keys) if kw == 2 else keys), dev_u64(counts), int(counts.size), k, BYTES, ctx)
    torch.cuda.synchronize()
    return s


@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("n", ["1.25 steps", "one step", "one step and a pair"])
def test_kmer_sets_validate_in_the_second_step(ctx, cu, kw, n):
    """ks_validate_kernel: an ascending list counts no violation; a swapped pair and a duplicate planted among the pairs of the second
    step count one each (the swapped pair breaks one order, and both its neighbours still ascend)."""
    step = step_of("ks_validate_kernel", cu)
    pairs = {"1.25 steps": 5 * step // 4, "one step": step, "one step and a pair": step + 1}[n]
    if n == "1.25 steps":
        past_one_step("ks_validate_kernel", pairs, cu)
    rng = np.random.default_rng(0x7A11 + kw)
    keys = np.cumsum(rng.integers(3, 1 << 41, pairs + 1, dtype=np.uint64))
    assert int(keys[-1]) < 1 << 62
    with key_set(ctx, keys, np.ones(keys.size, dtype=np.uint64), kw) as s:
        assert s.violations() == 0
    if pairs > step + 8:
        bad = keys.copy()
        a, b = step + (pairs - step) // 3, step + 2 * (pairs - step) // 3
        bad[[a, a + 1]] = bad[[a + 1, a]]
        bad[b + 1] = bad[b]
        wide_rows = as_wide(bad) if kw == 2 else bad.reshape(-1, 1)
        lex = (wide_rows[1:, 0] > wide_rows[:-1, 0]) | ((wide_rows[1:, 0] == wide_rows[:-1, 0]) & (wide_rows[1:, -1] > wide_rows[:-1, -1]))
        assert int((~lex).sum()) == 2 and not lex[a] and not lex[b] and min(a, b) >= step
        with key_set(ctx, bad, np.ones(bad.size, dtype=np.uint64), kw) as s:
            assert s.violations() == 2
    else:   # the last pair, which is the second step's only one where there is one
        bad = keys.copy()
        bad[-1] = bad[-2]
        with key_set(ctx, bad, np.ones(bad.size, dtype=np.uint64), kw) as s:
            assert s.violations() == 1


RULES = {"min": np.minimum, "max": np.maximum, "left": lambda a, b: a, "right": lambda a, b: b}


@pytest.mark.parametrize("kw", [1, 2])
def test_kmer_sets_every_op_takes_a_third_tile(ctx, cu, kw):
    """ks_join_kernel: two lists whose merge has more than 1.25 x 2 x the grid's blocks of tiles, so a part of the blocks take a third
    tile; every op and rule and the joint spectrum against numpy set algebra on the narrow values (the wide lists hold the same
    values as {hi, lo} rows in the same order).  Counts near 2^64 make "sum" saturate."""
    rng = np.random.default_rng(0x5E75 + kw)
    tile = 2048 // kw
    tiles = 5 * step_of("ks_join_kernel", cu) // 4 + 3
    n_a, n_b = (tiles * tile * 27) // 53, (tiles * tile * 26) // 53
    pool = np.unique(rng.integers(0, 1 << 62, 3 * (n_a + n_b) // 4, dtype=np.uint64))
    a = np.sort(rng.choice(pool, n_a, replace=False))
    b = np.sort(rng.choice(pool, n_b, replace=False))
    past_one_step("ks_join_kernel", -(-(a.size + b.size) // tile), cu)
    ca, cb = rng.integers(1, 300, a.size, dtype=np.uint64), rng.integers(1, 12, b.size, dtype=np.uint64)
    ca[::1001] = U(2 ** 64 - 5)
    shared, ia, ib = np.intersect1d(a, b, assume_unique=True, return_indices=True)
    assert shared.size > n_b // 4 and int((ca[ia] == U(2 ** 64 - 5)).sum()) > 10
    in_a, in_b = np.zeros(a.size, dtype=bool), np.zeros(b.size, dtype=bool)
    in_a[ia], in_b[ib] = True, True
    b_of_a = np.zeros(a.size, dtype=np.uint64)
    b_of_a[ia] = cb[ib]
    union = np.concatenate([a, b[~in_b]])
    order = np.argsort(union, kind="stable")
    total = ca[ia] + cb[ib]
    rules = dict(RULES, sum=lambda x, y: np.where(x + y < x, U(2 ** 64 - 1), x + y))
    assert int((total < ca[ia]).sum()) > 10, "sums that saturate"
    keyed = (lambda v: as_wide(v)) if kw == 2 else (lambda v: v)
    with key_set(ctx, a, ca, kw) as sa, key_set(ctx, b, cb, kw) as sb:
        def held(out, keys, counts, what):
            with out:
                gk, gc = out.items()
                same(gk, keyed(keys), (what, "keys"))
                same(gc, counts, (what, "counts"))
        for name, f in rules.items():
            held(sa.intersect(sb, name), shared, f(ca[ia], cb[ib]), ("intersect", name))
            both = ca.copy()
            both[ia] = f(ca[ia], cb[ib])
            held(sa.union(sb, name), union[order], np.concatenate([both, cb[~in_b]])[order], ("union", name))
        held(sa.subtract(sb), a[~in_a], ca[~in_a], "subtract")
        more = ca > b_of_a
        held(sa.counters_subtract(sb), a[more], (ca - b_of_a)[more], "counters_subtract")
        hist, totals = sa.compare(sb, 64, 16)
        want = np.zeros((64, 16), dtype=np.uint64)
        np.add.at(want, (np.minimum(ca, U(63)).astype(np.int64), np.minimum(b_of_a, U(15)).astype(np.int64)), 1)
        np.add.at(want, (np.zeros(int((~in_b).sum()), dtype=np.int64), np.minimum(cb[~in_b], U(15)).astype(np.int64)), 1)
        same(hist, want, "hist")
        assert (totals["n_a"], totals["n_b"], totals["n_shared"]) == (a.size, b.size, shared.size)
        assert totals["sum_b"] == int(cb.sum()) and totals["sum_b_only"] == int(cb[~in_b].sum())
        assert totals["sum_a"] == int(ca.sum(dtype=np.uint64)), "modulo 2^64, as numpy's uint64 sum"
        assert totals["sum_min"] == int(np.minimum(ca[ia], cb[ib]).sum())


# ---- dbg ---------------------------------------------------------------------------------------------------------------------------------

def dbg_keys_31(rng, target):
    """(keys, k-mers of the path, k-mers of the cycle): one path of 3 / 8 of `target` k-mers (491 520 at 256 CUs), one cycle of 7 / 32
    (286 720), one short sequence per 437 keys (3 000, some 90 000 k-mers), and isolated k-mers up to `target` keys."""
    k = 31
    n_path, n_ring = 3 * target // 8, 7 * target // 32
    parts = [DM.kmers_of_codes(rng.integers(0, 4, n_path + k - 1), k)]
    ring = rng.integers(0, 4, n_ring)
    parts.append(DM.kmers_of_codes(np.concatenate([ring, ring[:k - 1]]), k))
    for L in rng.integers(k, k + 60, target // 437).tolist():
        parts.append(DM.kmers_of_codes(rng.integers(0, 4, L), k))
    have = np.unique(np.concatenate(parts))
    assert have.size < 3 * target // 4   # (a share of the target whatever the device)
    v = np.zeros(target - have.size, dtype=np.uint64)
    for _ in range(k):
        v = (v << U(2)) | rng.integers(0, 4, v.size, dtype=np.uint64)
    lone = np.minimum(v, CM.revcomp(v, k))
    keys = np.unique(np.concatenate([have, lone]))
    assert target - 16 <= keys.size <= target
    return keys, n_path, n_ring


def dbg_keys_15(rng, target):
    """The k-mers of random sequences of 1 000 bases: at this density chance overlaps of k - 1 bases branch the graph."""
    k = 15
    n_seq = -(-target // (1000 - k + 1)) + 8   # (a few more: about one k-mer in a thousand comes twice)
    return np.unique(np.concatenate([DM.kmers_of_codes(rng.integers(0, 4, 1000), k) for _ in range(n_seq)]))


@pytest.mark.parametrize("k", [31, 15])
def test_dbg_lists_take_a_second_step(ctx, cu, k):
    """All ten dbg kernels: 1.25 steps of k-mers (2.5 of states).  Edge bytes, totals, k-mer rows, unitig rows and the spelled batch
    against the array model, and the ranking rounds against the longest path."""
    rng = np.random.default_rng(0xDB6 + k)
    target = 5 * step_of("dbg_adjacency_kernel", cu) // 4
    keys, n_path, n_ring = dbg_keys_31(rng, target) if k == 31 else (dbg_keys_15(rng, target), 0, 0)
    past_one_step("dbg_adjacency_kernel", keys.size, cu)
    past_one_step("dbg_link_kernel", 2 * keys.size, cu, whole=2)
    counts = DM.counts_for(keys)
    m = DM.ArrayGraph(keys, counts, k)
    t = m.totals()
    paths = m.unitig_rows[(m.unitig_rows[:, 3] & U(1)) == 0, 1]
    longest = int(paths.max())
    if k == 31:
        assert longest == n_path and int(m.unitig_rows[(m.unitig_rows[:, 3] & U(1)) == 1, 1].max()) == n_ring
        assert t["n_isolated"] > target // 16 and m.n_unitigs > target // 16
    else:
        assert t["n_branching"] > 1000 and t["n_tips"] > 1000 and t["n_self"] > 0 and longest > 64
    s = nt.KmerSet(dev_u64(keys), dev_u64(counts), int(keys.size), k, nt.PATH_BITS_CANONICAL, ctx)
    with nt.KmerGraph(s) as g:
        stats, _ = hold_graph(g, m, int(keys.size), f"k = {k}")
    assert stats["n_rounds"] >= math.ceil(math.log2(longest)), (stats["n_rounds"], longest)


@pytest.mark.parametrize("extra", [0, 1], ids=["one step", "one step and a key"])
def test_dbg_adjacency_at_one_step_and_one_more(ctx, cu, extra):
    """dbg_dir_mark_kernel, dbg_adjacency_kernel and dbg_link_kernel on exactly one step of k-mers (two of states) and on one k-mer more:
    the first keys of the k = 15 list (any ascending subset of canonical k-mers is a list).  What the three kernels answer is the edge
    bytes and the totals, which the array model has before its walk."""
    k = 15
    n = step_of("dbg_adjacency_kernel", cu) + extra
    keys = dbg_keys_15(np.random.default_rng(0xDB6 + k), n)[:n]
    assert keys.size == n
    print(f"dbg_adjacency_kernel: {n} items at {n - extra} per step on {cu} CUs: one step and {extra}")
    m = DM.ArrayGraph(keys, DM.counts_for(keys), k, walk=False)
    want = m.totals()
    assert want["n_branching"] > 1000 and want["n_tips"] > 1000 and want["n_links"] > n
    s = nt.KmerSet(dev_u64(keys), dev_u64(DM.counts_for(keys)), n, k, nt.PATH_BITS_CANONICAL, ctx)
    with nt.KmerGraph(s) as g:
        edges, totals = g.edges().cpu().numpy(), g.totals()
    same(edges, m.edges, ("edges", n))
    for key in DM.TOTALS:
        assert np.array_equal(totals[key], want[key]), (key, totals[key], want[key])


# ---- wide_count and minhash: the k > 32 kernels the inventory found under one step ----------------------------------------------------------

def wide_keys(rng, n, k):
    """n distinct canonical {hi, lo} keys of 2k bits, ascending."""
    hi, lo = WM.canonical(rng.integers(0, 1 << (2 * k - 64), n + n // 8, dtype=np.uint64), rng.integers(0, 1 << 64, n + n // 8, dtype=np.uint64), k)
    rows = np.unique(np.stack([hi, lo], axis=1), axis=0)
    assert rows.shape[0] >= n
    return rows[:n]


def test_wide_lookup_takes_a_second_step(ctx, cu):
    """wt_lookup_kernel: 1.25 steps of queries - every key of the table on a random strand, the rest absent keys."""
    rng = np.random.default_rng(0x41D)
    k = 41
    n_q = 5 * step_of("wt_lookup_kernel", cu) // 4
    past_one_step("wt_lookup_kernel", n_q, cu)
    rows = wide_keys(rng, 60_000, k)
    counts = rng.integers(1, 4, rows.shape[0])
    raw = np.frombuffer(WM.records_for(rows[:, 0], rows[:, 1], counts, k, seed=3), dtype=np.uint8)
    absent = wide_keys(rng, 40_000, k)
    have = set(map(tuple, rows.tolist()))
    assert not any(tuple(x) in have for x in absent.tolist())
    pick = rng.integers(0, rows.shape[0] + absent.shape[0], n_q)
    pool = np.concatenate([rows, absent])
    want = np.concatenate([counts.astype(np.uint64), np.zeros(absent.shape[0], dtype=np.uint64)])[pick]
    q = pool[pick]
    rh, rl = WM.revcomp(q[:, 0], q[:, 1], k)
    flip = rng.random(n_q) < 0.5
    q = np.stack([np.where(flip, rh, q[:, 0]), np.where(flip, rl, q[:, 1])], axis=1)
    with nt.WideKmerTable(k, BYTES, 2 * rows.shape[0], ctx) as t:
        t.count_device(upload(raw), int(raw.size), nt.PRE_NORMALIZE)
        ctx.synchronize()
        st = t.stats()
        assert st["n_distinct"] == rows.shape[0] and st["n_total"] == int(counts.sum()) and st["n_dropped"] == 0
        same(t.lookup(q), want, "wide lookup")


def test_wide_minhash_takes_a_second_step(ctx, cu):
    """mh_wide_filter_kernel: a scaled sketch takes the batch in one launch of one thread per run of 64 bytes; 1.25 steps of runs of
    records of exactly k bases, whose keys are known."""
    rng = np.random.default_rng(0x41E)
    k, scaled = 41, 2000
    runs = 5 * step_of("mh_wide_filter_kernel", cu) // 4
    n_rec = runs * 64 // (k + 1)
    rows = wide_keys(rng, n_rec - n_rec // 10, k)
    counts = np.ones(rows.shape[0], dtype=np.int64)
    counts[: n_rec - rows.shape[0]] = 2
    raw = np.frombuffer(WM.records_for(rows[:, 0], rows[:, 1], counts, k, seed=4), dtype=np.uint8)
    past_one_step("mh_wide_filter_kernel", -(-raw.size // 64), cu)
    want_h, want_c = M.sketch(np.repeat(rows, counts, axis=0), scaled=scaled)
    assert want_h.size > 200 and int(want_c.max()) == 2
    with nt.KmerMinHash(k, BYTES, scaled=scaled, ctx=ctx) as mh:
        mh.add_device(upload(raw), int(raw.size), nt.PRE_NORMALIZE)
        h, c = mh.hashes()
        assert mh.stats()["n_windows"] == int(counts.sum())
        same(h, want_h, "wide minhash hashes")
        same(c, want_c, "wide minhash counts")
