"""The de Bruijn graph library on the GPU (include/needletail_amd_dbg.h, needletail_amd/dbg.py) against tests/_dbg_model.py: edge bytes,
totals, k-mer rows, unitig rows and spelled bytes, all with array_equal.  Inputs are a few thousand keys at most.  k = 31 keys have 62
bits, so "the top bits set" means bits 61 and 60 (a first base T)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import needletail_amd as nt  # noqa: E402
from needletail_amd import dbg as D  # noqa: E402
import _dbg_model as DM  # noqa: E402
from _lib_fuzz import hold_graph  # noqa: E402

pytestmark = pytest.mark.gpu

CANON = nt.PATH_BITS_CANONICAL
ERR_BAD_ARG, ERR_CAPACITY = 2, 5
BLOCK = 256   # kThreads of ntk_consumer.hpp: a block's k-mers of one grid-stride step


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


def make(ctx, keys, counts, k):
    """A KmerSet straight from ascending host arrays."""
    s = nt.KmerSet(_dev(keys), _dev(counts), len(keys), k, CANON, ctx)
    torch.cuda.synchronize()
    return s


def hold(ctx, k, keys, counts, name):
    """Everything KmerGraph answers for the list, held to the model (`_lib_fuzz.hold_graph`, which the structured fuzz shares).  Returns
    (model, stats)."""
    m = DM.Graph(keys, counts, k)
    with nt.KmerGraph(make(ctx, keys, counts, k)) as g:
        stats, _ = hold_graph(g, m, len(keys), name)
    return m, stats


def test_subsets_of_3_mers_and_5_mers(ctx):
    """The CPU suite's cases: random subsets of all canonical 3-mers and 5-mers, and every 61st subset of its 14-key universe."""
    for name, k, keys in DM.subset_cases():
        hold(ctx, k, keys, DM.counts_for(keys), name)
    universe = DM.universe_keys()
    for mask in list(range(0, 1 << 14, 61)) + [(1 << 14) - 1]:
        keys = universe[[(mask >> j) & 1 == 1 for j in range(14)]]
        hold(ctx, 3, keys, DM.counts_for(keys, mask), f"subset {mask:#x}")


def test_sequences_at_k_15_and_31(ctx):
    for name, k, keys in DM.sequence_cases():
        hold(ctx, k, keys, DM.counts_for(keys), name)


LONG = 3000


def _long_sequence():
    rng = np.random.default_rng(0x10C)
    return DM.random_sequence(rng, LONG + 14)


def test_a_long_path_needs_its_rounds(ctx):
    keys = DM.keys_of([_long_sequence()], 15)
    m, stats = hold(ctx, 15, keys, DM.counts_for(keys), "long path")
    assert m.n_unitigs == 1 and len(keys) == LONG and not int(m.unitig_rows[0, 3]) & 1
    assert stats["n_rounds"] >= math.ceil(math.log2(LONG)) > 11
    assert stats["n_rounds"] <= math.ceil(math.log2(LONG)) + 1   # no cycle: one pass


def test_the_same_sequence_as_a_cycle(ctx):
    keys = DM.keys_of([_long_sequence()], 15, circular=True)
    m, stats = hold(ctx, 15, keys, DM.counts_for(keys), "long cycle")
    assert m.n_unitigs == 1 and int(m.unitig_rows[0, 3]) & 1 and int(m.unitig_rows[0, 1]) == len(keys) == LONG + 14
    assert stats["n_rounds"] >= 2 * math.ceil(math.log2(LONG))   # the pass that finds the cycle and the pass that ranks it


def test_k_31_keys_with_their_top_bits_set(ctx):
    rng = np.random.default_rng(0x31)
    # reads that begin with T and end with A: their first k-mer's reverse complement begins with T too, so whichever is smaller does
    seqs = ["T" + DM.random_sequence(rng, 29) + "A" + DM.random_sequence(rng, int(L)) for L in rng.integers(0, 40, 40)]
    keys = DM.keys_of(seqs, 31)
    assert int((keys >> np.uint64(60) == 3).sum()) >= 20 and int(keys.max()) < 1 << 62
    hold(ctx, 31, keys, DM.counts_for(keys), "k31 top bits")


def test_directory_with_empty_buckets_and_with_one_bucket(ctx):
    rng = np.random.default_rng(0xD1)
    # empty buckets: canonical keys rarely begin with T, so the last prefixes of the directory hold nothing
    keys = DM.keys_of([DM.random_sequence(rng, 700)], 31)
    b = math.ceil(math.log2(len(keys)))
    filled = np.unique(keys >> np.uint64(62 - b))
    assert len(filled) < (1 << b) - 8 and int(filled.max()) < (1 << b) - 1
    hold(ctx, 31, keys, DM.counts_for(keys), "empty buckets")
    # one bucket: 15-mers that begin with eight A (all canonical), so the top 16 bits of every key are 0
    x = np.flatnonzero(rng.random(2048) < 0.3).astype(np.uint64)
    assert 256 < len(x) < 1024
    m, _ = hold(ctx, 15, x, DM.counts_for(x), "one bucket")
    assert m.totals()["n_half_edges"] > 0
    # and a list as dense as lists get: all canonical 5-mers, the directory as wide as the key
    full = DM.all_canonical(5)
    hold(ctx, 5, full, DM.counts_for(full), "all 5-mers")


def test_a_neighbour_in_another_block(ctx):
    rng = np.random.default_rng(0xB10C)
    keys = DM.keys_of([DM.random_sequence(rng, BLOCK + 20 + 14)], 15)
    assert BLOCK < len(keys) <= BLOCK + 20
    m, _ = hold(ctx, 15, keys, DM.counts_for(keys), "just over a block")
    assert any((i < BLOCK) != (j < BLOCK) for (i, _, _), (j, _, _) in m.mate.items())


def test_capacity_round_trips(ctx):
    lib = D.lib()
    rng = np.random.default_rng(0xCA9)
    k = 15
    keys = DM.keys_of([DM.random_sequence(rng, int(L)) for L in rng.integers(k, 60, 30)], k)
    counts = DM.counts_for(keys)
    m = DM.Graph(keys, counts, k)
    n, need = len(keys), m.n_unitigs
    assert need > 3
    s = make(ctx, keys, counts, k)
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    with nt.KmerGraph(s) as g:
        h = g._h
        nu, nb = C.c_uint64(0), C.c_uint64(0)
        # unitigs: the query, one short, exact
        assert lib.ntk_dbg_unitigs_device(h, vp(s.keys), vp(s.counts), n, None, None, 0, C.byref(nu), C.byref(nb)) == ERR_CAPACITY
        assert (nu.value, nb.value) == (need, m.n_bases)
        kmer_rows = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
        unitig_rows = torch.full((need, 4), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert lib.ntk_dbg_unitigs_device(h, vp(s.keys), vp(s.counts), n, vp(kmer_rows), vp(unitig_rows), need - 1, C.byref(nu),
                                          C.byref(nb)) == ERR_CAPACITY
        assert nu.value == need and bool((kmer_rows == -1).all()) and bool((unitig_rows == -1).all()), "nothing written"
        assert lib.ntk_dbg_unitigs_device(h, vp(s.keys), vp(s.counts), n, None, vp(unitig_rows), need, C.byref(nu), C.byref(nb)) == ERR_BAD_ARG
        assert lib.ntk_dbg_unitigs_device(h, vp(s.keys), vp(s.counts), n, vp(kmer_rows), vp(unitig_rows), need, C.byref(nu), C.byref(nb)) == 0
        assert np.array_equal(unitig_rows.cpu().numpy().view(np.uint64), m.unitig_rows)
        assert np.array_equal(kmer_rows.cpu().numpy().view(np.uint32), m.kmer_rows)
        # spell: the query, a byte capacity one step short, a record capacity one short, exact
        text, off = m.batch()
        ob, orec = C.c_uint64(0), C.c_uint64(0)
        spell = lambda seq, cap_b, offs, cap_r: lib.ntk_dbg_spell_device(   # noqa: E731
            h, vp(s.keys), n, vp(kmer_rows), vp(unitig_rows), need, None if seq is None else vp(seq), cap_b, None if offs is None else vp(offs),
            cap_r, C.byref(ob), C.byref(orec))
        assert spell(None, 0, None, 0) == ERR_CAPACITY and (ob.value, orec.value) == (int(off[-1]), need)
        seq = torch.full((text.size,), 7, dtype=torch.uint8, device="cuda")
        offs = torch.full((need + 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert spell(seq, text.size - 16, offs, need) == ERR_CAPACITY
        assert spell(seq, text.size, offs, need - 1) == ERR_CAPACITY
        assert bool((seq == 7).all()) and bool((offs == -1).all()), "nothing written"
        assert spell(None, text.size, offs, need) == ERR_BAD_ARG
        assert spell(seq, text.size, offs, need) == 0 and (ob.value, orec.value) == (int(off[-1]), need)
        assert np.array_equal(seq.cpu().numpy(), text) and np.array_equal(offs.cpu().numpy().view(np.uint64), off)
        # a refused list size changes nothing
        nu.value = 99
        assert lib.ntk_dbg_unitigs_device(h, vp(s.keys), vp(s.counts), 1 << 31, None, None, 0, C.byref(nu), C.byref(nb)) == 6 and nu.value == 99
        assert lib.ntk_dbg_adjacency_device(h, vp(s.keys), 1 << 31, None, None) == 6
        st = g.stats()
        assert st["k"] == k and st["device_bytes"] > D.UNITIG_BYTES_PER_KMER * n and st["n_calls"] >= 5 and st["n_launches"] > 20
        g.release()
        assert g.stats()["device_bytes"] == 128 * 8


def test_an_empty_list(ctx):
    m, stats = hold(ctx, 21, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), "empty")
    assert m.n_unitigs == 0 and stats["n_launches"] == 0 and stats["n_rounds"] == 0


def test_counting_the_unitigs_gives_back_the_table(ctx):
    """Reads -> KmerTable -> KmerSet.from_table -> KmerGraph.unitig_batch -> a fresh table: exactly the original keys, each once."""
    rng = np.random.default_rng(0xE2E)
    k = 21
    genome = DM.random_sequence(rng, 1500)
    reads = []
    for _ in range(120):
        at = int(rng.integers(0, len(genome) - 100))
        r = list(genome[at: at + 100])
        if rng.random() < 0.3:
            r[int(rng.integers(0, 100))] = "ACGT"[int(rng.integers(0, 4))]
        r = "".join(r)
        reads.append((DM.rc(r) if rng.random() < 0.5 else r).encode())
    with nt.KmerTable(k, nt.PATH_BYTES_CANONICAL, 1 << 15, ctx) as table, nt.KmerTable(k, nt.PATH_BYTES_CANONICAL, 1 << 15, ctx) as again:
        table.count_records(reads, nt.PRE_NORMALIZE)
        keys, counts = table.items()
        assert np.array_equal(keys, DM.keys_of([r.decode() for r in reads], k)) and int(counts.max()) > 1
        s = nt.KmerSet.from_table(table)
        with nt.KmerGraph(s) as g:
            u = g.unitigs()
            seq, n_bytes, offsets, n_records = g.unitig_batch()
            assert 1 < u.n_unitigs < len(keys) and n_records == u.n_unitigs
            assert int(u.unitig_rows[:, 2].sum().item()) == int(counts.sum())
            torch.cuda.synchronize()
            again.count_device(seq, n_bytes, nt.PRE_NORMALIZE)
            ctx.synchronize()
        keys2, counts2 = again.items()
        assert np.array_equal(keys2, keys) and np.array_equal(counts2, np.ones(len(keys), dtype=np.uint64))


@pytest.mark.parametrize("min_count", [1, 2])
def test_the_unitigs_example_writes_the_models_fasta(ctx, tmp_path, min_count):
    """examples/unitigs on a FASTA file: the records are the model's unitigs of the table's entries with count >= min_count, with their
    lengths, summed counts and the cycle mark in the headers."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "unitigs")
    assert os.path.exists(exe), "build() compiles examples/unitigs"
    rng = np.random.default_rng(0xFA57A)
    k = 21
    genome = DM.random_sequence(rng, 1200)
    plasmid = DM.random_sequence(rng, 90)
    reads = [genome[at: at + 120] for at in rng.integers(0, len(genome) - 120, 80)] + [plasmid + plasmid[: k - 1]] * 3
    reads[5] = reads[5][:60] + "N" + reads[5][61:]
    path = tmp_path / "reads.fa"
    path.write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    with nt.KmerTable(k, nt.PATH_BYTES_CANONICAL, 1 << 15, ctx) as table:
        table.count_records([r.encode() for r in reads], nt.PRE_NORMALIZE)
        keys, counts = table.items(min_count)
    m = DM.Graph(keys, counts, k)
    assert m.n_unitigs > 1 and any(int(r[3]) & 1 for r in m.unitig_rows), "the plasmid is an isolated cycle"
    r = subprocess.run([exe, "-k", str(k), "-m", str(min_count), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * m.n_unitigs
    for u, (row, s) in enumerate(zip(m.unitig_rows, m.spelled)):
        assert lines[2 * u] == f">{u} LN:i:{len(s)} KC:i:{int(row[2])} circular:{int(row[3]) & 1}" and lines[2 * u + 1] == s, u
    assert f"{len(keys)} k-mers, {m.n_unitigs} unitigs, {m.n_bases} bases" in r.stderr
    assert subprocess.run([exe, "-k", "20", str(path)], capture_output=True).returncode == 2


def test_more_unitigs_than_the_first_capacity(ctx):
    """KmerGraph.unitigs starts from room for n / 4 unitigs: 5 000 k-mers that share nothing are 5 000 unitigs, and the call is made again
    with what the first one asked for."""
    rng = np.random.default_rng(0x150)
    keys = DM.keys_of([DM.random_sequence(rng, 31) for _ in range(5000)], 31)
    m, _ = hold(ctx, 31, keys, DM.counts_for(keys), "isolated k-mers")
    assert m.n_unitigs == len(keys) > 4096 and m.totals()["n_isolated"] == len(keys)
