"""tests/_dbg_model.ArrayGraph held to tests/_dbg_model.Graph: the array model that tests/test_gpu_grid_steps.py uses at a million keys
answers what the string model answers on every case the two suites share, on every seventh subset of the 14-key universe, and on paths and
cycles long enough for its walk's order to matter.  The array model is trusted through this file alone."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dbg_model as DM  # noqa: E402


def same(k, keys, counts, name):
    g, a = DM.Graph(keys, counts, k), DM.ArrayGraph(keys, counts, k)
    b = DM.ArrayGraph(keys, counts, k, walk=False)   # the adjacency alone answers the same edges and totals
    assert np.array_equal(b.edges, g.edges) and not hasattr(b, "unitig_rows"), name
    assert a.walk_steps == sum(1 for i in range(g.n) if (i, 0) in g.link or (i, 1) in g.link), name
    assert np.array_equal(a.edges, g.edges), name
    want, got = g.totals(), a.totals()
    for key in DM.TOTALS:
        assert np.array_equal(got[key], want[key]), (name, key, got[key], want[key])
        assert np.array_equal(b.totals()[key], want[key]), (name, key)
    assert (a.n_unitigs, a.n_bases) == (g.n_unitigs, g.n_bases), name
    assert a.kmer_rows.dtype == g.kmer_rows.dtype and np.array_equal(a.kmer_rows, g.kmer_rows), name
    assert a.unitig_rows.dtype == g.unitig_rows.dtype and a.unitig_rows.shape == g.unitig_rows.shape, name
    assert np.array_equal(a.unitig_rows, g.unitig_rows), name
    (text, off), (wtext, woff) = a.batch(), g.batch()
    assert text.dtype == wtext.dtype and off.dtype == woff.dtype
    assert np.array_equal(text, wtext) and np.array_equal(off, woff), name
    return g


def test_the_shared_cases():
    for name, k, keys in list(DM.subset_cases()) + list(DM.sequence_cases()):
        same(k, keys, DM.counts_for(keys), name)


def test_subsets_of_the_universe():
    universe = DM.universe_keys()
    bits = (np.arange(1 << 14)[:, None] >> np.arange(14)[None, :]) & 1 == 1
    cycles = 0
    for mask in list(range(0, 1 << 14, 7)) + [(1 << 14) - 1]:   # every seventh subset, and the whole universe
        keys = universe[bits[mask]]
        g = same(3, keys, DM.counts_for(keys, mask), f"subset {mask:#x}")
        cycles += any(int(r[3]) & 1 for r in g.unitig_rows)
    assert cycles > 15


def test_paths_and_cycles_whose_smaller_end_comes_second():
    """Sequences long enough that a path's ends, a cycle's smallest k-mer and the isolated k-mers between them interleave in key order;
    reverse complements, so that paths are walked from either side; and the kmers_of_codes helper against keys_of."""
    rng = np.random.default_rng(0xA77A)
    for k in (5, 15, 31):
        seqs = [DM.random_sequence(rng, int(L)) for L in rng.integers(k, 4 * k + 40, 60)]
        seqs = [DM.rc(s) if j % 2 else s for j, s in enumerate(seqs)]
        keys = DM.keys_of(seqs, k)
        ring = DM.random_sequence(rng, 200)
        both = np.union1d(keys, DM.keys_of([ring], k, circular=True))
        for name, ks in (("paths", keys), ("paths and a cycle", both)):
            same(k, ks, DM.counts_for(ks), (k, name))
        codes = np.array([DM.CODE[c] for c in seqs[0]])
        assert np.array_equal(np.unique(DM.kmers_of_codes(codes, k)), DM.keys_of(seqs[:1], k))
        assert DM.kmers_of_codes(codes[:k - 1], k).size == 0


def test_the_walk_is_linear():
    """A path of 40 000 k-mers and a cycle of 30 000: the bodies of the walk's loops run once per k-mer (a walk that follows a path again
    from each of its inner k-mers runs them some 10^9 times here)."""
    rng = np.random.default_rng(0x11EA)
    k = 31
    path = rng.integers(0, 4, 40_000 + k - 1)
    ring = rng.integers(0, 4, 30_000)
    keys = np.unique(np.concatenate([DM.kmers_of_codes(path, k), DM.kmers_of_codes(np.concatenate([ring, ring[:k - 1]]), k)]))
    assert keys.size == 70_000
    a = DM.ArrayGraph(keys, np.ones(keys.size, dtype=np.uint64), k)
    assert a.walk_steps == keys.size
    assert a.n_unitigs == 2 and sorted(a.unitig_rows[:, 1].tolist()) == [30_000, 40_000]
    assert sorted((a.unitig_rows[:, 3] & 1).tolist()) == [0, 1] and a.totals()["n_links"] == 2 * (40_000 - 1) + 2 * 30_000
