"""The host model of the seed-index library (tests/_seed_index_model.py) against a brute-force restatement of the definition: all
pairs (seed, occurrence), filtered and sorted by Python's tuple order, on lists small enough for it."""
from collections import Counter

import numpy as np
import pytest

import _seed_index_inputs as I
import _seed_index_model as M


def entries(lst):
    """[(record, pos, value, strand)] of the entries that belong to a record."""
    off, pos, values, info = lst
    return [(r, int(pos[i]), int(values[i]), int(info[i]) & 1) for r in range(off.size - 1) for i in range(int(off[r]), int(off[r + 1]))]


def brute(refs, reads, max_occ):
    """(anchors per read as sorted (ref_rev, rpos, qpos) tuples, rows) from the definition alone."""
    occurrences = entries(refs)
    occ = Counter(v for _, _, v, _ in occurrences)
    n_reads = reads[0].size - 1
    anchors, rows = [[] for _ in range(n_reads)], np.zeros((n_reads, 4), dtype=np.uint32)
    for q, qpos, value, qstrand in entries(reads):
        rows[q, 0] += 1
        if value not in occ:
            rows[q, 3] += 1
        elif max_occ != 0 and occ[value] > max_occ:
            rows[q, 2] += 1
        else:
            rows[q, 1] += 1
            anchors[q] += [(r << 1 | (strand ^ qstrand), rpos, qpos) for r, rpos, v, strand in occurrences if v == value]
    return [sorted(a) for a in anchors], rows


def as_tuples(result):
    a_offsets, ref, rev, rpos, qpos, _ = result
    flat = list(zip((ref.astype(np.int64) << 1 | rev).tolist(), rpos.tolist(), qpos.tolist()))
    return [flat[int(a_offsets[q]): int(a_offsets[q + 1])] for q in range(a_offsets.size - 1)]


def hold(refs, reads, max_occ):
    index = M.Index(refs)
    status, result, total = M.match(index, reads, max_occ)
    want, rows = brute(refs, reads, max_occ)
    assert status == M.OK and as_tuples(result) == want and np.array_equal(result[5], rows)
    assert total == sum(len(a) for a in want) == int(result[0][-1]) and int(result[0][0]) == 0
    assert np.array_equal(rows[:, 0], rows[:, 1:].sum(axis=1))
    return index, result


@pytest.mark.parametrize("max_occ", range(5))
@pytest.mark.parametrize("front,back", [(0, 0), (3, 2)])
def test_small_case_matches_the_definition(max_occ, front, back):
    refs, reads = I.small_case(front, back)
    index, result = hold(refs, reads, max_occ)
    plain = M.match(M.Index(I.small_case()[0]), I.small_case()[1], max_occ)[1]
    for g, w in zip(result, plain):   # entries outside every record change nothing
        assert np.array_equal(g, w)


@pytest.mark.parametrize("seed", I.RANDOM_SEEDS)
def test_random_lists_match_the_definition(seed):
    refs, reads = I.random_case(seed)
    for max_occ in (0, 1, I.RANDOM_MAX_OCC, 100):
        hold(refs, reads, max_occ)


def test_the_index_is_the_definition():
    refs, _ = I.small_case(2, 1)
    index = M.Index(refs)
    occurrences = sorted((v, r, pos, s) for r, pos, v, s in entries(refs))
    assert index.keys.tolist() == sorted({v for v, _, _, _ in occurrences}) and index.n_entries == len(occurrences) == 20
    assert index.ref.tolist() == [r << 1 | s for _, r, _, s in occurrences] and index.rpos.tolist() == [p for _, _, p, _ in occurrences]
    assert [int(index.occ[index.keys.tolist().index(I.A[c])]) for c in range(1, 6)] == [1, 2, 3, 4, 5] and index.max_occ == 5
    assert index.spectrum(4).tolist() == [0, 6, 1, 3] and index.spectrum(8).tolist() == [0, 6, 1, 1, 1, 1, 0, 0]
    assert M.stats(index) == {"n_refs": 3, "n_entries": 20, "n_keys": 10, "max_occ": 5, "n_reads": 0, "n_seeds": 0, "n_anchors": 0}
    # 10 keys: the cut at 10 % may drop one key, at 20 % two, and at 0 none
    assert [index.occ_cutoff(f) for f in (0, 99_999, 100_000, 200_000, 399_999, 400_000, 1_000_000)] == [5, 5, 4, 3, 2, 1, 1]
    assert M.Index(I.empty_list(3)).occ_cutoff(200) == 1


def test_empty_inputs():
    refs, reads = I.small_case()
    for r, q in ((I.empty_list(0), reads), (I.empty_list(3), reads), (refs, I.empty_list(0)), (refs, I.empty_list(4))):
        index, result = hold(r, q, 2)
        assert result[1].size == 0 and result[0].size == q[0].size
    assert M.Index(I.empty_list(2)).n_keys == 0 and M.Index(I.empty_list(2)).max_occ == 0


def test_capacity_and_refusals():
    refs, reads = I.small_case()
    index = M.Index(refs)
    _, full, total = M.match(index, reads, 0)
    status, result, needed = M.match(index, reads, 0, max_anchors=total - 1)
    assert status == M.ERR_CAPACITY and needed == total and result[1].size == 0 and not result[0].any() and np.array_equal(result[5], full[5])
    assert M.match(index, reads, 0, max_anchors=total)[0] == M.OK
    assert [M.verify(lst) for _, lst, _ in I.refused_lists()] == [status for _, _, status in I.refused_lists()]
    assert [s for _, _, s in I.refused_lists()] == [M.ERR_BAD_ARG, M.ERR_BAD_ARG, M.ERR_UNSUPPORTED, M.ERR_BAD_ARG]
    assert M.verify(I.small_case(3, 2)[1]) == M.OK, "a pos of 2^32 outside every record is not looked at"


def test_device_bytes_is_the_headers_statement():
    assert M.index_bytes(0, 0) == 4 and M.index_bytes(10, 20) == 12 * 10 + 4 + 8 * 20
    assert M.device_bytes(10, 20) == M.index_bytes(10, 20) + 32 + 28 * 20
    assert M.device_bytes(10, 20, build_work=False) == M.index_bytes(10, 20) + 32
    assert M.device_bytes(10, 20, n_reads=8, n_seeds=33, n_anchors=100, n_bins=7) == \
        M.index_bytes(10, 20) + 32 + 28 * 20 + 7 * 8 + 16 * 33 + 12 + 16 * 8 + 12 * 214 + 24 * 8 + 8
    assert M.device_bytes(1, 1, n_reads=1, n_seeds=1, n_anchors=4000, long_anchors=3000) - M.device_bytes(1, 1, n_reads=1, n_seeds=1, n_anchors=4000) == 72_000
    assert M.long_anchors([0, 5, 5 + M.SORT_TILE, 6 + 2 * M.SORT_TILE, 9 + 5 * M.SORT_TILE]) == 4 * M.SORT_TILE + 4
