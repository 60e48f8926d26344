"""The inputs of the GPU tests of the seed-index library (tests/_seed_index_inputs.py) are not vacuous: counts asserted from the model,
and each of the four wrong libraries the model can restate (the rightmost search, `>=` in the max_occ rule, a tie of the sort left
in another order, the last read left unsorted) gives another result on at least one of them."""
import numpy as np
import pytest

import _minimizer_list_model as MM
import _seed_index_inputs as I
import _seed_index_model as M

N_CU = 256   # what the sizes are worked out for here; the GPU tests take the device's


def shapes(refs, reads, max_occ):
    """What a case holds under max_occ, from the model: a dict of counts and flags."""
    index = M.Index(refs)
    status, (a_offsets, ref, rev, rpos, qpos, rows), total = M.match(index, reads, max_occ)
    assert status == M.OK
    per_read = [slice(int(a_offsets[q]), int(a_offsets[q + 1])) for q in range(rows.shape[0])]
    both = ties = False
    for s in per_read:
        on = {}
        for r, v in zip(ref[s].tolist(), rev[s].tolist()):
            on.setdefault(r, set()).add(v)
        both |= any(len(v) == 2 for v in on.values())
        pairs = list(zip(ref[s].tolist(), rev[s].tolist(), rpos[s].tolist()))
        ties |= len(set(pairs)) < len(pairs)
    return dict(hit=int(rows[:, 1].sum()), repetitive=int(rows[:, 2].sum()), absent=int(rows[:, 3].sum()), total=total,
                at_max=bool((index.occ == max_occ).any()), above_max=bool((index.occ == max_occ + 1).any()),
                no_seeds=bool((rows[:, 0] == 0).any()), no_anchors=bool(((rows[:, 0] > 0) & (rows[:, 1] == 0)).any()),
                both_strands=both, ties=ties, most=max(s.stop - s.start for s in per_read) if per_read else 0)


def differs(refs, reads, max_occ, mutant, index=None, right=None):
    index = index or M.Index(refs)
    right, wrong = right or M.match(index, reads, max_occ), M.match(index, reads, max_occ, mutant=mutant)
    return right[2] != wrong[2] or any(not np.array_equal(a, b) for a, b in zip(right[1], wrong[1]))


def test_small_case_holds_every_shape():
    refs, reads = I.small_case()
    assert refs[0].size - 1 == 3 and reads[0].size - 1 == 8 and max(np.diff(refs[0].astype(np.int64)).max(), np.diff(reads[0].astype(np.int64)).max()) <= 12
    for max_occ in range(5):
        s = shapes(refs, reads, max_occ)
        assert s["hit"] and s["absent"] and s["no_seeds"] and s["no_anchors"] and s["both_strands"] and s["ties"], (max_occ, s)
        assert (s["repetitive"] > 0) == (max_occ != 0) and s["above_max"] and s["at_max"] == (max_occ != 0)
    # seeds per value in the reads: A1 6, A2 5, A3 5, A4 5, A5 4 and two fillers, each times its occ
    assert [shapes(refs, reads, m)["total"] for m in range(5)] == [6 + 10 + 15 + 20 + 20 + 2, 8, 18, 33, 53]
    for mutant in M.MUTANTS:
        assert differs(refs, reads, 2, mutant), mutant
    assert differs(refs, reads, 0, "rightmost") and not differs(refs, reads, 0, "max_occ_ge")


@pytest.mark.parametrize("seed", I.RANDOM_SEEDS)
def test_random_cases_hold_every_shape(seed):
    refs, reads = I.random_case(seed)
    s = shapes(refs, reads, I.RANDOM_MAX_OCC)
    assert s["hit"] and s["repetitive"] and s["absent"] and s["at_max"] and s["above_max"], s
    assert s["no_seeds"] and s["no_anchors"] and s["both_strands"] and s["ties"], s
    for mutant in M.MUTANTS:
        assert differs(refs, reads, I.RANDOM_MAX_OCC, mutant), mutant


@pytest.mark.parametrize("n_anchors", [M.SORT_TILE - 1, M.SORT_TILE, M.SORT_TILE + 1, 3 * M.SORT_TILE + 5])
def test_sort_route_cases_have_exactly_that_many_anchors(n_anchors):
    refs, reads = I.sort_route_case(n_anchors)
    s = shapes(refs, reads, 0)
    assert s["most"] == n_anchors and s["ties"] and s["both_strands"] and s["total"] == n_anchors + 6
    a_offsets = M.match(M.Index(refs), reads, 0)[1][0]
    assert np.diff(a_offsets.astype(np.int64)).tolist() == [2, 0, 1, n_anchors, 1, 0, 2]
    assert differs(refs, reads, 0, "unstable_tie")
    # the fill's order is not the sorted one: the long read alone, left as made, is another result
    only = (reads[0][:5].copy(), reads[1], reads[2], reads[3])
    assert differs(refs, only, 0, "last_read")


def test_balanced_fill_case():
    refs, reads = I.balanced_fill_case(N_CU)
    s = shapes(refs, reads, 0)
    n_reads = reads[0].size - 1
    assert s["most"] == 20_002 and s["total"] == 20_002 + (n_reads - 1) and s["absent"] == 0
    long_read = int(np.argmax(np.diff(reads[0].astype(np.int64))))
    assert long_read > 2.25 * N_CU * M.BLOCKS_PER_CU and n_reads - long_read == 6
    assert shapes(refs, reads, 19_999)["total"] == n_reads + 1 and shapes(refs, reads, 20_000)["total"] == s["total"]


@pytest.mark.parametrize("quarters", [5, 9])
def test_capped_grid_cases_pass_one_step(quarters):
    refs, reads = I.capped_grid_case(N_CU, quarters)
    step = N_CU * M.BLOCKS_PER_CU * M.THREADS
    index = M.Index(refs)
    status, result, total = M.match(index, reads, 1)
    rows = result[5]
    assert index.max_occ == 1 and index.n_keys == index.n_entries > quarters * step // 4 and refs[0].size - 1 == 1000
    assert status == M.OK and total == int(rows[:, 1].sum()) > (quarters - 1) * step // 4
    assert int(rows[:, 3].sum()) > 1000 and int(rows[:, 2].sum()) == 0
    n_reads = reads[0].size - 1
    assert n_reads > 9 * N_CU * M.BLOCKS_PER_CU // 4, "more reads than 2.25 steps of a block per read, and of a wave per read"
    right = (status, result, total)
    assert differs(refs, reads, 1, "rightmost", index, right) and differs(refs, reads, 1, "max_occ_ge", index, right)
    assert (refs[1].nbytes + refs[2].nbytes + refs[3].nbytes) * 2 < 64 << 20


@pytest.mark.parametrize("k,w,order,path", I.END_TO_END)
def test_end_to_end_reads_lie_on_their_diagonals(k, w, order, path):
    """The model's anchors of the cut reads on their own references: every one on the diagonal of its cut, without exception."""
    refs, reads, cuts = I.sequences()
    assert len(refs) == 3 and len(reads) == 60 and sum(c is None for c in cuts) == 10
    assert sum(1 for c in cuts if c and c[2]) >= 20 and sum(1 for c in cuts if c and not c[2]) >= 20
    pre = 2   # NTK_PRE_NORMALIZE
    r_list, q_list = (I.as_seed_list(MM.lists(x, k, w, path, pre, order)) for x in (refs, reads))
    status, result, total = M.match(M.Index(r_list), q_list, 0)
    off, on = I.diagonal_exceptions(result, cuts, k)
    assert status == M.OK and off == [] and on > 400, (off, on)
    rows = result[5]
    assert all(rows[q, 1] >= 5 for q, c in enumerate(cuts) if c), "every cut read is found"
    assert sum(int(rows[q, 1]) for q, c in enumerate(cuts) if c is None) == 0, "no random read is"
    assert set(result[2].tolist()) == {0, 1}
