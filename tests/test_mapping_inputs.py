"""No GPU case of tests/test_gpu_mapping.py is vacuous: every fabricated case of tests/_mapping_inputs.py does what its name says, every
wrong library restated in tests/_mapping_model.py differs from the right one on the case named for it, and every random case holds
non-primaries, kept and dropped secondaries and mapping qualities of 0, of 60 and in between."""
import numpy as np
import pytest

import _mapping_inputs as I
import _mapping_model as M

F = M.W


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_wrong_library_fails_the_case_named_for_it(mutant):
    make, params = I.CASES[I.MUTANT_CASE[mutant]]
    ch = make()
    assert M.verify(ch, I.K) == M.OK
    assert _differs(M.run(ch, I.DEFAULT), M.run(ch, I.DEFAULT, mutant)) and I.DEFAULT in params, mutant
    assert set(I.MUTANT_CASE) == set(M.MUTANTS)


def test_seam_reads_have_their_only_overlap_where_they_say():
    ch = I.seams_case()
    r = M.run(ch, I.DEFAULT)
    assert [n for n, _ in I.seam_reads()] == r.read_rows[:, 0].tolist() and set(I.SEAM_SIZES) == {n for n, _ in I.seam_reads()}
    ats = set()
    for q, (n, at) in enumerate(I.seam_reads()):
        lo = int(ch.c_offsets[q])
        assert r.order[lo: lo + n].tolist() == list(range(lo, lo + n)), "the chains are fabricated in rank order"
        if at is None:
            continue
        iv = [(int(r.rows[c, 0]), int(r.rows[c, 1])) for c in range(lo, lo + n)]
        assert M.links(iv, 500) == [None] * (n - 1) + [at] and r.rows[lo + n - 1, F["parent"]] == lo + at
        assert r.read_rows[q].tolist()[:3] == [n, n - 1, 1]
        ats.add((at, n - 1 - at))
    assert {at for at, _ in ats} >= {0, 63, 64} and any(back == 64 for _, back in ats), "rank 0, 63 and 64, and exactly one strip back"
    big = M.run(I.big_reads_case(), I.DEFAULT)
    assert all(n > M.LDS_CHAINS for n in big.read_rows[:, 0].tolist()) and big.read_rows[:, 2].tolist() == [1] * len(I.BIG_READS)
    assert any(at % 64 == 0 and at >= M.LDS_CHAINS for _, at in I.BIG_READS) and any(n - 1 - at == 64 for n, at in I.BIG_READS)


def test_spans_and_mapq_cases_cover_their_edges():
    ch = I.spans_case()
    r = M.run(ch, I.DEFAULT)
    assert sorted(set(r.rows[:, F["cnt"]].tolist())) == [1, 2, 64, 65, 1000] and set(r.rows[:, F["ref_rev"]].tolist()) == {1, 4, 7}
    st = {s for c in range(ch.chain_rows.shape[0]) for s in M.steps(ch, c)}
    for lo, hi in ((1, I.K - 1), (I.K, I.K), (I.K + 1, 1000)):
        assert any(lo <= dr <= hi for dr, _ in st) and any(lo <= dq <= hi for _, dq in st) and any(lo <= min(s) <= hi for s in st)
    rev = [c for c in range(ch.chain_rows.shape[0]) if ch.chain_rows[c, 2] & 1 and r.rows[c, F["cnt"]] > 1]
    assert rev and all(ch.qpos[int(ch.m_offsets[c])] == ch.qpos[int(ch.m_offsets[c]): int(ch.m_offsets[c + 1])].max() for c in rev)
    assert np.all(r.rows[:, F["mlen"]] <= r.rows[:, F["blen"]]) and np.any(r.rows[:, F["mlen"]] < r.rows[:, F["blen"]])
    reads = I.mapq_reads()
    assert {9, 10, 11} <= {c for _, c, _ in reads} and {99, 100, 101} <= {s for s, _, _ in reads}
    assert any(subs and max(subs) < 40 for _, _, subs in reads) and any(subs and max(subs) > 40 for _, _, subs in reads)
    for p in I.CASES["mapq"][1]:
        r = M.run(I.mapq_case(), p)
        top = r.read_rows[:, 3].tolist()
        assert 0 in top and 60 in top and len(set(top)) > (6 if p == I.DEFAULT else 2), "both clamps and values between them"
    r = M.run(I.mapq_case(), I.DEFAULT)
    top = dict(zip(reads, r.read_rows[:, 3].tolist()))
    five = [top[(s, c, (90,))] for s, c in ((99, 9), (100, 10), (101, 11), (99, 11), (101, 9))]
    assert all(0 < v < 60 for v in five) and len(set(five)) >= 3, "cnt and score on both sides of their caps change an unclamped mapq"
    assert top[(200, 20, (39,))] == top[(200, 20, (40,))] == top[(200, 20, (30,))] > top[(200, 20, (41,))] - 5 and top[(200, 20, (150,))] < top[(200, 20, (41,))]


def test_tiny_refused_and_many_reads_cases():
    assert [c.chain_rows.shape[0] for c in I.tiny_cases().values()] == [0, 0, 1, 1, 6]
    assert [c.c_offsets.size - 1 for c in I.tiny_cases().values()] == [0, 2, 4, 1, 2]
    statuses = [s for _, _, s in I.refused_cases()]
    assert statuses.count(M.ERR_UNSUPPORTED) == 3 and statuses.count(M.ERR_BAD_ARG) >= 10
    for n_cu in (1, 256):
        ch, step = I.many_reads_case(n_cu)
        counts = np.diff(ch.c_offsets.astype(np.int64))
        assert ch.c_offsets.size - 1 == step + step // 4 > step and set(counts.tolist()) == {1, 2, 3}
    r = M.run(I.many_reads_case(2)[0], I.DEFAULT)
    assert set(r.read_rows[:, 1].tolist()) == {1, 2} and set(r.read_rows[:, 2].tolist()) == {0, 1}


@pytest.mark.parametrize("seed", I.RANDOM_SEEDS)
def test_random_cases_hold_every_kind_of_chain(seed):
    ch = I.random_case(seed)
    assert M.verify(ch, I.K) == M.OK and ch.c_offsets[0] > 0 and ch.c_offsets[-1] < ch.chain_rows.shape[0]
    for p in I.RANDOM_PARAMS:
        r = M.run(ch, p)
        lo, hi = int(ch.c_offsets[0]), int(ch.c_offsets[-1])
        flags = r.rows[lo:hi, F["flags"]]
        primary = flags & 1 == 1
        assert np.any(flags == 0) and np.any(flags == 2) and np.any(primary), "dropped and kept secondaries and primaries"
        q = r.rows[lo:hi, F["mapq"]][primary]
        assert np.any(q == 0) and np.any(q == 60) and np.any((q > 0) & (q < 60))
        assert np.all(r.rows[lo:hi, F["mapq"]][~primary] == 0) and not r.rows[:lo].any() and not r.rows[hi:].any()
        assert np.any(r.rows[lo:hi, F["n_sub"]] > 1) and len(set(r.rows[lo:hi, F["ref_rev"]].tolist())) == 8
        scores = r.rows[lo:hi, F["score"]]
        assert len(set(scores.tolist())) < scores.size, "tied scores"
    for mutant in M.MUTANTS:
        if mutant not in ("seam_lane", "mask_ge"):   # (no read of 65 chains; the boundary needs its exact ratio)
            assert _differs(M.run(ch, I.DEFAULT), M.run(ch, I.DEFAULT, mutant)), mutant
