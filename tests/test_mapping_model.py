"""The host model of the mapping library (tests/_mapping_model.py) held to hand-computed fixtures, to a sequential
mm_set_parent-style loop written separately from the model's link / root form, and to the float formula of the mapping quality."""
import itertools
import math

import numpy as np

import _mapping_inputs as I
import _mapping_model as M

K = I.K


def test_hand_computed_fixtures():
    """A [0,100) 300, B [40,140) 200, C [98,180) 100 at the defaults.  B and A share 60 of min 100: overlap.  C and A share 2 of min 82: no.
    C and B share 42 of 82 (42000 > 41000): overlap, so link[C] = B and parent[C] = parent[B] = A."""
    r = M.run(I.roots_case(), I.DEFAULT)
    a, b, c = r.rows[:3].tolist()
    assert a[:9] == [0, 100, 1000, 1100, 0, 300, 2, 30, 100] and b[:4] == [40, 140, 1000, 1100] and c[:2] == [98, 180]
    assert [x[M.W["parent"]] for x in (a, b, c)] == [0, 0, 0] and [x[M.W["flags"]] for x in (a, b, c)] == [1, 0, 0]
    assert (a[M.W["subsc"]], a[M.W["n_sub"]]) == (200, 2) and [x[M.W["rank"]] for x in (a, b, c)] == [0, 1, 2]
    # pen = min(100, 20) = 20; d = 100; lg8(300) = 2106; t = 40 * 20 * 100 * 2106 // 300 = 561600; raw = (561600 * 45426 >> 16) // 25600 = 15;
    # lg8(3) = 405: (405 * 771 + 32768) >> 16 = 5; mapq = 10
    assert M.lg8(300) == 2106 and M.lg8(3) == 405 and a[M.W["mapq"]] == 10 and r.read_rows[0].tolist() == [3, 1, 0, 10]
    assert r.out.tolist()[:1] == [0] and r.out_offsets.tolist() == [0, 1, 3] and r.order.tolist() == [0, 1, 2, 3, 4, 5]
    # the second read: C [40,150) overlaps A and B, both primary; its link is the lowest rank, A
    assert r.rows[3:, M.W["parent"]].tolist() == [3, 4, 3] and r.rows[3:, M.W["flags"]].tolist() == [1, 1, 0]
    # the boundary: 40 * 1000 == 500 * 80 is no overlap, 41 * 1000 is one
    r = M.run(I.boundary_case(), I.DEFAULT)
    assert r.rows[:, M.W["flags"]].tolist() == [1, 1, 1, 0] and r.rows[3, M.W["parent"]] == 2
    assert [M.run(I.boundary_case(), p).read_rows[:, 1].tolist() for p in I.MASK_PARAMS] == [[1, 1], [2, 2], [1, 1], [2, 2]]
    # ties: the first of equal scores is the primary; two equal children
    r = M.run(I.ties_case(), I.DEFAULT)
    assert r.rows[0, [M.W["subsc"], M.W["n_sub"], M.W["flags"], M.W["mapq"]]].tolist() == [100, 2, 1, 0] and r.order[:3].tolist() == [0, 1, 2]
    assert r.order[3:].tolist() == [4, 5, 3, 6] and r.rows[[3, 4, 5, 6], M.W["parent"]].tolist() == [3, 4, 4, 3]
    # secondaries: exactly 800 per mille is kept, one below is dropped; 5 of 7 eligible, the ineligible between them not counted
    r = M.run(I.secondaries_case(), I.DEFAULT)
    assert r.rows[:6, M.W["flags"]].tolist() == [1, 2, 0, 1, 2, 0] and r.rows[6:, M.W["flags"]].tolist() == [1, 2, 2, 0, 0, 1, 2, 2, 2, 0, 0]
    assert r.rows[6, M.W["n_sub"]] == 4 and r.rows[11, M.W["n_sub"]] == 5 and r.out[r.out_offsets[1]:].tolist() == [6, 7, 8, 11, 12, 13, 14]
    assert [M.run(I.secondaries_case(), p).read_rows[1, 2] for p in I.BEST_N_PARAMS] == [0, 1, 5, 7, 5, 0]
    # spans: k = 15 and the steps (14,14) (15,15) (16,16) (12,19) (20,13): mlen = 15 + 14 + 15 + 15 + 12 + 13, blen = 15 + 14 + 15 + 16 + 19 + 20
    ch = M.batch_of([[I.member_chain(100, 1, list(I.STEPS[:5]))]])
    row = M.run(ch, I.DEFAULT).rows[0].tolist()
    assert row[:9] == [20, 20 + 77 + 15, 500, 500 + 77 + 15, 1, 100, 6, 84, 99]
    assert ch.qpos[0] == 97 and ch.qpos[-1] == 20, "on the reverse strand the first member has the largest qpos"


def _sequential_parents(iv, mask_level_pm):
    """mm_set_parent's loop with a hard mask level: chain i takes the parent of the first chain before it that it overlaps."""
    parent = []
    for i, (qs, qe) in enumerate(iv):
        mine = i
        for j in range(i):
            lo, hi = max(qs, iv[j][0]), min(qe, iv[j][1])
            if hi > lo and (hi - lo) * 1000 > mask_level_pm * min(qe - qs, iv[j][1] - iv[j][0]):
                mine = parent[j]
                break
        parent.append(mine)
    return parent


def test_parent_is_the_sequential_loops_on_every_small_set():
    """Every set of up to 5 intervals over a 10-point grid, ranked as enumerated (1.4 M sets) and, up to 4, in the reverse order; every
    ordered tuple of up to 3, repeats included, at three mask levels; 40 000 random ordered tuples of 4 and 5 at five mask levels; then
    sets with distinct and tied scores through the whole model."""
    grid = [(a, b) for a in range(10) for b in range(a + 1, 10)]
    n = 0
    for size in range(1, 6):
        for iv in itertools.combinations(grid, size):
            assert M.parents(list(iv), 500) == _sequential_parents(iv, 500)
            if size < 5:
                assert M.parents(list(iv[::-1]), 500) == _sequential_parents(iv[::-1], 500)
            n += 1
    assert n == sum(math.comb(45, s) for s in range(1, 6))
    for size in range(1, 4):
        for iv in itertools.product(grid, repeat=size):
            for mask in (0, 500, 1000):
                assert M.parents(list(iv), mask) == _sequential_parents(iv, mask)
    rng = np.random.default_rng(3)
    for size in (4, 5):
        for _ in range(20000):
            iv = [grid[int(i)] for i in rng.integers(0, len(grid), size=size)]
            mask = int(rng.choice([0, 250, 500, 750, 1000]))
            assert M.parents(iv, mask) == _sequential_parents(iv, mask)
    # through run(): intervals scaled by K so that every chain has its seed's length, scores distinct and tied
    for _ in range(300):
        size = int(rng.integers(1, 6))
        iv = [grid[int(i)] for i in rng.integers(0, len(grid), size=size)]
        scores = [int(s) for s in rng.integers(50, 53, size=size)]
        ch = M.batch_of([[M.span(s, K * a, K * b, K) for s, (a, b) in zip(scores, iv)]])
        r = M.run(ch, I.DEFAULT)
        by_rank = sorted(range(size), key=lambda c: (-scores[c], c))
        assert r.order.tolist() == by_rank
        want = _sequential_parents([(K * iv[c][0], K * iv[c][1]) for c in by_rank], 500)
        assert [int(r.rows[c, M.W["parent"]]) for c in by_rank] == [by_rank[p] for p in want]


def test_lg8_is_the_floor_of_256_log2():
    """Exactly: 2^L <= v^256 < 2^(L + 1), for every v below 2^17, every power of two and its neighbours, and 20 000 random 32-bit v."""
    rng = np.random.default_rng(5)
    vs = set(range(1, 1 << 17)) | {int(x) for x in rng.integers(1, 1 << 32, size=20000)}
    for e in range(32):
        vs |= {x for x in ((1 << e) - 1, 1 << e, (1 << e) + 1) if 1 <= x < 1 << 32}
    for v in vs:
        L = M.lg8(v)
        big = v ** 256
        assert big >> L == 1, v


def _float_mapq(score, cnt, subsc, n_sub, min_chain_score):
    """minimap2 2.17's chain-only formula with uniq_ratio 1, in floating point: a real number."""
    pen = min(min(score, 100), 10 * min(cnt, 10)) / 100
    sub = max(subsc, min_chain_score)
    return (40 * pen * (1 - sub / score) * math.log(score) if score > sub else 0.0) - 4.343 * math.log(n_sub + 1)


def test_mapq_is_the_float_formula_to_within_one():
    """The integer mapq against the floor of the float formula, clamped to 0..60: at most 1 apart.  The integer form floors its first
    term A (lg8 floors 256 log2: A loses less than 0.1 before its own floor) and rounds its second term B to the nearest integer, so it
    lies in (A - B - 1.61, A - B + 0.51]: an integer there is within 1 of floor(A - B)."""
    rng = np.random.default_rng(9)
    worst = 0
    for _ in range(100000):
        score = int(rng.integers(1, 1 << int(rng.integers(1, 32))))
        cnt = int(rng.integers(1, 30))
        subsc = int(rng.integers(0, score + 1)) if rng.integers(0, 2) else 0
        n_sub = int(rng.integers(0, 1 << int(rng.integers(1, 17))))
        got, want = M.mapq(score, cnt, subsc, n_sub, 40), max(0, min(60, math.floor(_float_mapq(score, cnt, subsc, n_sub, 40))))
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1, (score, cnt, subsc, n_sub, got, want)
    assert worst <= 1
    assert M.mapq(300, 12, 0, 0, 40) == 60 and M.mapq(100, 10, 100, 1, 40) == 0 and 0 < M.mapq(60, 5, 0, 0, 40) < 60


def test_refusals_of_the_model_and_device_bytes():
    for what, ch, status in I.refused_cases():
        assert M.verify(ch, K) == status, what
    for what, ch in I.accepted_edges().items():
        assert M.verify(ch, K) == M.OK, what
        M.run(ch, I.DEFAULT)
    assert all(M.check_params(p) == M.ERR_BAD_ARG for p in I.bad_params()) and M.check_params(I.DEFAULT) == M.OK
    assert M.check_params(M.Params(255, 1000, 1000, 65535, (1 << 32) - 1)) == M.OK and M.check_params(M.Params(1, 0, 0, 0, 1)) == M.OK
    assert M.device_bytes() == 0 and M.device_bytes(0) == 48 + 8 + 4
    assert M.device_bytes(0, n_chains=1) - M.device_bytes(0) == 92 and M.device_bytes(1) - M.device_bytes(0) == 28
