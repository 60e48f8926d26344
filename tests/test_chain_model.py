"""The host model of the chain library (tests/_chain_model.py) against the issue's fixtures and against the definition: on every anchor
set of up to 7 anchors over a small grid, f[i] is the best score over all explicitly enumerated predecessor paths inside the window."""
import itertools

import numpy as np

import _chain_inputs as I
import _chain_model as M


def test_the_five_fixtures():
    results = []
    for anchors, f in I.fixtures():
        got = M.chain(anchors, I.DEFAULT)
        assert got.f.tolist() == f
        results.append(got)
    for got in (results[0], results[4]):     # forward and reverse spacing 20: one chain of score 150 over all ten anchors
        assert got.chain_rows.shape == (1, 8) and got.chain_rows[0, :2].tolist() == [150, 10] and got.members.tolist() == list(range(10))
        assert got.p.tolist() == [M.NONE] + list(range(9)) and got.read_rows.tolist() == [[10, 1, 10, 150]]
    assert results[0].chain_rows[0].tolist() == [150, 10, 0, 100, 50, 280, 230, 0]
    assert results[4].chain_rows[0].tolist() == [150, 10, 1, 100, 500, 280, 320, 0]
    assert results[1].f[-1] == 78 and results[1].chain_rows[0, :2].tolist() == [78, 10]
    assert results[2].p.tolist() == [M.NONE, 0] and results[2].chain_rows.shape == (0, 8)      # 28 < min_score
    assert results[3].p.tolist() == [M.NONE, M.NONE, 1], "a true tie, taken by the larger index"


def test_gap_cost_is_minimap2s_in_integers():
    assert [M.ilog2(v) for v in (1, 2, 3, 4, 7, 8, (1 << 31) - 1)] == [0, 1, 1, 2, 2, 3, 30]
    assert M.gap_cost(0, 15) == 0 and M.gap_cost(1, 15) == 0 and M.gap_cost(10, 15) == 2 and M.gap_cost(500, 15) == 75 + 4
    assert M.gap_cost((1 << 31) - 1, 255) == (((1 << 31) - 1) * 255 * 41 >> 12) + 15 < 1 << 34


def _best_path_scores(read, p):
    """f by the definition: the best score over every chain of predecessors that ends at i, every step inside the window."""
    n = len(read)
    best = [p.k] * n

    def extend(i, score):
        best[i] = max(best[i], score)
        for nxt in range(i + 1, min(n, i + p.h + 1)):
            if read[nxt][0] != read[i][0]:
                continue
            step = M.pair(read[i][0] & 1, read[i][1], read[i][2], read[nxt][1], read[nxt][2], p)
            if step is not None:
                # no max(k, .) on the way: a path that falls below k at an anchor is beaten by the path that starts there
                extend(nxt, score + step[0] - step[1])

    for start in range(n):
        extend(start, p.k)
    return best


def test_every_small_anchor_set_against_enumerated_paths():
    """Every set of up to 7 anchors of a grid of 12 - 3 rpos x 3 qpos forward and one reverse diagonal of 3 - under every window 1..3 and
    parameters at whose edges the grid's distances lie (dr, dq in 4, 16, 20; dd in 0, 4, 12, 16)."""
    grid = sorted([(0, r, q) for r in (10, 14, 30) for q in (5, 9, 25)] + [(1, 10, 25), (1, 14, 9), (1, 30, 5)])
    subsets = [s for n in range(1, 8) for s in itertools.combinations(range(len(grid)), n)]
    checked = chained = 0
    for h in (1, 2, 3):
        p = M.Params(3, max_dist=20, bw=4, h=h, min_score=4, min_cnt=2)
        for s in sorted(subsets):
            read = [grid[i] for i in s]
            f, pred = M.recurrence(M.one_read(read), p)
            assert f == _best_path_scores(read, p), (h, read)
            for i, j in enumerate(pred):
                if j != M.NONE:
                    step = M.pair(read[i][0] & 1, read[j][1], read[j][2], read[i][1], read[i][2], p)
                    assert 0 < i - j <= h and step is not None and f[i] == f[j] + step[0] - step[1] > p.k
                    chained += 1
                else:
                    assert f[i] == p.k
            checked += 1
    assert checked == 3 * 3301 and chained > 3000


def test_the_memory_arithmetic():
    assert M.device_bytes() == 0 and M.device_bytes(0) == 8 * M.CTR_WORDS + 8 + 8 + 4 + 16
    assert M.device_bytes(1) - M.device_bytes(0) == 24 + 16 and M.device_bytes(0, n_anchors=1) - M.device_bytes(0) == 8 + 25
    assert M.device_bytes(0, n_runs=1) - M.device_bytes(0) == 4 and M.device_bytes(0, n_chains=1) - M.device_bytes(0) == 40
    assert M.device_bytes(0, n_members=1) - M.device_bytes(0) == 4


def test_verify_and_params():
    assert M.verify(I.strands_case()) == M.OK and all(M.verify(a) == M.OK for a in I.tiny_cases().values())
    for what, anchors, status in I.refused_cases():
        assert M.verify(anchors) == status, what
    assert M.check_params(I.DEFAULT) == M.OK and M.check_params(M.Params(255, (1 << 31) - 1, (1 << 31) - 1, 512, (1 << 32) - 1, (1 << 32) - 1)) == M.OK
    assert M.check_params(M.Params(1, 1, 0, 1, 1, 1)) == M.OK
    assert all(M.check_params(p) == M.ERR_BAD_ARG for p in I.bad_params()) and len(I.bad_params()) == 11
