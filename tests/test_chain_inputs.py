"""The inputs of tests/test_gpu_chain.py (tests/_chain_inputs.py) are not vacuous, shown with the host model alone: the tie is a tie, the
window case changes between h and h - 1, the dropped chain really marks an anchor that a later chain stops at; and each of the eight
wrong libraries the model restates (M.MUTANTS) changes the model's result on the case named for it."""
import numpy as np
import pytest

import _chain_inputs as I
import _chain_model as M


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_every_case_is_a_valid_input():
    cases = list(I.tiny_cases().values()) + [I.strands_case(), I.ties_case(), I.pair_edges_case(), I.run_seams_case(), I.forks_case(), I.marked_case(),
                                             I.long_run_case(), I.many_runs_case(4)[0]] + [I.window_case(b) for b in (1, 2, 65, 513)]
    cases += [I.random_case(s) for s in I.RANDOM_SEEDS] + [c[0] for c in I.k_cases().values()]
    for anchors in cases:
        assert M.verify(anchors) == M.OK
    for p in I.RANDOM_PARAMS + (I.EDGE_PARAMS, I.SEAM_PARAMS, I.MIN_CNT_PARAMS, I.MARKED_PARAMS) + tuple(c[1] for c in I.k_cases().values()):
        assert M.check_params(p) == M.OK


def test_strands_and_references():
    got = M.chain(I.strands_case(), I.DEFAULT)
    assert got.chain_rows[:, 2].tolist() == [1, 0, 2, 5] and got.chain_rows[:, 1].tolist() == [7, 6, 5, 4]
    assert got.read_rows.tolist() == [[18, 3, 18, 105], [4, 1, 4, 60]]


@pytest.mark.parametrize("h", I.WINDOW_H)
def test_the_window_case_changes_between_h_and_h_minus_one(h):
    p = M.Params(I.K, h=h)
    at_h, behind = M.chain(I.window_case(h), p), M.chain(I.window_case(h + 1), p)
    assert at_h.f[-1] == 30 and at_h.p[-1] == 0 and behind.f[-1] == 15 and behind.p[-1] == M.NONE
    assert M.chain(I.window_case(h), p, mutant="window_short").f[-1] == 15
    if h > 1:
        assert M.chain(I.window_case(h), M.Params(I.K, h=h - 1)).f[-1] == 15
    assert (M.chain(I.window_case(h), p, mutant="seam_lane").f[-1] == 15) == (h % 64 == 0)
    assert M.stats(I.window_case(h), p, at_h)["n_runs"] == 1


def test_the_ties_are_ties():
    anchors = I.ties_case()
    got = M.chain(anchors, I.DEFAULT)
    off, ref_rev, rpos, qpos = (a.tolist() for a in anchors)
    scores = []
    for j in (0, 1):
        gain, gap = M.pair(0, rpos[j], qpos[j], rpos[2], qpos[2], I.DEFAULT)
        scores.append(int(got.f[j]) + gain - gap)
    assert scores == [28, 28] and got.p[2] == 1
    assert M.chain(anchors, I.DEFAULT, mutant="tie_smallest").p[2] == 0
    ends = got.chain_rows[:, 0].tolist()
    assert ends == [60, 60] and got.chain_rows[:, 2].tolist() == [0, 2], "equal f at two chain ends: the smaller index is visited first"


def test_pair_edges_lie_on_both_sides():
    got = M.chain(I.pair_edges_case(), I.EDGE_PARAMS)
    for q, (name, (read, follows)) in enumerate(I.pair_edge_reads().items()):
        assert (got.p[2 * q + 1] == 2 * q) == follows and (got.f[2 * q + 1] > I.K) == follows, name
    assert not same(got, M.chain(I.pair_edges_case(), I.EDGE_PARAMS, mutant="bw_lt"))
    assert not same(got, M.chain(I.pair_edges_case(), I.EDGE_PARAMS, mutant="max_dist_lt"))
    # each mutant moves exactly the reads named for its edge
    for mutant, names in (("bw_lt", {"dd = bw"}), ("max_dist_lt", {"dr = max_dist", "dq = max_dist", "reverse dq = max_dist"})):
        wrong = M.chain(I.pair_edges_case(), I.EDGE_PARAMS, mutant=mutant)
        moved = {name for q, name in enumerate(I.pair_edge_reads()) if wrong.f[2 * q + 1] != got.f[2 * q + 1]}
        assert moved == names, mutant
    for k, (anchors, p) in I.k_cases().items():
        r = M.chain(anchors, p)
        assert r.chain_rows.shape[0] >= 1 and int(r.f.max()) > 10 * k and p.k == k


def test_run_seams():
    anchors = I.run_seams_case()
    got = M.chain(anchors, I.SEAM_PARAMS)
    assert got.f.tolist() == [15, 30, 15, 15, 15, 30, 15, 30, 15, 15, 15, 15]
    st = M.stats(anchors, I.SEAM_PARAMS, got)
    assert st["n_runs"] == 1 + 2 + 2 + 2 + 2 and st["longest_run"] == 2
    wrong = M.chain(anchors, I.SEAM_PARAMS, mutant="run_split_ge")
    assert wrong.f.tolist()[:2] == [15, 15] and M.stats(anchors, I.SEAM_PARAMS, wrong, mutant="run_split_ge")["n_runs"] == st["n_runs"] + 3


def test_forks():
    anchors = I.forks_case()
    trace = []
    got = M.chain(anchors, I.DEFAULT, trace=trace)
    (q0, _, main, stop0, score0, kept0), (_, end, branch, stop, score, kept) = [t for t in trace if t[0] == 0]
    assert kept0 and stop0 == M.NONE and len(main) == 10 and score0 == 150
    assert kept and stop in main and len(branch) == 5 and score == int(got.f[end]) - int(got.f[stop]) >= 40, "kept with f[i] - f[t]"
    assert got.chain_rows[1].tolist()[:2] == [score, 5] and got.members[10:15].tolist() == sorted(branch)
    wrong = M.chain(anchors, I.DEFAULT, mutant="stop_not_subtracted")
    assert wrong.chain_rows[1, 0] == got.f[end] != score
    # read 1: the branch of three is dropped by min_score alone
    (_, _, _, _, _, kept_main), (_, _, short, stop1, score1, kept1) = [t for t in trace if t[0] == 1]
    assert kept_main and not kept1 and len(short) == 3 >= I.DEFAULT.min_cnt and stop1 != M.NONE and 0 < score1 < I.DEFAULT.min_score
    assert got.read_rows.tolist() == [[15, 2, 15, 150], [13, 1, 10, 150]]
    # the branch of five under min_cnt = 6: dropped by min_cnt alone
    trace = []
    six = M.chain(anchors, I.MIN_CNT_PARAMS, trace=trace)
    _, _, walk, _, s, kept = [t for t in trace if t[0] == 0][1]
    assert not kept and len(walk) == 5 < 6 and s >= I.MIN_CNT_PARAMS.min_score and six.read_rows[0].tolist() == [15, 1, 10, 150]


def test_a_later_chain_stops_at_an_anchor_a_dropped_chain_marked():
    anchors, p = I.marked_case(), I.MARKED_PARAMS
    trace = []
    got = M.chain(anchors, p, trace=trace)
    (_, _, dropped, stop_d, score_d, kept_d), (_, end, later, stop, score, kept) = trace[:2]
    assert not kept_d and stop_d == M.NONE and len(dropped) == 6 < p.min_cnt and score_d >= p.min_score, "dropped by min_cnt alone"
    assert kept and stop in dropped and len(later) >= p.min_cnt and score == int(got.f[end]) - int(got.f[stop]) >= p.min_score
    assert got.chain_rows.shape[0] == 1 and got.chain_rows[0, :2].tolist() == [score, len(later)]
    wrong = M.chain(anchors, p, mutant="dropped_unused")
    assert wrong.chain_rows[0, :2].tolist() != got.chain_rows[0, :2].tolist()


def test_sizes_and_random_cases_have_what_they_are_for():
    long_run = I.long_run_case()
    got = M.chain(long_run, I.DEFAULT)
    st = M.stats(long_run, I.DEFAULT, got)
    assert st["n_runs"] == 1 and st["longest_run"] == st["n_anchors"] > 4900 and st["n_chains"] >= 1 and int(got.chain_rows[0, 1]) > 1000
    many, step = I.many_runs_case(4)
    got = M.chain(many, I.DEFAULT)
    runs = M.run_lengths(many, I.DEFAULT.max_dist)
    assert step == 4 * M.BLOCKS_PER_CU * 4 and runs.count(1) > 5 * step // 4 and runs.count(3) > 5 * step // 4 and set(runs) == {1, 3}
    assert got.read_rows[:, 1].tolist() == [2] * (many[0].size - 1)
    for seed in I.RANDOM_SEEDS:
        anchors = I.random_case(seed)
        seen = [M.chain(anchors, p) for p in I.RANDOM_PARAMS]
        assert all(r.chain_rows.shape[0] > 50 for r in seen) and not same(seen[0], seen[1]) and not same(seen[0], seen[2])
        assert any(int(r.read_rows[:, 1].max()) >= 3 for r in seen) and (seen[0].read_rows[:, 0] == 0).any()
        assert {0, 1, 2, 3} <= set(seen[0].chain_rows[:, 2].tolist())
        # walks that stop at a used anchor are among them
        trace = []
        M.chain(anchors, I.DEFAULT, trace=trace)
        assert sum(1 for t in trace if t[3] != M.NONE) > 50


@pytest.mark.parametrize("mutant,case", [("tie_smallest", "ties"), ("bw_lt", "pair_edges"), ("max_dist_lt", "pair_edges"), ("window_short", "window 64"),
                                         ("seam_lane", "window 64"), ("run_split_ge", "run_seams"), ("dropped_unused", "marked"),
                                         ("stop_not_subtracted", "forks")])
def test_each_mutant_changes_the_case_named_for_it(mutant, case):
    cases = {"ties": (I.ties_case(), I.DEFAULT), "pair_edges": (I.pair_edges_case(), I.EDGE_PARAMS), "window 64": (I.window_case(64), M.Params(I.K, h=64)),
             "run_seams": (I.run_seams_case(), I.SEAM_PARAMS), "marked": (I.marked_case(), I.MARKED_PARAMS), "forks": (I.forks_case(), I.DEFAULT)}
    anchors, p = cases[case]
    assert mutant in M.MUTANTS and not same(M.chain(anchors, p), M.chain(anchors, p, mutant=mutant))
    assert len(M.MUTANTS) == 8
