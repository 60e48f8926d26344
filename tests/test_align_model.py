"""The host model of the alignment library (tests/_align_model.py) held to what does not depend on it: the tie cases as literals, an
unbanded Gotoh written separately, its own score three ways, the band, the columns of a chain - and six wrong restatements of the rule,
each told from the right one by at least one input of tests/_align_inputs.py."""
import itertools
import random

import numpy as np
import pytest

import _align_inputs as I
import _align_model as M

P = M.Params(7)


def codes(s):
    return [int(M.CODE[c]) for c in s]


def text(runs):
    return "".join("%d%s" % (n, M.OPS[op]) for op, n in runs)


def gotoh(ref, qry, p):
    """The best score of a global alignment with affine gaps, no band: three states by column, written from the textbook."""
    n, m, inf = len(ref), len(qry), float("-inf")
    best = {(0, 0, "M"): 0}
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                continue
            at = lambda a, b, s: best.get((a, b, s), inf)   # noqa: E731
            if i and j:
                s = p.a if ref[i - 1] == qry[j - 1] and ref[i - 1] < 4 else -p.b
                best[i, j, "M"] = max(at(i - 1, j - 1, t) for t in "MDI") + s
            if i:
                best[i, j, "D"] = max(at(i - 1, j, "D") - p.e, max(at(i - 1, j, "M"), at(i - 1, j, "I")) - p.q - p.e)
            if j:
                best[i, j, "I"] = max(at(i, j - 1, "I") - p.e, max(at(i, j - 1, "M"), at(i, j - 1, "D")) - p.q - p.e)
    return max(best.get((n, m, t), inf) for t in "MDI")


def test_the_tie_cases_as_literals():
    assert text(M.segment(codes(b"AAAA"), codes(b"AAA"), P).runs) == "1D3="
    assert text(M.segment(codes(b"ACA"), codes(b"AA"), P).runs) == "1=1D1="
    assert text(M.segment(codes(b"AAA"), codes(b"AAAA"), P).runs) == "1I3="
    assert text(M.segment(codes(b"ACGTN"), codes(b"acguN"), P).runs) == "4=1X"


@pytest.mark.parametrize("alphabet", [2, 5])
def test_every_small_segment_against_an_unbanded_gotoh(alphabet):
    """With band_pad >= max(n, m) the score is the unbanded one, it is H[n][m] and it is the score of the runs; the path stays in band;
    fill_fast is fill.  On two codes at the default scores: ALL 126 x 126 = 15 876 pairs of sequences with n, m <= 6.  At two other
    sets of scores (q = 0; a > b, q = 7), and on five codes at all three: a SAMPLE, every sequence (of 90 sampled on five codes)
    against 12 drawn partners."""
    rng = random.Random(alphabet)
    seqs = [list(s) for n in range(1, 7) for s in itertools.product(range(alphabet), repeat=n)]
    assert len(seqs) == (126 if alphabet == 2 else 19530)
    if alphabet == 5:
        seqs = rng.sample(seqs, 90)
    n_pairs = n_all = 0
    for p in (M.Params(7, band_pad=6), M.Params(7, 1, 3, 0, 1, 6), M.Params(7, 5, 2, 7, 1, 64)):
        everything = alphabet == 2 and p == M.Params(7, band_pad=6)
        for ref in seqs:
            for qry in seqs if everything else rng.sample(seqs, 12):
                a, b = M.segment(ref, qry, p, fast=False), M.segment(ref, qry, p, fast=True)
                assert a == b and a.in_band and a.score == M.score_of(a.runs, p) == gotoh(ref, qry, p), (p, ref, qry)
                assert sum(n for op, n in a.runs if op != M.OP_I) == len(ref) and sum(n for op, n in a.runs if op != M.OP_D) == len(qry)
                n_pairs, n_all = n_pairs + 1, n_all + everything
    assert n_all == (15876 if alphabet == 2 else 0) and n_pairs - n_all == (2 if alphabet == 2 else 3) * len(seqs) * 12


def test_the_band_binds_and_every_path_stays_inside():
    rng = random.Random(3)
    narrower = 0
    for _ in range(300):
        n, m = rng.randint(1, 40), rng.randint(1, 40)
        ref, qry = [rng.randrange(4) for _ in range(n)], [rng.randrange(4) for _ in range(m)]
        p = M.Params(7, rng.randint(1, 255), rng.randint(1, 255), rng.choice((0, 255, rng.randint(0, 255))), rng.randint(1, 255), rng.choice((0, 1, 3)))
        s = M.segment(ref, qry, p)
        free = M.segment(ref, qry, p._replace(band_pad=64))
        assert s.in_band and free.in_band and s.score == M.score_of(s.runs, p) <= free.score == gotoh(ref, qry, p)
        narrower += s.score < free.score
    assert narrower > 20


def all_cases():
    """name -> (Input, Params) of every fabricated GPU case."""
    out = dict(I.tiny_cases())
    out.update({name: (inp, p) for name, (inp, p, _) in I.band_cases().items()})
    out.update({"seams": (I.seams_case(), I.DEFAULT), "ties": I.ties_case(), "bases": (I.bases_case(), I.DEFAULT), "max_seg": I.max_seg_case()[:2],
                "strands": (I.strands_case()[0], I.DEFAULT), "selection": (I.selection_case(), I.DEFAULT)})
    return out


def test_columns_add_up_and_the_score_is_the_cigars():
    for name, (inp, p) in all_cases().items():
        want, chains = M.run(inp, p)
        ch = inp.chains
        for s, c in enumerate(inp.sel.tolist()):
            row = want.rows[s].tolist()
            if row[0] == M.TOO_LONG:
                assert row[1:] == [0] * 7 and want.scores[s] == 0 and want.g_offsets[s] == want.g_offsets[s + 1]
                continue
            m = M.members_of(ch, c)
            q = (int(ch.qpos[m[0]]), int(ch.qpos[m[-1]]))
            assert row[2] + row[3] + row[5] == int(ch.rpos[m[-1]]) + p.k - int(ch.rpos[m[0]]), (name, s)
            assert row[2] + row[3] + row[4] == max(q) + p.k - min(q), (name, s)
            words = want.cigar[int(want.g_offsets[s]): int(want.g_offsets[s + 1])].tolist()
            assert all(w >> 4 for w in words) and all(a & 15 != b & 15 for a, b in zip(words, words[1:])), (name, s, "canonical")
            runs = [(w & 15, w >> 4) for w in words]
            assert int(want.scores[s]) == M.score_of(runs, p) and row[1] == len(words) and row[6] == sum(1 for op, _ in runs if op in (M.OP_I, M.OP_D))


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_wrong_restatement_is_told_apart(mutant):
    """extend preferred over open, insertion before deletion, a band one narrower, the reverse strand not complemented, anchors trusted,
    runs not merged across segments: each changes the result of at least one GPU case."""
    told = []
    for name, (inp, p) in all_cases().items():
        right, wrong = M.run(inp, p)[0], M.run(inp, p, mutant)[0]
        if any(not np.array_equal(a, b) for a, b in zip(right, wrong)):
            told.append(name)
    assert told, mutant


def test_groups_and_memory():
    assert M.groups([5, 0, 6, 6, 0, 12, 1], 12) == [(0, 3, 11), (3, 5, 6), (5, 6, 12), (6, 7, 1)]
    assert M.groups([], 12) == [] and M.groups([0, 0], 12) == [(0, 2, 0)]
    assert M.device_bytes() == 0 and M.device_bytes(0) == 8 * 7 + 8 + 8 + 28
    assert M.device_bytes(1) - M.device_bytes(0) == 56 and M.device_bytes(0, n_seg=1) - M.device_bytes(0) == 32
    assert M.device_bytes(0, n_runs=1, n_cigar=1, dir_bytes=1) - M.device_bytes(0) == 9
    assert M.check_params(I.DEFAULT) == M.OK and all(M.check_params(p) == M.ERR_BAD_ARG for p in I.bad_params())
    assert all(M.check_params(p) == M.OK for p in I.edge_params())
