"""The inputs of the minimizer seam sweeps (tests/_seams.py min_seam_inputs) test the tie rule: on every palindrome case a plain numpy model
of "the minimizer of every window" that takes the leftmost of equal canonical values gives the oracle's counters, and the same model taking
the rightmost gives other counters on at least nine cases in ten - so a scan that resolves a tie the wrong way across a seam (an import from
the previous tile that loses its place in the order) cannot pass the sweeps of test_minimizer_seams_emu.py and test_gpu_minimizer_seams.py.
A condition on the inputs: where a sweep falls short, its seed or its A prefix changes, not the bar."""
import pytest

import oracle as O

from _seams import (TWO_PASS_PAIRS, map_threads, min_input_sets, min_seam_inputs, minimizer_model, owner_tiles, tie_distances,
                    two_pass_inputs)

SETS = [(k, w, s, None) for k, w, s, _ in min_input_sets() if tie_distances(k, w)] + [(k, w, 992, "two_pass_only") for k, w in TWO_PASS_PAIRS]


def rightmost_share(k, w, stride, kind):
    """(tie cases, [cases on which the rightmost model differs from the oracle, per tie rule], kinds of tile ownership met); asserts the
    leftmost model equal to the oracle on every case."""
    cases = two_pass_inputs(k, w) if kind else min_seam_inputs(k, w, stride)
    ties = [(tag, buf) for tag, buf in cases if tag[0] == "tie"]
    differ = []
    for tie_rc in (True, False):
        wants = map_threads(lambda c: O.minimizers_reduce(c[1], k, w, accept_u=tie_rc, tie_rc=tie_rc), ties)
        n = 0
        for (tag, buf), want in zip(ties, wants):
            got = (want["n_total"], want["n_fwd"], want["n_rc"])
            assert minimizer_model(buf, k, w, tie_rc) == got, (k, w, stride, tag, tie_rc)
            n += minimizer_model(buf, k, w, tie_rc, rightmost=True) != got
        differ.append(n)
    return len(ties), differ, {owner_tiles(tag, k, w) for tag, _ in ties}


@pytest.mark.parametrize("k,w,stride,kind", SETS)
def test_tie_cases_tell_leftmost_from_rightmost(k, w, stride, kind):
    n, differ, owners = rightmost_share(k, w, stride, kind)
    assert n > 0
    for d in differ:
        assert 10 * d >= 9 * n, (k, w, stride, d, n)
    # the two tied k-mers end in different tiles; both end in the earlier tile and a window over them ends in the later one (its halo holds both)
    assert "split" in owners
    if min(tie_distances(k, w)) < w - 1:
        assert "halo" in owners


def test_the_model_knows_a_tie():
    """The model on an input small enough to check by hand: AAC GTT is one canonical 3-mer on opposite strands, two positions apart."""
    buf = b"AACGTT"   # 3-mers AAC ACG CGT GTT: canonical AAC ACG ACG AAC
    assert minimizer_model(buf, 3, 4, True) == (1, 1, 0) and minimizer_model(buf, 3, 4, True, rightmost=True) == (1, 0, 1)
    want = O.minimizers_reduce(buf, 3, 4, accept_u=True, tie_rc=True)
    assert (want["n_total"], want["n_fwd"], want["n_rc"]) == (1, 1, 0)
    assert minimizer_model(b"AACNGTT", 3, 4, True) == (0, 0, 0)
