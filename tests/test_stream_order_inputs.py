"""The cases of tests/test_gpu_stream_order.py are not vacuous: computed with the host models alone, the answer for the true input differs
from the answer for the decoy, for the clobber (the all-'N' / all-zero fill), and for a chain with a stage lost, skipped or misplaced - in
every field and array the GPU test compares.  One fixed seed for the file (`_stream_order.SEED`)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_order as S  # noqa: E402

TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_true_answer_differs_from_every_other(name):
    case = S.CASES[name]
    truth = case.truth()
    assert truth, name
    for other, answer in case.others().items():
        S.assert_answers_differ(truth, answer, (name, other))
    if name not in ("mhset_compare", "chain"):   # (host inputs only; the chain's stages are held below)
        assert case.others(), name


@pytest.mark.parametrize("skip", list(S.CHAIN_AFTER))
def test_every_stage_of_the_chain_shows_in_what_follows_it(skip):
    truth, other = S.chain_answer(), S.chain_answer(skip)
    for key in S.CHAIN_AFTER[skip]:
        assert S.differs(truth[key], other[key]), (skip, key)


def test_the_batches_are_what_the_cases_say():
    for k, lower, repeat in ((21, False, False), (31, False, False), (27, False, False), (21, True, False), (47, True, True)):
        t, d = S.batches(k, lower, repeat)
        assert len(t.records) == len(d.records) == S.N_RECORDS and t.n == d.n and 5000 <= t.n <= 8000
        assert sorted(set(map(len, t.records))) == sorted({0, 1, k - 1, k, 150, 700})
        assert [len(r) for r in t.records] == [len(r) for r in d.records] and t.buf != d.buf
        assert np.array_equal(t.offsets, d.offsets) and int(t.offsets[-1]) == t.n
        assert b"N" in t.buf and b"N" not in d.buf
        assert (any(c & 0x20 for c in t.buf.replace(b"\n", b"")) == lower) and not any(c & 0x20 for c in d.buf.replace(b"\n", b""))
        assert (t.qual < S.CUTOFF).any() and (d.qual < S.CUTOFF).any() and not np.array_equal(t.qual, d.qual)
        assert sum(1 for i, r in enumerate(t.records) if len(r) == 150 and r in t.records[:i]) == 1, "one exact duplicate read"
        if repeat:   # the inverted repeat is longer than k and equals its own reverse complement
            r = next(r for r in t.records if len(r) == 700)
            ir = r[20:20 + 2 * (k + 8)]
            assert len(ir) > k and ir == ir[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def test_the_decoy_offsets_and_the_clobbers_are_valid_input():
    t, _ = S.batches(21)
    zero = np.zeros_like(t.offsets)
    assert S.records_of(t.buf, zero) == [b""] * S.N_RECORDS and S.records_of(t.buf, t.offsets) == t.records
    assert all(np.array_equal(a, b) for a, b in zip(S.quals_of(t.qual, t.offsets), t.quals))
    assert set(S.clobber_bytes(16)) == {ord("N")}
    assert S.POISON not in b"ACGTacgtUuNn\n" and S.POISON_WORD < 1 << 63


def test_the_redo_routes_are_the_speculative_pairs():
    """What test_reduce_device asserts from NTK_ACC_REDONE: on input that was not normalised the call is the speculative pair."""
    import _builds as B
    for route, (k, path, pre, lower, repeat) in S.REDUCE_ROUTES.items():
        for quality in (False, True):
            got = B.kernels(B.Call("reduce", k, 0, path, pre, quality, 0))
            if lower:
                first = B.wide_reduce(False, quality) if k > 32 else B.scan2(k, True, False, quality)
                assert got == (first, B.bytes_reduce(k > 32, quality)), (route, got)
            else:
                assert len(got) == 1, (route, got)


def test_every_case_is_used_by_the_gpu_file():
    text = open(os.path.join(TESTS, "test_gpu_stream_order.py")).read()
    for name in S.CASES:   # the case's name, or its stem in front of a parameter, is a string of the GPU file
        stem = name.split("-")[0]
        assert re.search(rf'"{stem}[-"{{]', text), name
    for stem in set(re.findall(r'S\.CASES\[f?"(\w+)', text)):
        assert any(name.split("-")[0] == stem for name in S.CASES), stem
    assert len(S.CASES) >= 40
