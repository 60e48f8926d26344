"""The chunk cut of csrc/ntk_compat_plan.hpp, which every batched Sequence-trait call walks (run_banked of csrc/ntk_api.hip), compiled here
with g++ and swept against a restatement: the chunks tile the records in order, none is empty, a chunk of more than one record fits the
budget, and every chunk is maximal.  Also the constants tests/_compat_scale.py aims at."""
import re

import numpy as np
import pytest

import _compat_plan as P
import _compat_scale as S

CHUNKS = (64, 97, 4096, 16 * S.MI)
PER_RECORD = (0, 1)   # records uploaded as they lie / packed with a break byte behind each


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("compat_plan"))


def test_the_header_is_plain_cpp_and_states_the_tests_constants(plan_lib):
    text = open(P.COMPAT_PLAN_HPP).read()
    assert not re.search(r"hip/|__device__|__global__|__host__", text), "the plan header is plain C++"
    assert plan_lib.plan_default_chunk() == S.DEFAULT_CHUNK_BYTES == CHUNKS[-1]
    assert plan_lib.plan_min_chunk() == S.MIN_CHUNK_BYTES == CHUNKS[0]
    assert plan_lib.plan_banks() == S.BANKS
    assert plan_lib.plan_long_record() == S.LONG_RECORD


def model_cut(offsets, chunk, per_record):
    """The restatement: r1 is the largest index with offsets[r1] - offsets[r0] + per_record * (r1 - r0) <= chunk, and r0 + 1 at the least."""
    offs = [int(o) for o in offsets]
    n, out, r0 = len(offs) - 1, [], 0
    while r0 < n:
        cost = lambda r1: offs[r1] - offs[r0] + per_record * (r1 - r0)
        r1 = max([r for r in range(r0 + 1, n + 1) if cost(r) <= chunk], default=r0 + 1)
        out.append((r0, r1, cost(r1)))
        r0 = r1
    return out


def _offsets(lengths, first=0):
    return np.concatenate(([first], first + np.cumsum(np.asarray(lengths, dtype=np.uint64)))).astype(np.uint64)


def length_lists(chunk):
    """name -> record lengths, aimed at `chunk`."""
    rng = np.random.default_rng([0xC47, chunk])
    big = chunk + 37
    part = max(chunk // 3, 1)
    lists = {
        "one record": [5],
        "one empty record": [0],
        "one oversize record": [big],
        "empty records": [0] * 70,                                    # (more of them than a chunk of 64 takes with a break byte each)
        "oversize first": [big, 3, 0, 4],
        "oversize last": [3, 0, 4, big],
        "oversize in the middle": [3, 4, big, 0, 5],
        "empties around an oversize record": [0, big, 0, 0],
        "runs of empties": [0, 0, 0, 7, 0, 0, big, 0, 0, 0, 0, 2, 0],
        "ragged": [int(x) for x in rng.integers(0, min(chunk, 400) + 1, 200)],
    }
    # sums that land on chunk - 1, chunk and chunk + 1, counted with and without the break bytes, twice in a row
    for per_record in PER_RECORD:
        for d in (-1, 0, 1):
            last = chunk + d - 2 * part - 3 * per_record
            if last >= 0:
                lists[f"sum at chunk {d:+d} (per_record {per_record})"] = [part, part, last] * 2 + [1]
    return lists


@pytest.mark.parametrize("per_record", PER_RECORD)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_cut_tiles_the_records_with_maximal_chunks(plan_lib, chunk, per_record):
    cases = [(name, _offsets(lens, first)) for name, lens in length_lists(chunk).items() for first in (0, 5)]
    if chunk <= 4096:   # the batches of tests/test_gpu_parity.py: hundreds of chunks at the forced sizes
        cases += [(name, _offsets([len(r) for r in recs])) for name, recs in
                  [("parity items", S.parity_item_records()), ("parity bit planes", S.parity_bit_plane_records()),
                   ("empties around oversize", S.empties_around_oversize())] + [(f"{len(b)} records", b) for b in S.bank_count_batches()]]
    for name, offs in cases:
        n = len(offs) - 1
        got = P.walk(plan_lib, offs, chunk, per_record)
        assert got == model_cut(offs, chunk, per_record), name
        at = 0
        for r0, r1, nbytes in got:
            assert r0 == at and r1 > r0, (name, r0)                                       # in order, none empty
            cost = int(offs[r1] - offs[r0]) + per_record * (r1 - r0)
            assert nbytes == cost and (r1 == r0 + 1 or cost <= chunk), (name, r0)         # more than one record: within the budget
            assert r1 == n or int(offs[r1 + 1] - offs[r0]) + per_record * (r1 + 1 - r0) > chunk, (name, r0)   # maximal
            at = r1
        assert at == n, name


def test_the_forced_cuts_of_the_parity_batches(plan_lib):
    """What tests/test_gpu_parity.py counts on when it sets the chunk option to 64: chunks of empty records on both sides of the oversize
    record, and one record per chunk - on every face - for the batches around the bank count."""
    offs = _offsets([len(r) for r in S.empties_around_oversize()])
    for chunk in S.PIPELINE_CHUNK_OPTIONS:
        for per_record in PER_RECORD:
            assert [(r0, r1) for r0, r1, _ in P.walk(plan_lib, offs, chunk, per_record)] == [(0, 1), (1, 2), (2, 4)], (chunk, per_record)
    sizes = [len(b) for b in S.bank_count_batches()]
    assert sizes == list(S.PIPELINE_BATCH_SIZES) and min(sizes) < S.BANKS and S.BANKS in sizes and S.BANKS + 1 in sizes and max(sizes) > 2 * S.BANKS
    for batch in S.bank_count_batches():
        assert {len(r) for r in batch} == {S.PIPELINE_RECORD_LEN}
        offs = _offsets([len(r) for r in batch])
        for per_record in PER_RECORD:
            assert [(r0, r1) for r0, r1, _ in P.walk(plan_lib, offs, 64, per_record)] == [(i, i + 1) for i in range(len(batch))]
