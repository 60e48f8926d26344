"""The inputs of the lower-case watch sweep (test_gpu_lower_watch.py) are not vacuous: turning the swept base to lower case changes the
oracle's n_fwd against the all-upper input on at least a quarter of the swept positions (the raw-byte compare of CanonicalKmers puts lower
case above upper case, reference src/kmer.rs:121-128).  A speculative launch that missed the byte and kept its packed-value result would
then give another result on those positions, not only another redo count.  The oracle alone; no kernel runs here."""
import numpy as np
import pytest

import oracle as O

from _seams import (LOWER_KS, LOWER_TAIL_OFFSETS, WIDE_N, WK_ROW, WK_TILE, WK_WAVE, lower_tail_lengths, lower_watch_input, lower_watch_positions,
                    stride_of, wide_input)

PATH_BYTES_CANONICAL, PRE_NONE = 0, 0   # include/needletail_amd.h


@pytest.mark.parametrize("k", LOWER_KS)
def test_one_lower_case_base_changes_the_oracle(k):
    a = lower_watch_input(k)
    s = stride_of(k)
    assert len(a) == 3 * s - 5 and not any(c & 0x20 for c in a.tobytes() if c != 0x0A) and b"N" in a.tobytes() and b"\n" in a.tobytes()
    upper = O.reduce_records(a.tobytes().split(b"\n"), k, PATH_BYTES_CANONICAL, PRE_NONE)
    positions = [p for p in lower_watch_positions(len(a), (s, 2 * s)) if a[p] in b"ACGT"]
    # every position of both ends and around both seams is there
    assert set(range(48)) | set(range(len(a) - 48, len(a))) | set(range(s - 40, s + 25)) | set(range(2 * s - 40, 2 * s + 25)) <= \
        set(lower_watch_positions(len(a), (s, 2 * s)))
    changed = 0
    for p in positions:
        b = a.copy()
        b[p] |= 0x20
        changed += O.reduce_records(b.tobytes().split(b"\n"), k, PATH_BYTES_CANONICAL, PRE_NONE)["n_fwd"] != upper["n_fwd"]
    assert 4 * changed >= len(positions), (k, changed, len(positions))


def _wide_n_fwd(buf: bytes, k: int) -> int:
    """n_fwd of CanonicalKmers with 33 <= k <= 255 through the oracle's literal iterator (raw bytes, as tests/test_gpu_parity.py reads it)."""
    n = 0
    for r in buf.split(b"\n"):
        pos, flg = O.canonical_kmers_arrays(r, O.reverse_complement(r), k)
        n += len(pos) - int(flg.sum())
    return n


@pytest.mark.parametrize("k", [40, 255])
def test_one_lower_case_base_changes_the_oracle_at_wide_k(k):
    a = wide_input()
    upper = _wide_n_fwd(a.tobytes(), k)
    positions = lower_watch_positions(WIDE_N, (WK_ROW, WK_WAVE, WK_TILE), ends=48, step=WIDE_N)
    changed = 0
    for p in positions:
        b = a.copy()
        b[p] |= 0x20
        changed += _wide_n_fwd(b.tobytes(), k) != upper
    assert 4 * changed >= len(positions), (k, changed, len(positions))


def test_wide_positions_cover_the_seams():
    pos = set(lower_watch_positions(WIDE_N, (WK_ROW, WK_WAVE, WK_TILE), ends=48, step=WIDE_N))
    for S in (WK_ROW, WK_WAVE, WK_TILE):
        assert set(range(S - 40, S + 25)) <= pos
    assert set(range(48)) | set(range(WIDE_N - 48, WIDE_N)) <= pos and len(pos) < 320
    assert not any(c & 0x20 for c in wide_input().tobytes())


@pytest.mark.parametrize("n", [WIDE_N, 3 * 1004 - 5, 3 * 1008 - 5, 17])
def test_tail_lengths_put_the_last_byte_where_they_say(n):
    got = lower_tail_lengths(n)
    assert [off for off, _ in got] == list(LOWER_TAIL_OFFSETS)
    for off, m in got:
        assert n - 16 < m <= n and (m - 1) % 16 == off % 16, (n, off, m)
    # a dword exactly full / one byte more / one byte short of the line / the line full / one byte in a line of its own
    assert sorted(m % 16 for _, m in got) == [0, 1, 4, 5, 6, 15]
