"""CPU check of the quality mask and of the speculative kernels' bit-5 watch on masked bytes: tests/emu/quality_watch.cpp compiles the
same source the HIP kernels use (needletail_amd/csrc/ntk_tile.hpp: quality_cut, quality_break16, lower_watch_or, lower_watch16) for the
host, and every (byte, quality) pair at every cutoff 1..255 is checked against a model of QualitySequence::quality_mask (reference
src/sequence.rs:285-296) and of the watch rule: a byte is watched when bit 5 is set and the mask left it alone (bit 7 clear)."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quality_watch") / "quality_watch")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "quality_watch.cpp")])
    out = subprocess.run([exe], check=True, capture_output=True).stdout
    per = 65536 * 2 + 4096 * 2
    assert len(out) == 255 * per
    return np.frombuffer(out, dtype=np.uint8).reshape(255, per)


def test_quality_break_and_masked_watch_on_every_pair(dump):
    i = np.arange(65536, dtype=np.uint32)
    pair = (i * 40503 + 12345) & 0xFFFF   # the program's perm()
    byte, qual = (pair >> 8).astype(np.uint8), (pair & 0xFF).astype(np.uint8)
    assert np.unique(pair).size == 65536
    keep = (np.arange(4096) % 17)[:, None] > np.arange(16)[None, :]
    for cutoff in range(1, 256):
        row = dump[cutoff - 1]
        masked_bits, watch_bits = row[:65536], row[65536:131072]
        line_any, line_keep = row[131072:131072 + 4096], row[131072 + 4096:]
        low = qual < cutoff
        # quality_mask: a masked byte only has to stop being a base - bit 7 set, the rest of the byte as it was
        want_masked = np.where(low, byte | 0x80, byte).astype(np.uint8)
        assert np.array_equal(masked_bits, want_masked), cutoff
        watched = ((byte & 0x20) != 0) & ((byte & 0x80) == 0) & ~low
        assert np.array_equal((watch_bits & 0x20) != 0, watched), cutoff
        lines = watched.reshape(4096, 16)
        assert np.array_equal(line_any.astype(bool), lines.any(axis=1)), cutoff
        assert np.array_equal(line_keep.astype(bool), (lines & keep).any(axis=1)), cutoff
    # the pairs that matter: a lower-case base is watched unless its quality is below the cutoff
    row = dump[53 - 1]
    for b in b"acgtu":
        for q, seen in ((52, False), (53, True), (200, True), (0, False)):
            j = int(np.flatnonzero((byte == b) & (qual == q))[0])
            assert bool(row[65536 + j] & 0x20) == seen, (chr(b), q)
