"""Inputs added for the survivors of the mutation audit (tools/mutation_audit.py, profiles/mutation_audit/README.md): each is the smallest
input that tells a small wrong edit of csrc/ntk_tile.hpp from the right logic where no input of tests/_seams.py did.  Shared by the CPU
emulator tests (test_mutant_inputs_emu.py) and the device tests (test_gpu_minimizer_seams.py, test_gpu_wide_seams.py, test_gpu_build_matrix.py;
test_gpu_lower_watch.py takes _seams.lower_tail_lengths).

- tail_input: the last 16-byte line holds 15 input bytes and the byte behind them is a BASE ('A', TAIL_FILL).  Every earlier input ended
  in padding that is no base (0xAA on the emulator) or at a length that left more than one byte of padding in the last line, so "the line is
  whole from 15 bytes on" (keep >= 15 for keep >= 16 in lane_tile, minimizer_invalid16, wk_stage_slot) emitted nothing extra.  For lane_tile
  the extra window shows only in the materialised valid16 word (tail_plane_words): a reduction over the planes stops at byte n.
- palindrome_kmer_inputs: a k-mer that IS its own reverse complement (k even), ending mid-tile and on both sides of a seam.  The sweeps'
  palindromes have k + d bases: two k-mers with one canonical value on opposite strands, none equal to its own reverse complement, and random
  text holds such a k-mer of 18 or more bases with probability 4^-9 per position; the tie rule of the two-word compare of lane_tile
  (byte path: a tie reports the reverse complement) was never asked."""
import numpy as np

from _seams import ACGT, revcomp

TAIL_FILL = b"A"          # behind byte n: a base the scans must not take
SCAN_STRIDE = 992         # scan_kernel (lane_tile): kTileStride
WIDE_TILE = 4096          # wide_canonical_reduce_kernel: kWkTile


def tail_length(at_least: int) -> int:
    """The smallest n >= at_least whose last 16-byte line holds 15 bytes."""
    return at_least + (15 - at_least) % 16


def tail_input(first_tile: int, seed: int = 0) -> bytes:
    """Random upper-case ACGT: one tile of `first_tile` bytes, two 16-byte lines and a last line of 15 bytes (the tail tile is the second;
    no break anywhere, so the window over the last bytes and the padding byte would be emitted if the padding counted)."""
    n = tail_length(first_tile + 32)
    assert n % 16 == 15 and n > first_tile
    return ACGT[np.random.default_rng(0x7A11 + first_tile + seed).integers(0, 4, n)].tobytes()


def pack16(bits) -> np.ndarray:
    """A plane of one flag per position as the scans write it: 16 positions per word, position p in bit 15 - p % 16 of word p // 16."""
    b = np.asarray(bits, dtype=bool)
    b = np.concatenate([b, np.zeros(-len(b) % 16, dtype=bool)]).reshape(-1, 16)
    return (b.astype(np.uint32) << (15 - np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint16)


def tail_plane_words(buf: bytes, k: int, canon: bool, tie_rc: bool):
    """(valid16, rc16) words of upper-case ACGT `buf` from the oracle's literal iterators, each k-mer at its window-end byte; tie_rc: the byte
    path (CanonicalKmers), else the bit paths (BitNuclKmer).  Positions from len(buf) on, the last word's low bits, are clear."""
    import oracle as O
    if tie_rc:
        pos, flg = O.canonical_kmers_arrays(buf, O.reverse_complement(buf), k)
    else:
        pos, _, flg = O.bit_kmers_arrays(buf, k, canon)
    valid, rcf = np.zeros(len(buf), dtype=bool), np.zeros(len(buf), dtype=bool)
    ends = pos.astype(np.int64) + k - 1
    valid[ends] = True
    rcf[ends] = flg.astype(bool)
    return pack16(valid), pack16(rcf)


def self_palindrome(k: int, rng) -> bytes:
    """k bases (k even) equal to their own reverse complement: u + rc(u)."""
    assert k % 2 == 0
    u = ACGT[rng.integers(0, 4, k // 2)].tobytes()
    s = u + revcomp(u)
    assert revcomp(s) == s
    return s


def palindrome_kmer_inputs(k: int, stride: int = SCAN_STRIDE, seed: int = 0):
    """Random upper-case ACGT of stride + 200 bytes with one self-palindrome of k bases written over it so that its k-mer ENDS at byte e:
    mid-tile at two lane offsets, on the last byte before the seam, on the first two behind it, and on both sides of the next lane boundary.
    Yields (e, bytes)."""
    rng = np.random.default_rng(0x9A11 + 64 * k + stride + seed)
    base = ACGT[rng.integers(0, 4, stride + 200)].copy()
    pal = np.frombuffer(self_palindrome(k, rng), dtype=np.uint8)
    for e in (300, 309, stride - 1, stride, stride + 1, stride + 15, stride + 16):
        a = base.copy()
        a[e - k + 1: e + 1] = pal
        yield e, a.tobytes()
