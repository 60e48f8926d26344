"""A small host model of the wide count table (needletail_amd/csrc/ntk_wide_count.hip, k = 33..63): its key split, hash, home slots,
probe bound and count-kernel lane geometry, restated so the tests can build inputs that land where they choose (hundreds of keys that
share one key word and one home slot, records across lane-run seams).  Test infrastructure only: the tests never read the table's
contents through this model, they only aim with it.  Built on tests/_count_model.py's fmix64 and its inverse.

A key is two u64 words (hi, lo): hi = the first k - 32 bases, lo = the last 32 (A = 0, C = 1, G = 2, T = 3, first base in the high
bits), the 2k-bit value hi * 2^64 + lo."""
import numpy as np

import _count_model as CM

M64 = CM.M64
EMPTY = CM.EMPTY
PROBE_MAX = 4096                    # kProbeMax
LANE_RUN = 64                       # kLaneRun: window ends per lane of the count kernel
PRIME = 64                          # kPrime: bytes a lane reads before its first end
THREADS = 256                       # kThreads: lanes per block
K_MIN, K_MAX = 33, 63

_U = np.uint64
fmix64, fmix64_inv, slots_for, probe_bound = CM.fmix64, CM.fmix64_inv, CM.slots_for, CM.probe_bound


def home(hi, lo, slots: int) -> np.ndarray:
    """The table's home slot: fmix64(lo ^ fmix64(hi)) & (slots - 1)."""
    return (fmix64(np.asarray(lo, dtype=np.uint64) ^ fmix64(hi))) & _U(slots - 1)


def split(v: int, k: int):
    """A 2k-bit value (Python int) -> (hi, lo)."""
    return v >> 64, v & M64


def join(hi: int, lo: int) -> int:
    return (int(hi) << 64) | int(lo)


def revcomp(hi, lo, k: int):
    """Reverse complement of keys given as word arrays: the 128-bit reverse complement of (hi, lo), shifted down to 2k bits."""
    top, bottom = CM.revcomp(lo, 32), CM.revcomp(hi, 32)
    s = _U(128 - 2 * k)
    return top >> s, (bottom >> s) | (top << _U(64 - (128 - 2 * k)))


def is_canonical(hi, lo, k: int) -> np.ndarray:
    """key <= revcomp(key) as 2k-bit values (the value the byte path keeps after normalize)."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    rh, rl = revcomp(hi, lo, k)
    return (hi < rh) | ((hi == rh) & (lo <= rl))


def canonical(hi, lo, k: int):
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    rh, rl = revcomp(hi, lo, k)
    keep = (hi < rh) | ((hi == rh) & (lo <= rl))
    return np.where(keep, hi, rh), np.where(keep, lo, rl)


def keys_sharing_hi(h: int, slots: int, k: int, hi: int, n: int):
    """n distinct canonical keys (hi, lo) with this hi word and home slot h: lo = fmix64_inv(j * slots + h) ^ fmix64(hi)."""
    assert 0 <= h < slots and slots & (slots - 1) == 0 and hi < (1 << (2 * k - 64))
    out, have, j = [], 0, 0
    fh = fmix64(np.array([hi], dtype=np.uint64))[0]
    while have < n:
        step = max(4 * (n - have), 1024)
        lo = fmix64_inv(np.arange(j, j + step, dtype=np.uint64) * _U(slots) + _U(h)) ^ fh
        j += step
        keep = is_canonical(np.full(lo.size, hi, dtype=np.uint64), lo, k)
        out.append(lo[keep])
        have += int(keep.sum())
    lo = np.concatenate(out)[:n]
    return np.full(n, hi, dtype=np.uint64), lo


def keys_sharing_lo(h: int, slots: int, k: int, lo: int, n: int):
    """n distinct canonical keys (hi, lo) with this lo word and home slot h: fmix64(hi) = lo ^ fmix64_inv(j * slots + h), inverted,
    and only the hi words that fit in 2k - 64 bits kept (about one in four at k = 63)."""
    assert 0 <= h < slots and slots & (slots - 1) == 0 and k >= 62, "a hi word fits for one candidate in 4^(64 - k)"
    out, have, j = [], 0, 0
    top = _U(2 * k - 64)
    while have < n:
        step = max(64 * (n - have), 4096)
        hi = fmix64_inv(fmix64_inv(np.arange(j, j + step, dtype=np.uint64) * _U(slots) + _U(h)) ^ _U(lo))
        j += step
        keep = (hi >> top) == 0
        hi = hi[keep]
        keep = is_canonical(hi, np.full(hi.size, lo, dtype=np.uint64), k)
        out.append(hi[keep])
        have += int(keep.sum())
    hi = np.concatenate(out)[:n]
    return hi, np.full(n, lo, dtype=np.uint64)


def render(hi, lo, k: int) -> np.ndarray:
    """keys -> an array [n, k] of base letters."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    sh_hi = (2 * np.arange(k - 33, -1, -1)).astype(np.uint64)
    sh_lo = (2 * np.arange(31, -1, -1)).astype(np.uint64)
    codes = np.concatenate([(hi[:, None] >> sh_hi[None, :]) & _U(3), (lo[:, None] >> sh_lo[None, :]) & _U(3)], axis=1)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[codes.astype(np.intp)]


def records_for(hi, lo, counts, k: int, seed: int = 0) -> bytes:
    """A packed batch holding key i counts[i] times, each occurrence a record of exactly k bases and its break byte, shuffled (seeded),
    so equal keys and keys with one home slot meet in one wave.  Each occurrence is written on a random strand: the table keys both
    strands alike."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), hi.shape)
    idx = np.repeat(np.arange(hi.size), counts)
    rng = np.random.default_rng(seed)
    rng.shuffle(idx)
    rh, rl = revcomp(hi, lo, k)
    flip = rng.random(idx.size) < 0.5
    h = np.where(flip, rh[idx], hi[idx])
    l_ = np.where(flip, rl[idx], lo[idx])
    out = np.full((idx.size, k + 1), ord("\n"), dtype=np.uint8)
    if idx.size:
        out[:, :k] = render(h, l_, k)
    return out.tobytes()
