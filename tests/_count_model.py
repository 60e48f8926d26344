"""A small host model of the device count table (needletail_amd/csrc/ntk_count.hip): its hash, home slots, sizing rule, probe bound and
chunk length, restated so the tests can build inputs that land where they choose (a chain of keys with one home slot, a record across a
chunk seam).  Test infrastructure only: the tests never read the table's contents through this model, they only aim with it.

Keys are the packed 2-bit values the table stores (A = 0, C = 1, G = 2, T = 3, first base in the high bits)."""
import numpy as np

M64 = (1 << 64) - 1
EMPTY = M64                         # the one key the table keeps in a side word (TTT...T forward at k = 32)
PROBE_MAX = 4096                    # kProbeMax: slots probed at most (the whole table when it has fewer)
CHUNK = 64 << 20                    # kChunkBases: bases materialised per pass
FMIX_SHIFT = 33
FMIX_MUL = (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53)
FMIX_INV = tuple(pow(m, -1, 1 << 64) for m in FMIX_MUL)

_U = np.uint64


def _mul(x: np.ndarray, m: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return x * _U(m)


def fmix64(x) -> np.ndarray:
    """The murmur3 / splitmix64 finaliser of ntk_count.hip, on uint64 arrays."""
    x = np.asarray(x, dtype=np.uint64).copy()
    s = _U(FMIX_SHIFT)
    x ^= x >> s
    x = _mul(x, FMIX_MUL[0])
    x ^= x >> s
    x = _mul(x, FMIX_MUL[1])
    x ^= x >> s
    return x


def fmix64_inv(x) -> np.ndarray:
    """Inverse of fmix64: x ^= x >> 33 is its own inverse (33 >= 32), and each multiplier has an inverse mod 2^64."""
    x = np.asarray(x, dtype=np.uint64).copy()
    s = _U(FMIX_SHIFT)
    x ^= x >> s
    x = _mul(x, FMIX_INV[1])
    x ^= x >> s
    x = _mul(x, FMIX_INV[0])
    x ^= x >> s
    return x


def home(key, slots: int) -> np.ndarray:
    return fmix64(key) & _U(slots - 1)


def slots_for(capacity: int) -> int:
    """The sizing rule of ntk_kmer_table_create: the smallest power of two >= 2 with capacity <= 0.75 * slots."""
    s = 2
    while capacity * 4 > s * 3:
        s <<= 1
    return s


def probe_bound(slots: int) -> int:
    return min(slots, PROBE_MAX)


def revcomp(x, k: int) -> np.ndarray:
    """Reverse complement of packed k-mers (complement = 3 - code = code ^ 3)."""
    x = ~np.asarray(x, dtype=np.uint64)
    for shift, mask in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        m, s = _U(mask), _U(shift)
        x = ((x >> s) & m) | ((x & m) << s)
    x = (x >> _U(32)) | (x << _U(32))
    return x >> _U(64 - 2 * k)


def keys_with_home(h: int, slots: int, k: int, n: int, canonical: bool = False) -> np.ndarray:
    """n distinct keys below 4^k whose home slot is h (deterministic: the same arguments give the same keys, and a larger n extends
    a smaller n's list).  canonical: only keys with key <= revcomp(key), the values a canonical path emits.  The all-ones key (the side
    word's) is never returned."""
    assert 0 <= h < slots and slots & (slots - 1) == 0 and 1 <= k <= 32
    out, have = [], 0
    if k == 32:   # invert the hash: every slot-sized step of the hash value with low bits h
        j = 0
        while have < n:
            step = max(2 * (n - have), 1024)
            cand = fmix64_inv(np.arange(j, j + step, dtype=np.uint64) * _U(slots) + _U(h))
            j += step
            keep = cand != _U(EMPTY)
            if canonical:
                keep &= cand <= revcomp(cand, k)
            out.append(cand[keep])
            have += int(keep.sum())
    else:         # search consecutive candidates
        top, lo, block = 1 << (2 * k), 0, 1 << 22
        while have < n:
            assert lo < top, f"fewer than {n} keys below 4^{k} with home {h} of {slots} slots"
            cand = np.arange(lo, min(lo + block, top), dtype=np.uint64)
            lo += block
            keep = home(cand, slots) == _U(h)
            if canonical:
                keep &= cand <= revcomp(cand, k)
            out.append(cand[keep])
            have += int(keep.sum())
    return np.concatenate(out)[:n]


def render(keys, k: int) -> np.ndarray:
    """keys -> an array [n, k] of base letters."""
    keys = np.asarray(keys, dtype=np.uint64)
    shifts = (2 * np.arange(k - 1, -1, -1)).astype(np.uint64)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[((keys[:, None] >> shifts[None, :]) & _U(3)).astype(np.intp)]


def records_for(keys, counts, k: int, seed: int = 0) -> bytes:
    """A packed batch holding key i counts[i] times, each occurrence a record of exactly k bases and its break byte: one window per
    record, so the batch emits exactly this multiset of keys.  The records are shuffled (seeded), so equal keys meet in one wave."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), keys.shape)
    rep = np.repeat(keys, counts)
    np.random.default_rng(seed).shuffle(rep)
    out = np.full((rep.size, k + 1), ord("\n"), dtype=np.uint8)
    if rep.size:
        out[:, :k] = render(rep, k)
    return out.tobytes()
