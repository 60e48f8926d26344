"""A host model of the k-mer sketch (needletail_amd/csrc/ntk_sketch.hip, include/needletail_amd_sketch.h): hash, register index, rank,
the registers of a set of keys, the estimator and the capacity rule, restated in numpy / Python from the header's text.  Independent
of needletail_amd/sketching.py: the tests compare the two, and hold the device's registers bit-exactly to this model applied to the
oracle's k-mers.  Built on tests/_count_model.py's fmix64 (the tables' hash)."""
import math

import numpy as np

import _count_model as CM

P = 14                                  # NTK_SKETCH_P: index bits
M = 1 << P                              # NTK_SKETCH_REGISTERS
RANK_MAX = 64 - P + 1                   # 51: the 50 bits below the index all zero
XOR = 0x9E3779B97F4A7C15                # NTK_SKETCH_XOR
SIGMA = 1.04 / math.sqrt(M)             # the estimator's relative standard error, 0.8125 %
CHUNK = 64 << 20                        # kChunkBases of ntk_sketch.hip: bases materialised per pass (k <= 32)
LANE_RUN, PRIME, THREADS = 64, 64, 1024   # the wide walker's lane geometry and the block size of the sketch's kernels

_U = np.uint64
fmix64 = CM.fmix64


def hash_keys(keys) -> np.ndarray:
    """One 64-bit hash per key: narrow values (a 1-d array), or [hi, lo] rows (an (n, 2) array)."""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.ndim == 2:
        return fmix64(keys[:, 1] ^ fmix64(keys[:, 0]) ^ _U(XOR))
    return fmix64(keys ^ _U(XOR))


def index(h) -> np.ndarray:
    """The register index: the top P bits."""
    return (np.asarray(h, dtype=np.uint64) >> _U(64 - P)).astype(np.int64)


def rank(h) -> np.ndarray:
    """1 + the number of leading zeros of the 50 bits below the index, RANK_MAX when they are all zero: a binary-search count of the
    leading zeros of those bits moved to the top, over a sentinel bit (rank_plain says the same bit by bit; the tests hold them equal)."""
    x = (np.asarray(h, dtype=np.uint64) << _U(P)) | _U(1 << (P - 1))
    lz = np.zeros(x.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        top_clear = (x >> _U(64 - s)) == 0
        lz += np.where(top_clear, s, 0)
        x = np.where(top_clear, x << _U(s), x)
    return (lz + 1).astype(np.uint8)


def rank_plain(h) -> np.ndarray:
    """rank(), one bit at a time (slow; for the tests of rank)."""
    rest = np.asarray(h, dtype=np.uint64) & _U((1 << (64 - P)) - 1)
    r = np.full(rest.shape, RANK_MAX, dtype=np.int64)
    for bit in range(64 - P):           # the highest set bit wins: write from the lowest up
        r = np.where((rest >> _U(bit)) & _U(1) == 1, 64 - P - bit, r)
    return r.astype(np.uint8)


def registers(keys, regs=None) -> np.ndarray:
    """The M registers after these keys (into `regs` if given: the sketch accumulates)."""
    regs = np.zeros(M, dtype=np.uint8) if regs is None else regs
    h = hash_keys(keys)
    if h.size:
        np.maximum.at(regs, index(h), rank(h))
    return regs


def estimate(regs) -> float:
    """The classical estimator with linear counting below 2.5 m, in the summation order the header fixes."""
    regs = np.asarray(regs, dtype=np.uint8)
    assert regs.shape == (M,) and int(regs.max(initial=0)) <= RANK_MAX
    c = [int((regs == r).sum()) for r in range(RANK_MAX + 1)]
    z = 0.0
    for r in range(RANK_MAX, -1, -1):
        z += math.ldexp(float(c[r]), -r)
    e = (0.7213 / (1.0 + 1.079 / M)) * M * M / z
    if e <= 2.5 * M and c[0] > 0:
        e = M * math.log(M / c[0])
    return e


def capacity(e: float, n_windows: int, k: int) -> int:
    """ceil(E (1 + 5 sigma)) + 8, at most n_windows, at most 4^k where that fits a word (k < 32), at least 1."""
    cap = math.ceil(e * (1.0 + 5.0 * 1.04 / math.sqrt(M))) + 8
    cap = min(cap, n_windows)
    if k < 32:
        cap = min(cap, 4 ** k)
    return max(cap, 1)


def evaluate(regs, n_windows: int, k: int) -> dict:
    e = estimate(regs)
    return {"distinct": e, "n_windows": int(n_windows), "capacity": capacity(e, int(n_windows), k),
            "zero_registers": int((np.asarray(regs) == 0).sum())}
