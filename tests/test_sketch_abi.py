"""CPU-side checks of the sketch library (include/needletail_amd_sketch.h, libneedletail_amd_sketch.so) beyond those every library is held
to (tests/test_consumer_abi.py): the host model (tests/_sketch_model.py) with its constants tied to the kernel source, and the capacity
rule's accuracy sweep."""
import math
import os
import re

import numpy as np
import pytest

import _count_model as CM
import _libraries as L
import _sketch_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_sketch.h")
HIP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_sketch.hip")
CHUNKS = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_chunks.hpp")   # the chunk geometry every library walks
WIDE_HIP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_wide_count.hip")
WALK_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_wide_walk.hpp")
ROW = L.BY_NAME["sketch"]


def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


def test_header_compiles_as_c(tmp_path):
    L.check_header(ROW, tmp_path)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    L.check_no_device(ROW)


# ---- the host model (tests/_sketch_model.py), which the GPU tests hold the registers to ----------------------------------------------

def test_sketch_constants_are_the_models():
    """The GPU tests compare registers bit for bit with tests/_sketch_model.py.  If the sketch's hash, index, rank, chunk length or the
    walker's geometry changes, say so here, on the CPU, rather than as a puzzling register mismatch on the GPU."""
    src, hdr, wide = open(HIP).read(), open(HEADER).read(), open(WIDE_HIP).read()
    assert int(re.search(r"#define NTK_SKETCH_P (\d+)", hdr).group(1)) == S.P
    assert re.search(r"#define NTK_SKETCH_REGISTERS \(1u << NTK_SKETCH_P\)", hdr)
    assert int(re.search(r"#define NTK_SKETCH_MAX_RANK (\d+)", hdr).group(1)) == S.RANK_MAX == 64 - S.P + 1
    assert int(re.search(r"#define NTK_SKETCH_XOR (0x[0-9A-Fa-f]+)ull", hdr).group(1), 16) == S.XOR != 0
    assert int(re.search(r"kXor = (0x[0-9A-Fa-f]+)ull;", src).group(1), 16) == S.XOR
    assert re.search(r"kP = NTK_SKETCH_P, kRegisters = NTK_SKETCH_REGISTERS;", src)
    assert re.search(r"kRankMax = 64 - kP \+ 1;", src)
    assert re.search(r"sketch_hash\(uint64_t key\) \{ return fmix64\(key \^ kXor\); \}", src)
    assert re.search(r"sketch_hash\(uint64_t hi, uint64_t lo\) \{ return fmix64\(lo \^ fmix64\(hi\) \^ kXor\); \}", src)
    assert re.search(r"sketch_slot\(uint64_t h\) \{ return \(uint32_t\)\(h >> \(64 - kP\)\); \}", src)
    assert re.search(r"sketch_rank\(uint64_t h\) \{ return \(uint32_t\)__builtin_clzll\(\(h << kP\) \| \(\(uint64_t\)1 << \(kP - 1\)\)\) \+ 1; \}", src)
    # the tables' hash, defined once, in the shared header
    assert '#include "ntk_consumer.hpp"' in src and not re.search(r"\bfmix64\([^)]*\)\s*\{", src), "fmix64 defined again"
    chunk = re.search(r"kChunkBases = \(uint64_t\)(\d+) << (\d+);", open(CHUNKS).read())
    assert int(chunk.group(1)) << int(chunk.group(2)) == S.CHUNK == CM.CHUNK
    assert not re.search(r"kChunkBases\s*=", src), "the chunk length is ntk_chunks.hpp's alone"
    assert int(re.search(r"kSketchThreads = (\d+);", src).group(1)) == S.THREADS
    # the wide walker (ntk_wide_walk.hpp, which the sketch includes) restates wt_count_kernel's: the same lane geometry, k range and
    # per-byte rules as ntk_wide_count.hip
    assert '#include "ntk_wide_walk.hpp"' in src
    walk = open(WALK_HPP).read()
    for text in (walk, wide):
        assert int(re.search(r"kLaneRun = (\d+);", text).group(1)) == S.LANE_RUN
        assert int(re.search(r"kPrime = (\d+);", text).group(1)) == S.PRIME
        assert re.search(r"kKMax = (\d+);", text).group(1) == "63"
    norm = lambda t: re.sub(r"\s+", " ", t.replace("a.cutoff", "cutoff").replace("a.n_bytes", "n_bytes"))
    for rule in ("const uint32_t l = b | 0x20;", "(l == 'a' || l == 'c' || l == 'g' || l == 't' || l == 'u') && qb >= cutoff &&",
                 "const uint64_t c = ((b >> 1) ^ (b >> 2)) & 3;", "fh = ((fh << 2) | (fl >> 62)) & hi_mask;", "fl = (fl << 2) | c;",
                 "rl = (rl >> 2) | (rh << 62);", "rh = (rh >> 2) | ((3 - c) << rc_shift);", "run = base ? run + 1 : 0;",
                 "const bool fwd = fh < rh || (fh == rh && fl <= rl);"):
        assert rule in norm(walk) and rule in norm(wide), rule


def _int_rank(h):
    rest = h & ((1 << 50) - 1)
    return 51 if rest == 0 else 50 - rest.bit_length() + 1


def test_model_index_and_rank_edges():
    M64 = (1 << 64) - 1
    edges = [0, M64, 1 << 50, (1 << 50) - 1, 1, 1 << 49, M64 << 50 & M64, (1 << 63) | 1, 0x3FFF << 50, (0x2ABC << 50) | (1 << 20)]
    h = np.array(edges, dtype=np.uint64)
    assert [int(v) for v in S.index(h)] == [e >> 50 for e in edges]
    assert [int(v) for v in S.rank(h)] == [_int_rank(e) for e in edges]
    assert int(S.rank(h[:1])[0]) == 51 and int(S.index(h[:1])[0]) == 0                 # h = 0
    assert int(S.rank(h[1:2])[0]) == 1 and int(S.index(h[1:2])[0]) == S.M - 1          # h = ~0
    assert int(S.rank(h[2:3])[0]) == 51 and int(S.index(h[2:3])[0]) == 1               # the low 50 bits all zero
    assert int(S.rank(h[4:5])[0]) == 50                                                # only the lowest bit
    rng = np.random.default_rng(0x51)
    h = rng.integers(0, 1 << 64, 200_000, dtype=np.uint64) >> rng.integers(0, 64, 200_000).astype(np.uint64)
    assert np.array_equal(S.rank(h), S.rank_plain(h))
    assert [int(v) for v in S.rank(h[:200])] == [_int_rank(int(v)) for v in h[:200]]
    assert S.rank(h).max() <= S.RANK_MAX and S.rank(h).min() >= 1


def test_model_hash_is_the_header_text():
    def fmix(x):
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd & CM.M64
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 & CM.M64
        return x ^ (x >> 33)
    rng = np.random.default_rng(0x52)
    keys = rng.integers(0, 1 << 64, 64, dtype=np.uint64)
    keys[0] = 0
    assert [int(v) for v in S.hash_keys(keys)] == [fmix(int(v) ^ S.XOR) for v in keys]
    assert int(S.hash_keys(keys[:1])[0]) != 0, "key 0 (AAA...A) must not hash to 0"
    rows = rng.integers(0, 1 << 62, (64, 2), dtype=np.uint64)
    assert [int(v) for v in S.hash_keys(rows)] == [fmix(int(lo) ^ fmix(int(hi)) ^ S.XOR) for hi, lo in rows]
    regs = S.registers(keys)
    again = S.registers(np.concatenate([keys, keys[::-1]]))
    assert np.array_equal(regs, again) and int((regs != 0).sum()) <= 64
    assert np.array_equal(S.registers(keys[32:], S.registers(keys[:32])), regs)   # accumulating = all at once


def test_estimate_from_registers_equals_the_model():
    from needletail_amd import sketching as K
    assert (K.P, K.REGISTERS, K.MAX_RANK) == (S.P, S.M, S.RANK_MAX) and K.SIGMA == S.SIGMA
    rng = np.random.default_rng(0x53)
    files = [np.zeros(S.M, np.uint8), np.full(S.M, S.RANK_MAX, np.uint8)]
    one = np.zeros(S.M, np.uint8)
    one[777] = 9
    files.append(one)
    for top in (1, 2, 5, 12, 30, S.RANK_MAX):
        files.append(rng.integers(0, top + 1, S.M).astype(np.uint8))
    files.append(S.registers(rng.integers(0, 1 << 64, 300_000, dtype=np.uint64)))
    for regs in files:
        for n_windows, k in ((0, 21), (5, 21), (10 ** 6, 21), (1 << 40, 51), (1 << 40, 3), (1 << 40, 31), (1 << 40, 32)):
            got, want = K.estimate_from_registers(regs, n_windows, k), S.evaluate(regs, n_windows, k)
            assert got == want, (got, want)
    empty = K.estimate_from_registers(files[0], 0, 21)
    assert empty["distinct"] == 0.0 and empty["capacity"] == 1 and empty["zero_registers"] == S.M
    assert K.estimate_from_registers(files[0], 1000, 21)["capacity"] == 8          # ceil(0) + 8
    single = K.estimate_from_registers(one, 1000, 21)
    assert single["distinct"] == S.M * math.log(S.M / (S.M - 1)) and single["capacity"] == 2 + 8 and single["zero_registers"] == S.M - 1
    full = K.estimate_from_registers(files[1], 1 << 62, 32)
    a = 0.7213 / (1 + 1.079 / S.M)
    assert full["distinct"] == pytest.approx(a * S.M * 2.0 ** S.RANK_MAX, rel=1e-12) and full["zero_registers"] == 0
    assert K.estimate_from_registers(files[1], 1 << 62, 3)["capacity"] == 64         # 4^k
    assert K.estimate_from_registers(files[1], 77, 32)["capacity"] == 77             # n_windows
    import needletail_amd as nt
    for bad in (np.zeros(S.M - 1, np.uint8), np.zeros(S.M, np.int32), np.full(S.M, S.RANK_MAX + 1, np.uint8)):
        with pytest.raises(nt.NtkError) as e:
            K.estimate_from_registers(bad, 10, 21)
        assert e.value.status == 2


def test_capacity_rule_accuracy_sweep():
    """The capacity rule on distinct keys `base + i * 2654435761` through the sketch's hash: 6 seeds, the 52 cardinalities
    round(10^(i / 8)) from 10 to 2.4e7.  At every checkpoint n the capacity (unclamped: n_windows huge, k = 32) is never below n - the
    table would drop k-mers for good - and from n = 64 on at most 2 n, one doubling of the table.  The bounds are conditions held
    against the exact n, not measurements.  Worst relative error of the estimate seen here: -1.97 % (seed 0, n = 7 498 942) and
    +3.38 % (seed 4, n = 42 170, where linear counting hands over to the raw estimator); five standard errors are 4.06 %."""
    checks = sorted(set(int(round(10 ** (i / 8))) for i in range(8, 8 * 8 + 1)))
    checks = [c for c in checks if c <= 30_000_000]
    assert len(checks) == 52 and checks[0] == 10 and checks[-1] == 23_713_737
    worst_under = worst_over = 0.0
    for seed in range(6):
        base = np.random.default_rng(1000 + seed).integers(0, 1 << 62, dtype=np.uint64)
        regs, n = np.zeros(S.M, dtype=np.uint8), 0
        for c in checks:
            while n < c:
                take = min(c - n, 4_000_000)
                with np.errstate(over="ignore"):
                    keys = base + np.arange(n, n + take, dtype=np.uint64) * np.uint64(2654435761)
                S.registers(keys, regs)
                n += take
            e = S.estimate(regs)
            cap = S.capacity(e, 1 << 62, 32)
            worst_under, worst_over = min(worst_under, e / n - 1), max(worst_over, e / n - 1 if n >= 64 else 0.0)
            assert cap >= n, (seed, n, e, cap)
            if n >= 64:
                assert cap <= 2 * n, (seed, n, e, cap)
    print(f"sweep: worst under-estimate {worst_under * 100:+.2f} %, worst over-estimate {worst_over * 100:+.2f} %, "
          f"5 sigma = {5 * S.SIGMA * 100:.2f} %")
