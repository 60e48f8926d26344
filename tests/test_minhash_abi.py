"""CPU-side checks of the MinHash library (include/needletail_amd_minhash.h, libneedletail_amd_minhash.so) beyond those every library is
held to (tests/test_consumer_abi.py): the struct fields of the bindings, the constants and the byte walker tied to the sketch's and the
wide table's sources, the host model's (tests/_minhash_model.py) algebra, and ntk_minhash_compare - host code - against the model's set
restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _count_model as CM
import _libraries as L
import _minhash_model as M
import _sketch_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_minhash.h")
SKETCH_HEADER = os.path.join(ROOT, "include", "needletail_amd_sketch.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, WALK_HPP = os.path.join(CSRC, "ntk_minhash.hip"), os.path.join(CSRC, "ntk_wide_walk.hpp")
CHUNKS = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_chunks.hpp")   # the chunk geometry every library walks
SKETCH_HIP, WIDE_HIP = os.path.join(CSRC, "ntk_sketch.hip"), os.path.join(CSRC, "ntk_wide_count.hip")
GPU_TESTS = "test_gpu_minhash.py"
ERR_BAD_ARG = 2
ROW = L.BY_NAME["minhash"]


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


def test_struct_fields_are_the_bindings():
    from needletail_amd import minhashing as K
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for tag, cls in (("ntk_minhash_stats", K.Stats), ("ntk_minhash_comparison", K.Comparison)):
        body = re.search(rf"struct {tag} \{{(.*?)\}};", hdr, re.S).group(1)
        fields = [f.strip() for decl in re.findall(r"(?:uint64_t|uint32_t|double) ([^;]+);", body) for f in decl.split(",")]
        assert fields == [name for name, _ in cls._fields_], tag
    assert C.sizeof(K.Stats) == 72 and C.sizeof(K.Comparison) == 56   # the header's, which its C program states (tests/_libraries.py)
    assert (K.MAX_NUM, K.BUFFER_DEFAULT, K.BUFFER_MIN, K.BUFFER_MAX) == (M.MAX_NUM, M.BUFFER_DEFAULT, M.BUFFER_MIN, M.BUFFER_MAX)


# ---- constants, the hash and the walker --------------------------------------------------------------------------------------------

def test_minhash_constants_are_the_sketchs_and_the_models():
    """The GPU tests compare hashes bit for bit with tests/_minhash_model.py, which hashes with tests/_sketch_model.py.  The two headers,
    the two sources and the model must state one hash and one chunk length."""
    from needletail_amd import minhashing as K
    src, hdr, sk_hdr, sk_src = open(HIP).read(), open(HEADER).read(), open(SKETCH_HEADER).read(), open(SKETCH_HIP).read()
    xor = int(re.search(r"#define NTK_MINHASH_XOR (0x[0-9A-Fa-f]+)ull", hdr).group(1), 16)
    assert xor == int(re.search(r"#define NTK_SKETCH_XOR (0x[0-9A-Fa-f]+)ull", sk_hdr).group(1), 16) == S.XOR == M.XOR == K.XOR != 0
    assert int(re.search(r"kXor = (0x[0-9A-Fa-f]+)ull;", src).group(1), 16) == xor
    assert int(re.search(r"kXor = (0x[0-9A-Fa-f]+)ull;", sk_src).group(1), 16) == xor
    assert "needletail_amd_sketch.h" not in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S) and "needletail_amd_sketch.h" not in src
    # the two hash functions, text for text, under this library's name
    for text, name in ((src, "minhash_hash"), (sk_src, "sketch_hash")):
        assert re.search(name + r"\(uint64_t key\) \{ return fmix64\(key \^ kXor\); \}", text)
        assert re.search(name + r"\(uint64_t hi, uint64_t lo\) \{ return fmix64\(lo \^ fmix64\(hi\) \^ kXor\); \}", text)
    assert '#include "ntk_consumer.hpp"' in src and not re.search(r"\bfmix64\([^)]*\)\s*\{", src), "fmix64 defined again"
    chunk = re.search(r"kChunkBases = \(uint64_t\)(\d+) << (\d+);", open(CHUNKS).read())
    assert int(chunk.group(1)) << int(chunk.group(2)) == M.CHUNK == S.CHUNK == CM.CHUNK
    assert not re.search(r"kChunkBases\s*=", src), "the chunk length is ntk_chunks.hpp's alone"
    assert int(re.search(r"#define NTK_MINHASH_MAX_NUM \(1ull << (\d+)\)", hdr).group(1)) == 20
    assert int(re.search(r"#define NTK_MINHASH_BUFFER_DEFAULT \(1ull << (\d+)\)", hdr).group(1)) == 22
    assert int(re.search(r"#define NTK_MINHASH_BUFFER_MIN (\d+)ull", hdr).group(1)) == M.BUFFER_MIN == M.LANE_RUN
    assert int(re.search(r"#define NTK_MINHASH_BUFFER_MAX \(1ull << (\d+)\)", hdr).group(1)) == 28
    assert re.search(r"if \(take\[u\] && h <= a\.c\.tau\)", src) and re.search(r"if \(h <= a\.c\.tau\)", src), "the test is inclusive"
    assert not re.search(r"\basm\b|__asm", src + open(WALK_HPP).read()), "plain HIP C++"
    gpu_tests = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()   # the seam test spans three blocks of the wide kernel
    assert re.search(r"kFilterThreads = (\d+);", src).group(1) == re.search(r"^FILTER_THREADS = (\d+)\b", gpu_tests, re.M).group(1)
    # the hash the model takes from the sketch model is the header's text
    def fmix(x):
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd & CM.M64
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 & CM.M64
        return x ^ (x >> 33)
    rng = np.random.default_rng(0x61)
    keys = rng.integers(0, 1 << 64, 32, dtype=np.uint64)
    h, c = M.sketch(keys, scaled=1)
    assert [int(v) for v in h] == sorted(fmix(int(v) ^ xor) for v in keys) and c.tolist() == [1] * 32
    rows = rng.integers(0, 1 << 62, (32, 2), dtype=np.uint64)
    assert [int(v) for v in M.sketch(rows, scaled=1)[0]] == sorted(fmix(int(lo) ^ fmix(int(hi)) ^ xor) for hi, lo in rows)
    assert int(M.sketch(np.array([xor], dtype=np.uint64), num=1)[0][0]) == 0   # the key C hashes to 0


def test_walker_header_is_the_two_sources_walk():
    """ntk_wide_walk.hpp restates the walk of ntk_wide_count.hip, which keeps its own: the same lane run, lead, k range and per-byte
    rules.  The sketch's walk is the header's by construction: ntk_sketch.hip includes it and defines neither a walker nor the lane
    geometry.  The MinHash library and the sketch include it, and nothing else does."""
    walk, sk, wide = open(WALK_HPP).read(), open(SKETCH_HIP).read(), open(WIDE_HIP).read()
    for text in (walk, wide):
        assert int(re.search(r"kLaneRun = (\d+);", text).group(1)) == M.LANE_RUN
        assert int(re.search(r"kPrime = (\d+);", text).group(1)) == M.PRIME
        assert re.search(r"kKMax = (\d+);", text).group(1) == "63"
    norm = lambda t: re.sub(r"\s+", " ", t.replace("a.cutoff", "cutoff").replace("a.n_bytes", "n_bytes").replace("kPrime", "kLead")
                            .replace("kLaneRun", "kRun"))
    rules = ("hi_bits = 2 * k - 64, rc_shift = 2 * k - 66;", "const uint64_t hi_mask = ((uint64_t)1 << hi_bits) - 1;",
             "blk < (kLead + kRun) / 16; blk++)", "const uint64_t at = first_end + 16 * blk;",
             "uint4 s = make_uint4(0, 0, 0, 0), q = make_uint4(~0u, ~0u, ~0u, ~0u);", "if (at >= kLead && at - kLead < n_bytes) {",
             "const uint32_t b = s.x & 0xFF, qb = q.x & 0xFF;",
             "s.x = (s.x >> 8) | (s.y << 24); s.y = (s.y >> 8) | (s.z << 24); s.z = (s.z >> 8) | (s.w << 24); s.w >>= 8;",
             "q.x = (q.x >> 8) | (q.y << 24); q.y = (q.y >> 8) | (q.z << 24); q.z = (q.z >> 8) | (q.w << 24); q.w >>= 8;",
             "const uint64_t pos_plus = at + j;", "const uint32_t l = b | 0x20;",
             "(l == 'a' || l == 'c' || l == 'g' || l == 't' || l == 'u') && qb >= cutoff &&", "pos_plus - kLead < n_bytes;",
             "const uint64_t c = ((b >> 1) ^ (b >> 2)) & 3;", "fh = ((fh << 2) | (fl >> 62)) & hi_mask;", "fl = (fl << 2) | c;",
             "rl = (rl >> 2) | (rh << 62);", "rh = (rh >> 2) | ((3 - c) << rc_shift);", "run = base ? run + 1 : 0;",
             "if (run >= k && pos_plus >= first_end + kLead) {", "const bool fwd = fh < rh || (fh == rh && fl <= rl);")
    for rule in rules:
        for name, text in (("walk", walk), ("wide", wide)):
            assert rule in norm(text), (name, rule)
    # the sketch walks with the header's walker and geometry: it includes the header and restates neither
    assert '#include "ntk_wide_walk.hpp"' in sk and "walk_lane_run<kLaneRun, kPrime>(" in sk
    assert not re.search(r"template <uint32_t kRun, uint32_t kLead, class Emit>", sk), "a walker defined again in ntk_sketch.hip"
    assert not re.search(r"\bk(?:LaneRun|Prime|KMax)\s*=", sk), "the lane geometry stated again in ntk_sketch.hip"
    assert len(re.findall(r"template <uint32_t kRun, uint32_t kLead, class Emit>", walk)) == 1
    users = [f for f in sorted(os.listdir(CSRC)) if "ntk_wide_walk.hpp" in open(os.path.join(CSRC, f), errors="replace").read()
             and f != "ntk_wide_walk.hpp" and f != "Makefile"]
    assert users == ["ntk_minhash.hip", "ntk_sketch.hip"], users


# ---- the model's algebra ------------------------------------------------------------------------------------------------------------

def _key_multiset(rng, n, distinct):
    pool = rng.integers(0, 1 << 64, distinct, dtype=np.uint64)
    return pool[rng.integers(0, distinct, n)]


@pytest.mark.parametrize("kind", [dict(num=1), dict(num=50), dict(num=10 ** 6), dict(scaled=1), dict(scaled=7), dict(scaled=40)])
def test_model_sketch_of_a_sum_is_the_merge_of_the_sketches(kind):
    rng = np.random.default_rng(0x62)
    for n_a, n_b, distinct in ((3000, 2000, 800), (500, 0, 100), (0, 0, 1), (40, 4000, 3000)):
        pool = rng.integers(0, 1 << 64, distinct, dtype=np.uint64)
        a, b = pool[rng.integers(0, distinct, n_a)], pool[rng.integers(0, distinct, n_b)]
        whole = M.sketch(np.concatenate([a, b]), **kind)
        parts = M.merge(M.sketch(a, **kind), M.sketch(b, **kind), **kind)
        assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1]), (kind, n_a, n_b)
        assert int(whole[1].sum()) <= n_a + n_b and np.all(whole[0][1:] > whole[0][:-1])
        if "scaled" in kind and kind["scaled"] == 1:
            assert int(whole[1].sum()) == n_a + n_b
    wide = rng.integers(0, 1 << 62, (600, 2), dtype=np.uint64)
    wide = wide[rng.integers(0, 600, 2500)]
    whole, parts = M.sketch(wide, **kind), M.merge(M.sketch(wide[:1000], **kind), M.sketch(wide[1000:], **kind), **kind)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])


def test_model_scaled_sketches_nest():
    rng = np.random.default_rng(0x63)
    keys = _key_multiset(rng, 20000, 6000)
    for a, b in ((1, 7), (3, 5), (7, 7), (2, 1000)):
        fine, coarse = M.sketch(keys, scaled=a), M.sketch(keys, scaled=a * b)
        keep = fine[0] <= np.uint64(M.max_hash(a * b))
        assert np.array_equal(fine[0][keep], coarse[0]) and np.array_equal(fine[1][keep], coarse[1])
        assert M.threshold(coarse[0], scaled=a * b) == ((1 << 64) - 1) // (a * b)
    assert len(M.sketch(keys, scaled=3)[0]) > len(M.sketch(keys, scaled=15)[0]) > 100
    h = M.sketch(keys, num=100)[0]
    assert M.threshold(h, num=100) == int(h[-1]) and M.threshold(h[:99], num=100) == M.ALL


# ---- ntk_minhash_compare: host code, against the set model ---------------------------------------------------------------------------

def _assert_compare(a, ca, b, cb, num=0, max_hash=M.ALL):
    from needletail_amd import minhashing as K
    got, want = K.compare(a, ca, b, cb, num, max_hash), M.compare(a, ca, b, cb, num, max_hash)
    for key in ("n_a", "n_b", "n_shared", "n_union"):
        assert got[key] == want[key], (key, got, want)
    for key in ("dot", "norm2_a", "norm2_b"):
        assert got[key] == pytest.approx(want[key], rel=1e-12), (key, got, want)
    return got


def _sorted_unique(rng, n, top=1 << 64):
    return np.unique(rng.integers(0, top, n, dtype=np.uint64))


def test_compare_matches_the_set_model():
    rng = np.random.default_rng(0x64)
    none = np.zeros(0, dtype=np.uint64)
    for top in (1 << 64, 3000):   # sparse: few shared; dense: many shared
        for n_a, n_b in ((1000, 1000), (1500, 200), (1, 1), (300, 0), (0, 0)):
            a, b = _sorted_unique(rng, n_a, top), _sorted_unique(rng, n_b, top)
            ca, cb = rng.integers(1, 1 << 20, a.size, dtype=np.uint64), rng.integers(1, 1 << 20, b.size, dtype=np.uint64)
            for num in (0, 1, 10, 500, 10 ** 6):   # 10^6: more than the union holds
                for cut in (M.ALL, top // 2, top // 1000, 0):
                    got = _assert_compare(a, ca, b, cb, num, cut)
                    _assert_compare(a, None, b, cb, num, cut)
                    plain = _assert_compare(a, None, b, None, num, cut)
                    assert plain["dot"] == plain["n_shared"] and got["n_union"] == plain["n_union"]
                    if num:
                        assert got["n_union"] == min(num, len(set(a[a <= np.uint64(cut)].tolist()) | set(b[b <= np.uint64(cut)].tolist())))
        dense = _assert_compare(_sorted_unique(rng, 2000, 3000), None, _sorted_unique(rng, 2000, 3000), None)
        assert dense["n_shared"] > 100
    a = _sorted_unique(rng, 400)
    ca = rng.integers(1, 100, a.size, dtype=np.uint64)
    same = _assert_compare(a, ca, a, ca)
    assert same["n_shared"] == same["n_union"] == same["n_a"] == a.size and same["dot"] == same["norm2_a"] == same["norm2_b"]
    disjoint = _assert_compare(a[::2], None, a[1::2], None)
    assert disjoint["n_shared"] == 0 and disjoint["n_union"] == a.size and disjoint["dot"] == 0.0
    mash = _assert_compare(a[::2], None, a[1::2], None, num=50)
    assert mash["n_union"] == 50 and mash["n_shared"] == 0 and mash["norm2_a"] + mash["norm2_b"] == 50.0
    empty = _assert_compare(none, None, none, None, num=10)
    assert empty == {"n_a": 0, "n_b": 0, "n_shared": 0, "n_union": 0, "dot": 0.0, "norm2_a": 0.0, "norm2_b": 0.0}
    # downsampling two scaled sketches of different `scaled` to the coarser one
    keys_a, keys_b = _key_multiset(rng, 30000, 9000), _key_multiset(rng, 30000, 9000)
    keys_b[:10000] = keys_a[:10000]
    fine, coarse = M.sketch(keys_a, scaled=2), M.sketch(keys_b, scaled=6)
    down = _assert_compare(*fine, *coarse, 0, M.max_hash(6))
    both = M.sketch(keys_a, scaled=6)
    assert down["n_a"] == len(both[0]) < len(fine[0]) and down["n_b"] == len(coarse[0]) and down["n_shared"] > 100
    # large counts: the sums are doubles
    big = np.array([M.ALL, M.ALL - 1], dtype=np.uint64)
    _assert_compare(a[:2], big, a[:2], big)


def test_compare_refuses_unsorted_and_repeated_input():
    from needletail_amd import minhashing as K
    import needletail_amd as nt
    good = np.array([1, 5, 9], dtype=np.uint64)
    for bad in (np.array([1, 9, 5], dtype=np.uint64), np.array([1, 5, 5], dtype=np.uint64), np.array([9, 5, 1], dtype=np.uint64)):
        for args in ((bad, None, good, None), (good, None, bad, None)):
            with pytest.raises(nt.NtkError) as e:
                K.compare(*args)
            assert e.value.status == ERR_BAD_ARG
        with pytest.raises(nt.NtkError) as e:   # also where the cut would hide it
            K.compare(bad, None, good, None, 0, 0)
        assert e.value.status == ERR_BAD_ARG
    for args in ((good.astype(np.int64), None, good, None), (good, good[:2], good, None), (None, None, good, None)):
        with pytest.raises(nt.NtkError) as e:
            K.compare(*args)
        assert e.value.status == ERR_BAD_ARG
    lib, out = K.lib(), K.Comparison()
    assert lib.ntk_minhash_compare(None, None, 3, good.ctypes.data, None, 3, 0, M.ALL, C.byref(out)) == ERR_BAD_ARG
    assert lib.ntk_minhash_compare(good.ctypes.data, None, 3, good.ctypes.data, None, 3, 0, M.ALL, None) == ERR_BAD_ARG
    assert lib.ntk_minhash_compare(None, None, 0, None, None, 0, 0, M.ALL, C.byref(out)) == 0 and out.n_union == 0
