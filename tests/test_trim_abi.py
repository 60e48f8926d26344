"""CPU-side checks of the trim library (include/needletail_amd_trim.h, libneedletail_amd_trim.so) beyond those every library is held to
(tests/test_consumer_abi.py): the row layout and the modes, the scratch bound's arithmetic, the refusal of a wide table, the host model
(tests/_trim_model.py) on hand-made solid patterns, and the run search of csrc/ntk_trim_runs.hpp, compiled here with g++, against that
model: exhaustively on short bit strings at every bit offset, on random strings around the word and round seams, and split at every point
into two parts that are combined."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _libraries as L
import _trim_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_trim.h")
HIP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_trim.hip")
CHUNKS = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_chunks.hpp")   # the chunk geometry every library walks
RUNS_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_trim_runs.hpp")
MEM = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_device_mem.hpp")   # how the handle owns its arrays

T_GROUP_WORDS, T_LONG_PIECES = 32, 2048   # tests/test_gpu_trim.py GROUP_WORDS, LONG_PIECES
ROW = L.BY_NAME["trim"]


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


def test_row_layout_is_the_columns():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct ntk_read_trim_row \{(.*?)\};", hdr, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]+);", body) for f in decl.split(",")]
    assert tuple(fields) == T.COLUMNS
    from needletail_amd import trimming
    assert trimming.COLUMNS == T.COLUMNS
    assert (trimming.TRIM_PREFIX, trimming.TRIM_LONGEST) == (T.PREFIX, T.LONGEST)
    hdr = open(HEADER).read()
    assert re.search(r"NTK_TRIM_PREFIX = 0,", hdr) and re.search(r"NTK_TRIM_LONGEST = 1\b", hdr)


def test_kernel_constants_are_the_tests():
    """The GPU tests aim at the group / wave seam of the interval kernel, the long-record threshold of the copy and the chunk length."""
    import _count_model as CM
    src = open(HIP).read()
    chunk = re.search(r"kChunkBases = \(uint64_t\)(\d+) << (\d+);", open(CHUNKS).read())
    assert int(chunk.group(1)) << int(chunk.group(2)) == CM.CHUNK
    assert not re.search(r"kChunkBases\s*=", src), "the chunk length is ntk_chunks.hpp's alone"
    group, rounds = (int(re.search(rf"{name} = (\d+);", src).group(1)) for name in ("kGroup", "kGroupRounds"))
    assert group * rounds == T_GROUP_WORDS and 64 % group == 0
    assert int(re.search(r"kLongPieces = (\d+);", src).group(1)) == T_LONG_PIECES
    assert not re.search(r"\basm\b|__asm", src), "plain HIP C++"
    assert not re.search(r"\basm\b|__asm|hip/|__shfl", open(RUNS_HPP).read()), "the run header is plain C++"


def test_scratch_bound_arithmetic():
    """The header's memory statement, term by term, against the allocation sizes in the source: no batch-long 8 B per base array (the
    lookup writes a chunk-long one from its start), two planes of 1/8 B per base + 16 B each, 16 B per record + 16 B for the scan,
    8 B per 16 384 bases + 16 B for the list of long records."""
    import _count_model as CM
    src, hdr = open(HIP).read(), re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    assert re.search(r"ntk_kmer_table_lookup_device\(t->table, t->scratch\.d_values\.p \+ c\.skip\(\), c\.end - c\.start, t->d_counts\.p\)", src)
    # every array of the handle grows to exactly what is asked for (grow_exact of ntk_device_mem.hpp), in elements of its type
    assert re.search(r"uint64_t grow_exact\(uint64_t, uint64_t need\) \{ return need; \}", open(MEM).read())
    assert re.search(r"DeviceArray<uint64_t> d_counts;", src) and re.search(r"DeviceArray<uint64_t> d_solid, d_valid;", src)
    assert re.search(r"DeviceArray<ScanItem> d_scan;", src) and re.search(r"DeviceArray<uint64_t> d_long;", src)
    assert re.search(r"t->d_counts\.ensure\(t->stream, \(chunk_bases\(n_bytes\) \+ 15\) & ~\(uint64_t\)15, grow_exact\)", src)
    for plane in ("d_solid", "d_valid"):
        assert re.search(rf"t->{plane}\.ensure\(t->stream, planes_words\(n_bytes\), grow_exact\)", src)
    assert re.search(r"uint64_t chunk_bases\(uint64_t n_bytes\) \{ return n_bytes < kChunkBases \? n_bytes : kChunkBases; \}", open(CHUNKS).read())
    assert re.search(r"uint64_t planes_words\(uint64_t n_bytes\) \{ return \(n_bytes \+ 63\) / 64 \+ 1; \}", src)
    assert re.search(r"t->d_scan\.ensure\(t->stream, n_records \+ 1, grow_exact\)", src)
    assert re.search(r"t->d_long\.ensure\(t->stream, \(n_bytes >> 14\) \+ 2, grow_exact\)", src)
    assert re.search(r"struct ScanItem \{\s*uint64_t bytes, records;", src)
    for phrase in ("8 B per base of at most 64 MiB of bases", "no batch-long count array", "1/8 B per base each, plus 16 B",
                   "16 B per record plus 16 B", "8 B per 16 384 bases"):
        assert phrase in hdr, phrase
    for n in (1, 15, 16, 63, 64, 65, 1000, CM.CHUNK - 1, CM.CHUNK, CM.CHUNK + 1, 10 * CM.CHUNK + 12345, 1 << 40):
        chunk = min(n, CM.CHUNK)
        assert 8 * ((chunk + 15) // 16 * 16) <= 8 * CM.CHUNK                              # the counts: of one chunk
        assert 8 * ((n + 63) // 64 + 1) * 8 <= n + 16 * 8                                 # a plane: n / 8 + 16 bytes (times 8: integers)
        assert 8 * ((n >> 14) + 2) * 16384 <= 8 * n + 16 * 16384                          # the list: 8 n / 16384 + 16 bytes
        for n_records in (1, n):
            assert 16 * (n_records + 1) == 16 * n_records + 16
    # a long record of the copy needs more than (kLongPieces - 2) * 16 bytes, so the list's capacity holds every one of them
    assert (T_LONG_PIECES - 2) * 16 >= 16384


def test_wide_table_is_a_type_error():
    import needletail_amd as nt
    wide = object.__new__(nt.WideKmerTable)   # no device needed: the argument's type alone decides
    wide._h = None
    with pytest.raises(TypeError, match=r"k <= 32.*33\.\.63"):
        nt.ReadTrimmer(wide)
    with pytest.raises(TypeError):
        nt.ReadTrimmer("table")


# ---- the host model (tests/_trim_model.py), which the GPU tests hold the rows to ------------------------------------------------------

def _bits(s):
    return [c == "1" for c in s]


def test_model_intervals_on_hand_made_patterns():
    P, Lg, k = T.PREFIX, T.LONGEST, 5
    iv = lambda s, mode, ml=0: T.interval(_bits(s), k, mode, ml)   # noqa: E731
    # all solid: the whole record, L = windows + k - 1
    assert iv("1111", P) == iv("1111", Lg) == (0, 8)
    assert iv("1", P) == iv("1", Lg) == (0, 5)                     # L = k: one window
    assert iv("11", P) == iv("11", Lg) == (0, 6)                   # L = k + 1
    assert iv("", P) == iv("", Lg) == (0, 0)                       # L = k - 1 (or empty): no window
    # a weak first window: khmer keeps nothing, the longest run starts later
    assert iv("0111", P) == (0, 0) and iv("0111", Lg) == (1, 7)
    # a weak last window
    assert iv("1110", P) == (0, 7) and iv("1110", Lg) == (0, 7)
    # PREFIX cuts at the first weak window end j* = k - 1 + i: kept [0, j*)
    assert iv("1101111", P) == (0, 6) and iv("1101111", Lg) == (3, 8)
    # ties: the leftmost run wins
    assert iv("0110110", Lg) == (1, 6) and iv("1101100", Lg) == (0, 6) and iv("1010101", Lg) == (0, 5)
    assert iv("0011101110", Lg) == (2, 7)
    assert iv("0000", P) == iv("0000", Lg) == (0, 0)
    # min_length: 0 counts as k; a shorter interval becomes empty (and no shorter run is taken in its place)
    assert iv("1101111", P, 6) == (0, 6) and iv("1101111", P, 7) == (0, 0)
    assert iv("1101111", Lg, 8) == (3, 8) and iv("1101111", Lg, 9) == (0, 0)
    assert iv("1", P, 0) == iv("1", P, 5) == iv("1", P, 3) == (0, 5) and iv("1", P, 6) == (0, 0)
    # rows: n_kmers and n_solid are counted before min_length empties anything; min_count 0 = 1
    ends, counts = np.array([4, 5, 7, 8]), np.array([3, 1, 0, 9], dtype=np.uint64)   # L = 9: windows end at 4 .. 8, the one at 6 not emitted
    assert T.row(9, k, ends, counts, P, 1).tolist() == [0, 6, 4, 3]
    assert T.row(9, k, ends, counts, P, 0).tolist() == [0, 6, 4, 3]
    assert T.row(9, k, ends, counts, Lg, 3).tolist() == [0, 5, 4, 2]                 # 1 0 x 0 1: a tie, the leftmost
    assert T.row(9, k, ends, counts, Lg, 3, 6).tolist() == [0, 0, 4, 2]
    assert T.row(3, k, [], [], P).tolist() == [0, 0, 0, 0] and T.row(0, k, [], [], Lg).tolist() == [0, 0, 0, 0]
    assert T.row(9, k, ends, counts, P).dtype == np.uint64
    with pytest.raises(ValueError):
        T.interval([True], k, 2)
    # every kept interval holds only solid windows, and extends no further
    rng = np.random.default_rng(0x71)
    for _ in range(2000):
        n, kk = int(rng.integers(0, 40)), int(rng.integers(1, 8))
        s = rng.random(n) < rng.random()
        for mode in (P, Lg):
            st, ln = T.interval(s, kk, mode)
            if ln:
                w0, w1 = st, st + ln - kk   # the windows of the interval: those ending at st + kk - 1 .. st + ln - 1
                assert ln >= kk and s[w0:w1 + 1].all() and (w1 + 1 == n or not s[w1 + 1]) and (mode == P or w0 == 0 or not s[w0 - 1])
                assert mode == Lg or st == 0
            else:
                assert not s.any() if mode == Lg else (n == 0 or not s[0])


def test_model_windows_compaction_and_text():
    import needletail_amd as nt
    from _count_helpers import PATH_PRES, oracle_values, random_records
    # positions: the values are oracle_values', the ends ascend, and a record's N breaks them
    for path, pre in PATH_PRES:
        for k in (1, 5, 21, 32):
            for r in random_records(0x7A, 12) + [b"", b"ACGT", b"ACGTNACGTAC"]:
                ends, vals = T.record_windows(r, k, path, pre)
                assert np.array_equal(vals, oracle_values(r + b"\n", k, path, pre))
                assert len(ends) == len(vals) and (np.diff(ends) > 0).all()
                assert all(k - 1 <= e < len(r) for e in ends)
    ends, _ = T.record_windows(b"ACGTNACGTAC", 3, nt.PATH_BITS, nt.PRE_NONE)
    assert ends.tolist() == [2, 3, 7, 8, 9, 10]
    ends, _ = T.record_windows(b"ACGTNACGTAC", 3, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE)
    assert ends.tolist() == [2, 3, 7, 8, 9, 10]
    # the output batch
    recs = [b"ACGTACGT", b"", b"TTTTT", b"GGGGGGGGGGGGGGGGGGGG"]
    rows = [[2, 4, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [19, 50, 0, 0]]   # the last one is clamped to one byte
    seq, n, off, src = T.compact(recs, rows)
    assert (seq, n, off.tolist(), src.tolist()) == (b"GTAC\nG\n" + b"\n" * 9, 7, [0, 5, 7], [0, 3])
    aux = [b"abcdefgh", b"", b"vwxyz", b"01234567890123456789"]
    out = T.compact(recs, rows, aux, [ord("!"), ord("?"), ord("#"), ord("$")])
    assert out[4] == b"cdef!9$" + b"\n" * 9
    assert T.compact(recs, [[0, 0, 0, 0]] * 4)[:2] == (b"", 0)
    assert T.clamp(5, 9, 9) == (5, 0) and T.clamp(5, 2, 9) == (2, 3) and T.clamp(5, 1, 2) == (1, 2)
    assert T.cli_text(["a", "b"], [b"ACGT", b"TT"], [[1, 2, 0, 0], [0, 0, 0, 0]]) == ">a\nCG\n"
    assert T.cli_text(["a x", "b"], [b"ACGT", b"TT"], [[1, 2, 0, 0], [0, 2, 0, 0]], [b"IJKL", b"MN"]) == "@a x\nCG\n+\nJK\n@b\nTT\n+\nMN\n"


# ---- the run search of csrc/ntk_trim_runs.hpp, compiled with g++ -----------------------------------------------------------------------

SHIM = r"""
#include "ntk_trim_runs.hpp"
#include <vector>
static void put(const RtRuns &r, uint64_t *o) { o[0] = r.len; o[1] = r.lead; o[2] = r.trail; o[3] = r.best; o[4] = r.best_pos; }
static bool same(const RtRuns &r, const uint64_t *w) { return r.len == w[0] && r.lead == w[1] && r.trail == w[2] && r.best == w[3] && r.best_pos == w[4]; }
// the words of [lo, hi) folded one after the other
static RtRuns serial(const uint64_t *plane, uint64_t lo, uint64_t hi)
{
    RtRuns r;
    if (lo < hi)
        for (uint64_t w = lo >> 6; w <= (hi - 1) >> 6; w++) r = rt_combine(r, rt_plane_word_runs(plane[w], w, lo, hi));
    return r;
}
// as the kernel folds them: rounds of G words, lane i with lane i + off for off = 1, 2, 4 .., then onto the carry
static RtRuns lanes(const uint64_t *plane, uint64_t lo, uint64_t hi, uint32_t G)
{
    RtRuns carry;
    if (lo >= hi) return carry;
    const uint64_t w_end = ((hi - 1) >> 6) + 1;
    std::vector<RtRuns> e(G), n(G);
    for (uint64_t w0 = lo >> 6; w0 < w_end; w0 += G) {
        for (uint32_t s = 0; s < G; s++) e[s] = w0 + s < w_end ? rt_plane_word_runs(plane[w0 + s], w0 + s, lo, hi) : RtRuns();
        for (uint32_t off = 1; off < G; off <<= 1) {
            for (uint32_t s = 0; s < G; s++) n[s] = rt_combine(e[s], s + off < G ? e[s + off] : RtRuns());
            e = n;
        }
        carry = rt_combine(carry, e[0]);
    }
    return carry;
}
extern "C" {
void runs_serial(const uint64_t *plane, uint64_t lo, uint64_t hi, uint64_t *out) { put(serial(plane, lo, hi), out); }
void runs_lanes(const uint64_t *plane, uint64_t lo, uint64_t hi, uint32_t G, uint64_t *out) { put(lanes(plane, lo, hi, G), out); }
void runs_interval(const uint64_t *r, int prefix, uint32_t k, uint64_t min_length, uint64_t *out)
{
    RtRuns x; x.len = r[0]; x.lead = r[1]; x.trail = r[2]; x.best = r[3]; x.best_pos = r[4];
    rt_interval(x, prefix != 0, k, min_length, out[0], out[1]);
}
// every split point of [lo, hi): the two parts' summaries combined are want; -1, or the first split that is not
int64_t runs_splits(const uint64_t *plane, uint64_t lo, uint64_t hi, const uint64_t *want)
{
    for (uint64_t mid = lo; mid <= hi; mid++)
        if (!same(rt_combine(serial(plane, lo, mid), serial(plane, mid, hi)), want)) return (int64_t)(mid - lo);
    return -1;
}
// Every bit string of `len` bits (string v: bit i of v is its bit i), at every start offset 0..63 of a plane whose other bits are all
// `fill`: serial, lanes at 8 and 64, every split, and the two intervals at k, against want[v] = {len, lead, trail, best, best_pos,
// prefix start, prefix length, longest start, longest length}.  -1, or v * 64 + offset of the first that differs.
int64_t runs_exhaustive(uint32_t len, uint32_t k, int fill, const uint64_t *want)
{
    for (uint64_t v = 0; v < ((uint64_t)1 << len); v++)
        for (uint32_t o = 0; o < 64; o++) {
            uint64_t plane[3] = {fill ? ~(uint64_t)0 : 0, fill ? ~(uint64_t)0 : 0, fill ? ~(uint64_t)0 : 0};
            for (uint32_t i = 0; i < len; i++) {
                const uint64_t at = 64 + o + i, bit = (uint64_t)1 << (at & 63);
                if ((v >> i) & 1) plane[at >> 6] |= bit; else plane[at >> 6] &= ~bit;
            }
            const uint64_t lo = 64 + o, hi = lo + len, *w = want + 9 * v;
            const RtRuns r = serial(plane, lo, hi);
            uint64_t iv[4];
            rt_interval(r, true, k, 0, iv[0], iv[1]);
            rt_interval(r, false, k, 0, iv[2], iv[3]);
            if (!same(r, w) || !same(lanes(plane, lo, hi, 8), w) || !same(lanes(plane, lo, hi, 64), w) || runs_splits(plane, lo, hi, w) >= 0 ||
                iv[0] != w[5] || iv[1] != w[6] || iv[2] != w[7] || iv[3] != w[8])
                return (int64_t)(v * 64 + o);
        }
    return -1;
}
}
"""


@pytest.fixture(scope="module")
def runs_lib(tmp_path_factory):
    td = tmp_path_factory.mktemp("trim_runs")
    src, so = td / "shim.cpp", td / "libshim.so"
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.dirname(RUNS_HPP), "-o", str(so),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    u64p = C.POINTER(C.c_uint64)
    lib.runs_serial.argtypes = [u64p, C.c_uint64, C.c_uint64, u64p]
    lib.runs_lanes.argtypes = [u64p, C.c_uint64, C.c_uint64, C.c_uint32, u64p]
    lib.runs_interval.argtypes = [u64p, C.c_int, C.c_uint32, C.c_uint64, u64p]
    lib.runs_splits.argtypes = [u64p, C.c_uint64, C.c_uint64, u64p]
    lib.runs_splits.restype = C.c_int64
    lib.runs_exhaustive.argtypes = [C.c_uint32, C.c_uint32, C.c_int, u64p]
    lib.runs_exhaustive.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _plane(bits, lo, fill, rng):
    """A plane with `bits` from bit `lo` on; the bits around them are `fill` (0, 1, or random for None)."""
    n_words = (lo + len(bits)) // 64 + 2
    if fill is None:
        plane = rng.integers(0, 1 << 64, n_words, dtype=np.uint64)
    else:
        plane = np.full(n_words, (1 << 64) - 1 if fill else 0, dtype=np.uint64)
    every = np.unpackbits(plane.view(np.uint8), bitorder="little")
    every[lo:lo + len(bits)] = bits
    return np.packbits(every, bitorder="little").view(np.uint64).copy()


def test_run_header_exhaustively_on_short_strings_at_every_offset(runs_lib):
    """Every bit string of length 0..16 at every start offset 0..63, in a plane of zeros and in a plane of ones (the bits outside the
    range must not count): the summary, the kernel's lane fold at both widths, every split, and both modes' intervals."""
    k = 3
    for n in range(17):
        want = np.zeros((1 << n, 9), dtype=np.uint64)
        for v in range(1 << n):
            bits = [(v >> i) & 1 for i in range(n)]
            want[v] = T.runs(bits) + T.interval(bits, k, T.PREFIX) + T.interval(bits, k, T.LONGEST)
        for fill in (0, 1):
            bad = runs_lib.runs_exhaustive(n, k, fill, _p(want))
            assert bad == -1, (n, fill, bad >> 6, bad & 63)


def test_run_header_on_random_strings_around_the_seams(runs_lib):
    """63, 64, 65, 4095, 4096, 4097 windows and a few of 10^5, at random offsets and densities (all ones included): serial, the lane
    fold at 8 and 64 lanes (4096 windows are one round of the wave at offset 0 and two anywhere else), and the intervals."""
    rng = np.random.default_rng(0x7B)
    out, iv = np.zeros(5, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    for n in [63, 64, 65, 4095, 4096, 4097] * 6 + [100_000] * 4 + [1, 2, 511, 512, 513]:
        for density in (1.0, 0.999, 0.9, 0.5, float(rng.random())):
            bits = (rng.random(n) < density).astype(np.uint8)
            want = T.runs(bits)
            settings = [(mode, k, ml) for mode in (T.PREFIX, T.LONGEST) for k, ml in ((1, 0), (21, 0), (21, 50), (32, 5000))]
            want_iv = [T.interval(bits, k, mode, ml) for mode, k, ml in settings]
            for lo in (0, 63, 64, int(rng.integers(0, 5000))):
                plane = _plane(bits, lo, None, rng)
                for call in (lambda: runs_lib.runs_serial(_p(plane), lo, lo + n, _p(out)),
                             lambda: runs_lib.runs_lanes(_p(plane), lo, lo + n, 8, _p(out)),
                             lambda: runs_lib.runs_lanes(_p(plane), lo, lo + n, 64, _p(out))):
                    call()
                    assert tuple(out.tolist()) == want, (n, density, lo)
                for (mode, k, ml), w in zip(settings, want_iv):
                    runs_lib.runs_interval(_p(out), int(mode == T.PREFIX), k, ml, _p(iv))
                    assert tuple(iv.tolist()) == w, (n, density, lo, mode, k, ml)


def test_run_header_split_at_every_point(runs_lib):
    rng = np.random.default_rng(0x7C)
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 1000):
        for density in (1.0, 0.95, 0.6, 0.0):
            bits = (rng.random(n) < density).astype(np.uint8)
            for lo in (0, 1, 63, int(rng.integers(0, 200))):
                plane = _plane(bits, lo, None, rng)
                want = np.array(T.runs(bits), dtype=np.uint64)
                assert runs_lib.runs_splits(_p(plane), lo, lo + n, _p(want)) == -1, (n, density, lo)
