"""CPU-side checks of the wide count library (include/needletail_amd_wide_count.h, libneedletail_amd_wide_count.so, k = 33..63) beyond
those every library is held to (tests/test_consumer_abi.py): the host model of the table (tests/_wide_count_model.py) with its constants
tied to the kernel source."""
import os
import re

import numpy as np
import pytest

import _count_model as CM
import _libraries as L
import _wide_count_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_wide_count.hip")
COMMON = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_count_common.hpp")   # what the narrow and the wide table share
CONSUMER = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_consumer.hpp")    # what every library on the core's ABI shares
ROW = L.BY_NAME["wide_count"]


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


# ---- the host model (tests/_wide_count_model.py), which the GPU tests aim with ------------------------------------------------------

def test_table_hash_probe_bound_and_lane_geometry_are_the_models():
    """The GPU tests aim keys at home slots and records at lane-run seams with tests/_wide_count_model.py.  If the table's hash, probe
    bound or the count kernel's geometry changes, say so here, on the CPU, rather than as a puzzling count mismatch on the GPU."""
    src, common, consumer = open(HIP).read(), open(COMMON).read(), open(CONSUMER).read()
    m = re.search(r"inline uint64_t fmix64\(uint64_t x\)\s*\{(.*?)\}", consumer, re.S)
    assert m, "fmix64 not found in ntk_consumer.hpp"
    steps = re.findall(r"x \^= x >> (\d+);|x \*= (0x[0-9a-fA-F]+)ull;", m.group(1))
    got = [int(a) if a else int(b, 16) for a, b in steps]
    assert got == [CM.FMIX_SHIFT, CM.FMIX_MUL[0], CM.FMIX_SHIFT, CM.FMIX_MUL[1], CM.FMIX_SHIFT], got
    assert re.search(r"home_slot\(uint64_t hi, uint64_t lo, uint64_t mask\) \{ return fmix64\(lo \^ fmix64\(hi\)\) & mask; \}", src)
    assert len(re.findall(r"home_slot\(x, y, t\.mask\)", src)) == 2, "insert and lookup do not both start at home_slot"
    assert len(re.findall(r"slot = \(slot \+ 1\) & t\.mask", src)) == 2, "probing is not linear with wrap-around"
    assert int(re.search(r"kProbeMax = (\d+);", common).group(1)) == W.PROBE_MAX
    assert int(re.search(r"kLaneRun = (\d+);", src).group(1)) == W.LANE_RUN
    assert int(re.search(r"kPrime = (\d+);", src).group(1)) == W.PRIME
    assert int(re.search(r"kThreads = (\d+);", consumer).group(1)) == W.THREADS
    assert re.search(r"kKMin = (\d+), kKMax = (\d+);", src).groups() == (str(W.K_MIN), str(W.K_MAX))


def _int_revcomp(v, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (v & 3))
        v >>= 2
    return r


def test_model_revcomp_and_canonical():
    rng = np.random.default_rng(0xA1)
    for k in (33, 34, 40, 51, 62, 63):
        vals = [int(rng.integers(0, 1 << 62)) << 64 | int(rng.integers(0, 1 << 63)) * 2 for _ in range(64)]
        vals = [v & ((1 << (2 * k)) - 1) for v in vals]
        hi = np.array([v >> 64 for v in vals], dtype=np.uint64)
        lo = np.array([v & W.M64 for v in vals], dtype=np.uint64)
        rh, rl = W.revcomp(hi, lo, k)
        assert [W.join(a, b) for a, b in zip(rh, rl)] == [_int_revcomp(v, k) for v in vals], k
        ch, cl = W.canonical(hi, lo, k)
        assert [W.join(a, b) for a, b in zip(ch, cl)] == [min(v, _int_revcomp(v, k)) for v in vals], k


def _kmer(s, k):
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    v = 0
    for ch in s:
        v = (v << 2) | code[ch]
    assert len(s) == k
    return v


def _adversarial(k):
    """A^i T^j and T^i A^j for every split, C/G runs, the palindromes of even k, and a few random keys."""
    out = set()
    for i in range(k + 1):
        for a, b in (("A", "T"), ("T", "A"), ("C", "G"), ("G", "C"), ("T", "T"), ("A", "C")):
            out.add(_kmer(a * i + b * (k - i), k))
    if k % 2 == 0:
        rng = np.random.default_rng(k)
        for _ in range(200):
            half = "".join("ACGT"[x] for x in rng.integers(0, 4, k // 2))
            comp = half[::-1].translate(str.maketrans("ACGT", "TGCA"))
            out.add(_kmer(half + comp, k))
    return sorted(out)


@pytest.mark.parametrize("k", list(range(33, 64)))
def test_no_canonical_key_has_an_empty_word(k):
    rng = np.random.default_rng(0xE0 + k)
    hi = rng.integers(0, 1 << (2 * k - 64), 100_000, dtype=np.uint64)
    lo = rng.integers(0, 1 << 63, 100_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 100_000, dtype=np.uint64)
    lo[:1000] = W.M64   # the keys that end in 32 T
    ch, cl = W.canonical(hi, lo, k)
    assert not (ch == np.uint64(W.EMPTY)).any() and not (cl == np.uint64(W.EMPTY)).any()
    for v in _adversarial(k):
        c = min(v, _int_revcomp(v, k))
        assert c >> 64 != W.M64 and c & W.M64 != W.M64, (k, hex(v))


def test_at_k_64_exactly_the_two_palindromes_have_an_empty_word():
    k = 64
    bad = set()
    for v in _adversarial(k):
        c = min(v, _int_revcomp(v, k))
        if c >> 64 == W.M64 or c & W.M64 == W.M64:
            bad.add(c)
    assert bad == {_kmer("T" * 32 + "A" * 32, k), _kmer("A" * 32 + "T" * 32, k)}


@pytest.mark.parametrize("k,h", [(63, 0), (63, 8191), (51, 4000), (33, 17)])
def test_model_keys_sharing_hi(k, h):
    slots = 8192
    word = 5 & ((1 << (2 * k - 64)) - 1)
    hi, lo = W.keys_sharing_hi(h, slots, k, word, 300)
    assert hi.size == 300 and np.unique(lo).size == 300 and (hi == word).all()
    assert (W.home(hi, lo, slots) == h).all() and W.is_canonical(hi, lo, k).all()
    assert (lo != np.uint64(W.EMPTY)).all()


@pytest.mark.parametrize("h", [0, 5000, 8191])
def test_model_keys_sharing_lo(h):
    k, slots = 63, 8192
    hi, lo = W.keys_sharing_lo(h, slots, k, 0x0123456789ABCDEF, 300)
    assert hi.size == 300 and np.unique(hi).size == 300 and (lo == 0x0123456789ABCDEF).all()
    assert (hi >> np.uint64(2 * k - 64) == 0).all()
    assert (W.home(hi, lo, slots) == h).all() and W.is_canonical(hi, lo, k).all()


def test_model_records_emit_exactly_the_keys():
    import oracle as O
    k = 51
    hi, lo = W.keys_sharing_hi(3, 1024, k, 77, 4)
    buf = W.records_for(hi, lo, [3, 1, 2, 7], k, seed=1)
    assert len(buf) == 13 * (k + 1)
    seq = buf.replace(b"\n", b"N")
    pos, flg = O.canonical_kmers_arrays(seq, O.reverse_complement(seq), k)
    assert pos.size == 13
    want = {W.join(a, b): c for a, b, c in zip(hi, lo, [3, 1, 2, 7])}
    got = {}
    rc = O.reverse_complement(seq)
    for p, f in zip(pos.tolist(), flg.tolist()):
        s = rc[len(seq) - p - k: len(seq) - p] if f else seq[p: p + k]
        v = _kmer(s.decode(), k)
        got[v] = got.get(v, 0) + 1
    assert got == want
