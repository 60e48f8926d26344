"""CPU-side checks of the de Bruijn graph library (include/needletail_amd_dbg.h, libneedletail_amd_dbg.so) beyond those every library is
held to (tests/test_consumer_abi.py): the struct fields of the binding and the model, the refusals that need no device, what of the
shared scaffold it uses and what it leaves alone, and the allocation arithmetic of the header's memory statement against the source."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _dbg_model as DM
import _libraries as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_dbg.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RULE_HPP = (os.path.join(CSRC, f) for f in ("ntk_dbg.hip", "ntk_dbg_rule.hpp"))
ROW = L.BY_NAME["dbg"]


def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


def test_header_compiles_as_c_and_states_the_struct_sizes(tmp_path):
    L.check_header(ROW, tmp_path)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    L.check_no_device(ROW)


def test_struct_fields_are_the_binding_and_the_model():
    from needletail_amd import dbg as D
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for struct, names in (("ntk_dbg_totals", [n for n, _ in D.Totals._fields_]), ("ntk_dbg_stats", [n for n, _ in D.Stats._fields_]),
                          ("ntk_dbg_unitig_row", list(D.UNITIG_COLUMNS)), ("ntk_dbg_kmer_row", list(D.KMER_COLUMNS))):
        body = re.search(r"struct %s \{(.*?)\};" % struct, hdr, re.S).group(1)
        fields = [re.sub(r"\[.*", "", f.strip()) for decl in re.findall(r"uint(?:64|32)_t ([^;]+);", body) for f in decl.split(",")]
        assert fields == names, struct
    assert tuple(n for n, _ in D.Totals._fields_) == DM.TOTALS
    assert C.sizeof(D.Totals) == 248 and C.sizeof(D.Stats) == 40   # the header's, which its C program states (tests/_libraries.py)
    assert (D.K_MIN, D.K_MAX, D.N_MAX, D.UNITIG_BYTES_PER_KMER, D.FLAG_CYCLE) == (3, 31, 2 ** 31 - 1, 96, 1)
    assert len(D.UNITIG_COLUMNS) * 8 == 32 and len(D.KMER_COLUMNS) * 4 == 8
    rule = open(RULE_HPP).read()
    assert "DBG_SUM_SELF = 25, DBG_SUM_LINKS = 26, DBG_N_SUMS = 27" in rule and "DBG_N_TOTALS = 31" in rule


def test_bad_k_and_a_forward_path_are_refused_before_any_device_is_looked_at():
    """NTK_ERR_BAD_K for k = 4, 1 and 33 from the library (checked before the context is used) and from KmerGraph; a PATH_BITS set
    is NTK_ERR_UNSUPPORTED."""
    import needletail_amd as nt
    from needletail_amd import dbg as D
    lib = D.lib()
    for k in (4, 1, 33, 0, 32):
        h = C.c_void_p()
        assert lib.ntk_dbg_create(C.c_void_p(8), k, C.byref(h)) == 1 and not h.value, k   # the context is never touched for such a k
    h = C.c_void_p()
    assert lib.ntk_dbg_create(None, 21, C.byref(h)) == 2
    assert lib.ntk_dbg_release(None) == 2 and lib.ntk_dbg_stats(None, None) == 2
    n = C.c_uint64(7)
    assert lib.ntk_dbg_adjacency_device(None, None, 0, None, None) == 2
    assert lib.ntk_dbg_unitigs_device(None, None, None, 0, None, None, 0, C.byref(n), C.byref(n)) == 2 and n.value == 7
    assert lib.ntk_dbg_spell_device(None, None, 0, None, None, 0, None, 0, None, 0, C.byref(n), C.byref(n)) == 2 and n.value == 7
    lib.ntk_dbg_destroy(None)
    ctx = object()   # never used: the refusal comes first
    for k in (4, 1, 33):
        with pytest.raises(nt.NtkError) as e:
            nt.KmerGraph(nt.KmerSet(None, None, 0, k, nt.PATH_BITS_CANONICAL, ctx))
        assert e.value.status == 1, k
    with pytest.raises(nt.NtkError) as e:
        nt.KmerGraph(nt.KmerSet(None, None, 0, 21, nt.PATH_BITS, ctx))
    assert e.value.status == 6
    with pytest.raises(TypeError):
        nt.KmerGraph([1, 2, 3])


def test_the_shared_pieces_are_used_and_not_defined_again():
    """Beyond the rule every library is held to: nothing is hashed, no inline assembly, no floating point."""
    src, rule = open(HIP).read(), open(RULE_HPP).read()
    for text in (src, rule):
        code = L.no_comments(text)
        assert not re.search(r"fmix64|0x9E3779B97F4A7C15|0xff51afd7ed558ccd", code), "this library hashes nothing"
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
        assert not re.search(r"\b(?:double|float)\b", code), "no floating point anywhere in the library"
    code = L.no_comments(src)
    for name in ("wave_sum", "add_agent", "grid_for", "with_tmp"):
        assert re.search(rf"\b{name}\(", code), name
    assert "h->bind(ctx, k, 0)" in src and "rocprim::exclusive_scan" in src and "rocprim::inclusive_scan" in src
    assert not re.search(r"needletail_amd_(?:count|wide_count|kmer_sets)\.h", src), "it never touches a table or another library"
    assert not re.search(r"atomic\w*\([^;]*counts", code), "no atomic per k-mer for the sums"


def test_allocation_arithmetic_is_the_headers_memory_statement():
    """The header's memory statement, term by term, against the allocation sizes in the source."""
    src, hdr = open(HIP).read(), open(HEADER).read()
    e = lambda arr, size: re.search(rf"h->{arr}\.ensure\(h->stream, {size}, grow_exact\)", src)   # noqa: E731
    # adjacency: the directory (4 B per entry), 1 B of edges and 2 * 4 B of targets per k-mer
    assert e("d_rdir", "words") and "const uint64_t words = dbg_dir_words(h->k, n);" in src and "DeviceArray<uint32_t> d_rdir;" in src
    assert e("d_edges", "n") and e("d_tgt", r"2 \* \(uint64_t\)n") and "DeviceArray<uint8_t> d_edges;" in src and "DeviceArray<uint32_t> d_tgt;" in src
    assert "4 B per entry" in hdr and "9 B per k-mer for adjacency" in hdr and "fewer than 2 n + 2 entries" in hdr
    for n in (1, 2, 3, 1000, 1024, 1025, 2 ** 31 - 1):
        for k in (3, 15, 31):
            b = min(2 * k, int(np.ceil(np.log2(n))) if n > 1 else 0)
            assert (1 << b) + 1 < 2 * n + 2
    # unitigs: per k-mer, 2 * 4 (next) + 2 * 2 * 8 (pointer and hops, two buffers) + 2 * 2 * 4 (smallest index, two buffers) + 8 (place)
    # + 4 (length) + 4 (order) + 16 (scan) + 8 (sums)
    assert e("d_next", "states") and e(r"d_pd\[q\]", "states") and e(r"d_mn\[q\]", "states") and "const uint64_t states = 2 * n;" in src
    assert e("d_place", "n") and e("d_len", "n") and e("d_perm", "n") and e("d_scan", r"n \+ 1") and e("d_prefix", r"n \+ 1")
    assert "DeviceArray<uint64_t> d_pd[2];" in src and "DeviceArray<uint32_t> d_mn[2];" in src and "DeviceArray<uint2> d_place;" in src
    assert "DeviceArray<ScanItem> d_scan;" in src and "uint64_t units, kmers;" in src
    per_kmer = 2 * 4 + 2 * 2 * 8 + 2 * 2 * 4 + 8 + 4 + 4 + 16 + 8
    assert per_kmer == 96 == int(re.search(r"#define NTK_DBG_UNITIG_BYTES_PER_KMER (\d+)u", hdr).group(1))
    # spell: 8 B per unitig
    assert e("d_offsets", r"n_unitigs \+ 1") and "8 B per\n * unitig for spell" in hdr
    # the flags of the rounds fit the small words: two passes of at most 32 rounds
    assert "kSmallWords = 128" in src and "kFlagAt = 32" in src and 32 + 2 * 33 + 2 <= 128
    # every array is released and counted
    arrays = set(re.findall(r"\b(d_[a-z_]+)(?:\[2\])?[;,]", re.search(r"struct ntk_dbg : Consumer \{(.*?)\n\};", src, re.S).group(1)))
    release = re.search(r"void release_scratch\(\)\s*\{(.*?)\n    \}", src, re.S).group(1)
    count = re.search(r"uint64_t device_bytes\(\) const\s*\{(.*?)\n    \}", src, re.S).group(1)
    for a in arrays:
        assert a in count, a
        assert a in release or a == "d_small", a
