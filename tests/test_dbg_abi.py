"""CPU-side checks of the de Bruijn graph library (include/needletail_amd_dbg.h, libneedletail_amd_dbg.so): exports, the C header and
its struct sizes, the link to the core alone, the kernels it ships (each names the GPU test that launches it), no leak of them into the
other ten libraries, the refusals that need no device, the shared scaffold used and not restated, and the allocation arithmetic of the
header's memory statement against the source."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _builds as B
import _dbg_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "needletail_amd")
SO = os.path.join(LIBDIR, "libneedletail_amd_dbg.so")
HEADER = os.path.join(ROOT, "include", "needletail_amd_dbg.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RULE_HPP, CONSUMER = (os.path.join(CSRC, f) for f in ("ntk_dbg.hip", "ntk_dbg_rule.hpp", "ntk_consumer.hpp"))
MEM_DEFS = (r"struct DeviceArray\b\s*\{", r"struct Pinned\b\s*\{", r"\bint\s+with_tmp\s*\(")
GPU_TESTS = "test_gpu_dbg.py"
OTHER_LIBS = ("libneedletail_amd.so", "libneedletail_amd_count.so", "libneedletail_amd_wide_count.so", "libneedletail_amd_sketch.so",
              "libneedletail_amd_abundance.so", "libneedletail_amd_trim.so", "libneedletail_amd_minhash.so",
              "libneedletail_amd_minhash_set.so", "libneedletail_amd_record_minhash.so", "libneedletail_amd_kmer_sets.so")
CALLS = ("create", "destroy", "release", "stats", "adjacency_device", "unitigs_device", "spell_device")

# every kernel of the library that is not rocPRIM's, with a GPU test that launches it
KERNELS = {
    "dbg_dir_mark_kernel": "test_directory_with_empty_buckets_and_with_one_bucket",
    "dbg_adjacency_kernel": "test_subsets_of_3_mers_and_5_mers",
    "dbg_link_kernel": "test_subsets_of_3_mers_and_5_mers",
    "dbg_rank_init_kernel": "test_a_long_path_needs_its_rounds",
    "dbg_rank_round_kernel": "test_a_long_path_needs_its_rounds",
    "dbg_rank_cut_kernel": "test_the_same_sequence_as_a_cycle",
    "dbg_resolve_kernel": "test_subsets_of_3_mers_and_5_mers",
    "dbg_perm_kernel": "test_subsets_of_3_mers_and_5_mers",
    "dbg_rows_kernel": "test_subsets_of_3_mers_and_5_mers",
    "dbg_spell_kernel": "test_subsets_of_3_mers_and_5_mers",
}


def _built():
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return SO


def _no_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_every_declared_function_is_exported_and_listed():
    from needletail_amd import dbg
    lib = C.CDLL(_built())
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ntk_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted("ntk_dbg_" + c for c in CALLS) and len(syms) == 7
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/needletail_amd_dbg.h but not exported"
    assert sorted(dbg.SYMBOLS) == syms and list(dbg.CALLS) == list(CALLS)
    exported = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ntk_\w+)", exported))) == syms, "nothing else is exported under the project's prefix"
    import needletail_amd as nt
    assert nt.KmerGraph is dbg.KmerGraph and "KmerGraph" in nt.__all__
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "dbg.lib()" in entry and '"examples", "unitigs.cpp"' in entry


def test_header_compiles_as_c_and_states_the_struct_sizes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "needletail_amd_dbg.h"\nint main(void) { struct ntk_dbg_totals t; struct ntk_dbg_stats s; struct ntk_dbg_kmer_row kr; '
                   "struct ntk_dbg_unitig_row ur; t.deg_hist[4][4] = NTK_DBG_K_MAX; s.n_rounds = NTK_DBG_K_MIN; kr.pos_flip = 1; ur.flags = NTK_DBG_FLAG_CYCLE; "
                   "return sizeof t == 248 && sizeof s == 40 && sizeof kr == 8 && sizeof ur == 32 && t.deg_hist[4][4] == 31 && s.n_rounds == 3 && "
                   "kr.pos_flip == ur.flags && NTK_DBG_N_MAX == 2147483647 && NTK_DBG_UNITIG_BYTES_PER_KMER == 96 ? 0 : 1; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HEADER).read()) == ["needletail_amd.h"]
    from needletail_amd import dbg as D
    assert C.sizeof(D.Totals) == 248 and C.sizeof(D.Stats) == 40
    assert (D.K_MIN, D.K_MAX, D.N_MAX, D.UNITIG_BYTES_PER_KMER, D.FLAG_CYCLE) == (3, 31, 2 ** 31 - 1, 96, 1)
    assert len(D.UNITIG_COLUMNS) * 8 == 32 and len(D.KMER_COLUMNS) * 4 == 8


def test_struct_fields_are_the_binding_and_the_model():
    from needletail_amd import dbg as D
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for struct, names in (("ntk_dbg_totals", [n for n, _ in D.Totals._fields_]), ("ntk_dbg_stats", [n for n, _ in D.Stats._fields_]),
                          ("ntk_dbg_unitig_row", list(D.UNITIG_COLUMNS)), ("ntk_dbg_kmer_row", list(D.KMER_COLUMNS))):
        body = re.search(r"struct %s \{(.*?)\};" % struct, hdr, re.S).group(1)
        fields = [re.sub(r"\[.*", "", f.strip()) for decl in re.findall(r"uint(?:64|32)_t ([^;]+);", body) for f in decl.split(",")]
        assert fields == names, struct
    assert tuple(n for n, _ in D.Totals._fields_) == DM.TOTALS
    rule = open(RULE_HPP).read()
    assert "DBG_SUM_SELF = 25, DBG_SUM_LINKS = 26, DBG_N_SUMS = 27" in rule and "DBG_N_TOTALS = 31" in rule


def test_library_links_the_core_alone_by_rpath():
    out = subprocess.run(["readelf", "-d", _built()], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert "$ORIGIN" in out
    assert [n for n in needed if n.startswith("libneedletail_amd")] == ["libneedletail_amd.so"], needed
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^DBG_OUT = \.\./libneedletail_amd_dbg\.so$", make, re.M)
    assert re.search(r"^all:.*\$\(DBG_OUT\)", make, re.M) and re.search(r"rm -f.*\$\(DBG_OUT\) ntk_dbg\.o", make)
    rule = re.search(r"^ntk_dbg\.o:(.*)$", make, re.M).group(1)
    assert "ntk_dbg_rule.hpp" in rule and "$(CONSUMER_HPP)" in rule and "needletail_amd_dbg.h" in rule


def test_every_kernel_names_the_test_that_launches_it():
    names = B.library_kernels(_built())
    ours = {re.sub(r"^\(anonymous namespace\)::", "", n).split("(")[0] for n in names if not n.startswith("rocprim::")}
    assert ours == set(KERNELS), sorted(ours ^ set(KERNELS))
    src = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    for sym, test in KERNELS.items():
        assert re.search(rf"^def {re.escape(test)}\(", src, re.M), (sym, test)
    assert len(re.findall(r"__global__", open(HIP).read())) == len(KERNELS)


def test_no_graph_kernel_leaks_into_the_other_libraries():
    _built()
    for name in OTHER_LIBS:
        leaked = {n for n in B.library_kernels(os.path.join(LIBDIR, name)) if re.search(r"(?:^|::)dbg_", n)}
        assert not leaked, (name, leaked)


def test_product_files_never_name_the_checker():
    for path in (HEADER, HIP, RULE_HPP, os.path.join(ROOT, "needletail_amd", "dbg.py"), os.path.join(ROOT, "examples", "unitigs.cpp"),
                 os.path.join(ROOT, "tools", "dbg_bench.py")):
        txt = open(path).read()
        assert not re.search(r"\boracle\b|ntko_", txt), path


def test_no_device_is_a_loud_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import needletail_amd as nt
    from needletail_amd import engine
    engine._default_ctx = None
    with pytest.raises(nt.NtkError) as e:
        nt.KmerGraph(nt.KmerSet.from_arrays([1, 2, 3], [1, 1, 1], 21))
    assert e.value.status == 4   # NTK_ERR_NO_DEVICE


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
    """The scaffold comes from ntk_consumer.hpp, memory from ntk_device_mem.hpp; nothing is hashed, no inline assembly, no floating point."""
    shared = ("fmix64", "wave_sum", "add_agent", "block_sum_u32", "grid_for", "alloc_status", "record_span", "uniform", "for_each_chunk")
    src, rule, consumer = open(HIP).read(), open(RULE_HPP).read(), open(CONSUMER).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_dbg_rule.hpp"' in src
    for name in shared:
        for text in (src, rule):
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", text), (name, "defined again")
    assert '#include "ntk_device_mem.hpp"' in consumer
    for text in (src, rule):
        for pat in MEM_DEFS:
            assert not re.search(pat, text), (pat, "defined again")
        assert not re.search(r"struct (?:MaterialiseScratch|Consumer)\b\s*\{", text)
        code = _no_comments(text)
        assert not re.search(r"fmix64|0x9E3779B97F4A7C15|0xff51afd7ed558ccd", code), "this library hashes nothing"
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
        assert not re.search(r"\b(?:double|float)\b", code), "no floating point anywhere in the library"
        assert not re.search(r"hip(?:Host)?(?:Malloc|Free)\b", text), "the memory layer allocates"
    code = _no_comments(src)
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
