"""CPU-side checks of the k-mer sets library (include/needletail_amd_kmer_sets.h, libneedletail_amd_kmer_sets.so) beyond those every library
is held to (tests/test_consumer_abi.py): the struct fields of the binding and the model, what of the shared scaffold it uses and what it
leaves alone, and the constants of the header, the source, the rule, the binding, the model and the GPU tests tied to each other."""
import ctypes as C
import os
import re

import _kmer_sets_model as KM
import _libraries as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_kmer_sets.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RULE_HPP = (os.path.join(CSRC, f) for f in ("ntk_kmer_sets.hip", "ntk_kset_rule.hpp"))
GPU_TESTS = "test_gpu_kmer_sets.py"
ROW = L.BY_NAME["kmer_sets"]


def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


def test_header_compiles_as_c_and_includes_the_core_alone(tmp_path):
    L.check_header(ROW, tmp_path)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    L.check_no_device(ROW)


def test_struct_fields_are_the_binding_and_the_model():
    from needletail_amd import kmer_sets as K
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for struct, binding in (("ntk_kmer_sets_totals", K.Totals), ("ntk_kmer_sets_stats", K.Stats)):
        body = re.search(r"struct %s \{(.*?)\};" % struct, hdr, re.S).group(1)
        fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]+);", body) for f in decl.split(",")]
        assert fields == [name for name, _ in binding._fields_], struct
        assert all(t is C.c_uint64 for _, t in binding._fields_)
    assert tuple(name for name, _ in K.Totals._fields_) == KM.TOTALS
    assert len(K.CALLS["compare_device"]) == 11 and len(K.CALLS["apply_device"]) == 13
    assert C.sizeof(K.Totals) == 104 and C.sizeof(K.Stats) == 32


def test_the_shared_pieces_are_used_and_not_defined_again():
    """Beyond the rule every library is held to: nothing is hashed, there is no inline assembly and no floating point."""
    src, rule = open(HIP).read(), open(RULE_HPP).read()
    for text in (src, rule):
        code = L.no_comments(text)
        assert not re.search(r"fmix64|0x9E3779B97F4A7C15|0xff51afd7ed558ccd", code), "this library hashes nothing"
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
        assert not re.search(r"\b(?:double|float)\b", code), "no floating point anywhere in the library"
    code = L.no_comments(src)
    for name in ("wave_sum", "add_agent", "block_sum_u32", "grid_for", "with_tmp"):   # (alloc_status is used by the memory layer now)
        assert re.search(rf"\b{name}\(", code), name
    assert "h->bind(ctx, 0, 0)" in src and "rocprim::exclusive_scan" in src
    assert not re.search(r"needletail_amd_(?:count|wide_count)\.h", src), "it never touches a table"


def test_constants_agree_everywhere():
    from needletail_amd import kmer_sets as K
    hdr, src, rule = open(HEADER).read(), open(HIP).read(), open(RULE_HPP).read()
    gpu_tests = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    tile = int(re.search(r"#define NTK_KSET_TILE_WORDS (\d+)\b", hdr).group(1))
    assert tile == int(re.search(r"kTileWords = (\d+);", src).group(1)) == K.TILE_WORDS == KM.TILE_WORDS == 2048
    assert re.search(r"kTileOf = kTileWords / KW;", src) and re.search(r"tile = kTileWords / h->kw;", src)
    assert re.search(r"^TILE = \{1: KM\.TILE_WORDS, 2: KM\.TILE_WORDS // 2\}", gpu_tests, re.M)
    bins = int(re.search(r"#define NTK_KSET_MAX_BINS (\d+)\b", hdr).group(1))
    assert bins == int(re.search(r"kBinsBig = (\d+);", src).group(1)) == K.MAX_BINS == KM.MAX_BINS == 16384
    ops = {name: int(v) for name, v in re.findall(r"#define NTK_KSET_([A-Z_]+) (\d+)u", hdr)}
    assert ops == {"INTERSECT": 1, "UNION": 2, "SUBTRACT": 3, "COUNTERS_SUBTRACT": 4, "MIN": 1, "MAX": 2, "SUM": 3, "LEFT": 4, "RIGHT": 5}
    for name, v in ops.items():
        assert getattr(K, name) == v == getattr(KM, name)
        assert re.search(rf"\bKS_{name} = {v}\b", rule), name
    assert K.RULES == {"min": 1, "max": 2, "sum": 3, "left": 4, "right": 5}
    # a block's u32 bins: at most 2^20 tiles of at most 2^11 elements
    assert int(re.search(r"kMaxTilesPerBlock = \(uint64_t\)1 << (\d+);", src).group(1)) + 11 < 32
