"""CPU-side checks of the k-mer sets library (include/needletail_amd_kmer_sets.h, libneedletail_amd_kmer_sets.so): exports, the C header,
the link to the core alone, the kernels it ships (each names the GPU test that launches it), no leak of them into the other nine
libraries, the loud error without a device, the shared scaffold used and not restated, and the constants of the header, the source,
the rule, the binding, the model and the GPU tests tied to each other."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _builds as B
import _kmer_sets_model as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "needletail_amd")
SO = os.path.join(LIBDIR, "libneedletail_amd_kmer_sets.so")
HEADER = os.path.join(ROOT, "include", "needletail_amd_kmer_sets.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RULE_HPP, CONSUMER = (os.path.join(CSRC, f) for f in ("ntk_kmer_sets.hip", "ntk_kset_rule.hpp", "ntk_consumer.hpp"))
# the memory layer of the scaffold (ntk_device_mem.hpp, which ntk_consumer.hpp includes): what it defines, and nobody else does
MEM = os.path.join(CSRC, "ntk_device_mem.hpp")
MEM_DEFS = (r"struct DeviceArray\b\s*\{", r"struct Pinned\b\s*\{", r"\bint\s+with_tmp\s*\(")
GPU_TESTS = "test_gpu_kmer_sets.py"
OTHER_LIBS = ("libneedletail_amd.so", "libneedletail_amd_count.so", "libneedletail_amd_wide_count.so", "libneedletail_amd_sketch.so",
              "libneedletail_amd_abundance.so", "libneedletail_amd_trim.so", "libneedletail_amd_minhash.so",
              "libneedletail_amd_minhash_set.so", "libneedletail_amd_record_minhash.so")
CALLS = ("create", "destroy", "release", "stats", "validate_device", "compare_device", "apply_device")

# every kernel of the library that is not rocPRIM's, with a GPU test that launches it: <key words, mode (0 COMPARE, 1 COUNT, 2 WRITE),
# LDS bins of the build>
_JOIN = "(anonymous namespace)::ks_join_kernel<{}, {}, {}u>((anonymous namespace)::JoinArgs)"
_SPLIT = "(anonymous namespace)::ks_split_kernel<{}>"
_VALIDATE = "(anonymous namespace)::ks_validate_kernel<{}>"
KERNELS = {
    _SPLIT.format(1): "test_lengths_around_the_tile_seams", _SPLIT.format(2): "test_lengths_around_the_tile_seams",
    _VALIDATE.format(1): "test_validate_counts_a_swapped_pair_and_a_duplicate",
    _VALIDATE.format(2): "test_validate_counts_a_swapped_pair_and_a_duplicate",
    _JOIN.format(1, 0, 4096): "test_lengths_around_the_tile_seams", _JOIN.format(2, 0, 4096): "test_lengths_around_the_tile_seams",
    _JOIN.format(1, 0, 16384): "test_counts_at_below_and_above_the_last_bin", _JOIN.format(2, 0, 16384): "test_key_edges_wide",
    _JOIN.format(1, 1, 1): "test_capacity_query_exact_fit_and_one_short", _JOIN.format(2, 1, 1): "test_capacity_query_exact_fit_and_one_short",
    _JOIN.format(1, 2, 1): "test_every_op_and_rule_on_random_lists", _JOIN.format(2, 2, 1): "test_every_op_and_rule_on_random_lists",
}


def _built():
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return SO


def _no_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_every_declared_function_is_exported_and_listed():
    from needletail_amd import kmer_sets
    lib = C.CDLL(_built())
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ntk_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted("ntk_kmer_sets_" + c for c in CALLS) and len(syms) == 7
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/needletail_amd_kmer_sets.h but not exported"
    assert sorted(kmer_sets.SYMBOLS) == syms and list(kmer_sets.CALLS) == list(CALLS)
    exported = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ntk_\w+)", exported))) == syms, "nothing else is exported under the project's prefix"
    import needletail_amd as nt
    assert nt.KmerSet is kmer_sets.KmerSet and "KmerSet" in nt.__all__


def test_header_compiles_as_c_and_includes_the_core_alone(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "needletail_amd_kmer_sets.h"\nint main(void) { struct ntk_kmer_sets_totals t; struct ntk_kmer_sets_stats s; '
                   "t.sum_max = NTK_KSET_MAX_BINS; s.n_calls = NTK_KSET_TILE_WORDS; "
                   "return t.sum_max == 16384 && s.n_calls == 2048 && sizeof t == 104 && sizeof s == 32 && NTK_KSET_INTERSECT == 1 && "
                   "NTK_KSET_UNION == 2 && NTK_KSET_SUBTRACT == 3 && NTK_KSET_COUNTERS_SUBTRACT == 4 && NTK_KSET_MIN == 1 && NTK_KSET_MAX == 2 && "
                   "NTK_KSET_SUM == 3 && NTK_KSET_LEFT == 4 && NTK_KSET_RIGHT == 5 ? 0 : 1; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HEADER).read()) == ["needletail_amd.h"]
    from needletail_amd import kmer_sets as K
    assert C.sizeof(K.Totals) == 104 and C.sizeof(K.Stats) == 32


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


def test_library_links_the_core_alone_by_rpath():
    out = subprocess.run(["readelf", "-d", _built()], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert "$ORIGIN" in out
    assert [n for n in needed if n.startswith("libneedletail_amd")] == ["libneedletail_amd.so"], needed
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KMER_SETS_OUT = \.\./libneedletail_amd_kmer_sets\.so$", make, re.M)
    assert re.search(r"^all:.*\$\(KMER_SETS_OUT\)", make, re.M) and re.search(r"rm -f.*\$\(KMER_SETS_OUT\) ntk_kmer_sets\.o", make)
    rule = re.search(r"^ntk_kmer_sets\.o:(.*)$", make, re.M).group(1)
    assert "ntk_kset_rule.hpp" in rule and "$(CONSUMER_HPP)" in rule and "needletail_amd_kmer_sets.h" in rule


def test_every_kernel_names_the_test_that_launches_it():
    names = B.library_kernels(_built())
    ours = {n for n in names if not n.startswith("rocprim::")}
    assert ours == set(KERNELS), sorted(ours ^ set(KERNELS))
    assert all(re.search(r"::ks_(?:split|join|validate)_kernel<", n) for n in ours)
    src = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    for sym, test in KERNELS.items():
        assert re.search(rf"^def {re.escape(test)}\(", src, re.M), (sym, test)
    # three kernels in the source, instantiated for both key widths; the join for its three modes and COMPARE's two bin builds
    assert len(re.findall(r"__global__", open(HIP).read())) == 3


def test_no_set_kernel_leaks_into_the_other_libraries():
    _built()
    for name in OTHER_LIBS:
        leaked = {n for n in B.library_kernels(os.path.join(LIBDIR, name)) if re.search(r"(?:^|::)ks_", n)}
        assert not leaked, (name, leaked)


def test_product_files_never_name_the_checker():
    for path in (HEADER, HIP, RULE_HPP, os.path.join(ROOT, "needletail_amd", "kmer_sets.py"),
                 os.path.join(ROOT, "examples", "compare_tables.cpp"), os.path.join(ROOT, "tools", "kmer_sets_bench.py")):
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
        nt.KmerSet.from_arrays([1, 2, 3], [1, 1, 1], 21)
    assert e.value.status == 4   # NTK_ERR_NO_DEVICE


def test_the_shared_pieces_are_used_and_not_defined_again():
    """The scaffold comes from ntk_consumer.hpp, nothing is hashed, there is no inline assembly and no floating point."""
    shared = ("fmix64", "wave_sum", "add_agent", "block_sum_u32", "grid_for", "alloc_status", "record_span", "uniform", "for_each_chunk")
    src, rule, consumer = open(HIP).read(), open(RULE_HPP).read(), open(CONSUMER).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_kset_rule.hpp"' in src
    for name in shared:
        assert re.search(rf"\b{name}\([^)]*\)\s*\{{", consumer), (name, "not defined in ntk_consumer.hpp")
        for text in (src, rule):
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", text), (name, "defined again")
    assert '#include "ntk_device_mem.hpp"' in consumer
    for pat in MEM_DEFS:
        assert len(re.findall(pat, open(MEM).read())) == 1, (pat, "not defined in ntk_device_mem.hpp")
        for text in (src, rule):
            assert not re.search(pat, text), (pat, "defined again")
    for text in (src, rule):
        assert not re.search(r"struct (?:MaterialiseScratch|Consumer)\b\s*\{", text)
        code = _no_comments(text)
        assert not re.search(r"fmix64|0x9E3779B97F4A7C15|0xff51afd7ed558ccd", code), "this library hashes nothing"
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
        assert not re.search(r"\b(?:double|float)\b", code), "no floating point anywhere in the library"
    code = _no_comments(src)
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
