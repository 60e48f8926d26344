"""CPU-side checks of the sketch-set library (include/needletail_amd_minhash_set.h, libneedletail_amd_minhash_set.so): exports, the C
header, the link to the core alone, the two kernels it ships (each names the test that launches it), no leak of them into the other
seven libraries, the loud error without a device, the shared scaffold used and not restated, and the constants of the header, the
source, the binding, the model and the GPU tests tied to each other."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _builds as B
import _mhset_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "needletail_amd")
SO = os.path.join(LIBDIR, "libneedletail_amd_minhash_set.so")
HEADER = os.path.join(ROOT, "include", "needletail_amd_minhash_set.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RANK_HPP, CONSUMER = (os.path.join(CSRC, f) for f in ("ntk_minhash_set.hip", "ntk_mhset_rank.hpp", "ntk_consumer.hpp"))
# the memory layer of the scaffold (ntk_device_mem.hpp, which ntk_consumer.hpp includes): what it defines, and nobody else does
MEM = os.path.join(CSRC, "ntk_device_mem.hpp")
MEM_DEFS = (r"struct DeviceArray\b\s*\{", r"struct Pinned\b\s*\{", r"\bint\s+with_tmp\s*\(")
GPU_TESTS = "test_gpu_minhash_set.py"
OTHER_LIBS = ("libneedletail_amd.so", "libneedletail_amd_count.so", "libneedletail_amd_wide_count.so", "libneedletail_amd_sketch.so",
              "libneedletail_amd_abundance.so", "libneedletail_amd_trim.so", "libneedletail_amd_minhash.so")
CALLS = ("create", "destroy", "reset", "add", "read", "stats", "compare")

# every kernel of the library with the test that launches it
SET_KERNELS = {
    "(anonymous namespace)::ms_cut_kernel((anonymous namespace)::CutArgs)": "test_block_matches_the_host_compare",
    "(anonymous namespace)::ms_pair_kernel((anonymous namespace)::PairArgs)": "test_block_matches_the_host_compare",
}


def _built():
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return SO


def _no_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_every_declared_function_is_exported_and_listed():
    from needletail_amd import minhash_sets
    lib = C.CDLL(_built())
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ntk_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted("ntk_mhset_" + c for c in CALLS) and len(syms) == 7
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/needletail_amd_minhash_set.h but not exported"
    assert sorted(minhash_sets.SYMBOLS) == syms
    exported = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ntk_\w+)", exported))) == syms, "nothing else is exported under the project's prefix"
    import needletail_amd as nt
    assert nt.MinHashSet is minhash_sets.MinHashSet and "MinHashSet" in nt.__all__


def test_header_compiles_as_c_and_includes_the_core_alone(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "needletail_amd_minhash_set.h"\nint main(void) { struct ntk_mhset_stats s; s.n_sketches = NTK_MHSET_BLOCK_MAX; '
                   "return s.n_sketches == 67108864 && sizeof s == 56 && sizeof(struct ntk_mhset_stats) == 56 && "
                   "NTK_MHSET_BLOCK_DEFAULT == 1048576 && NTK_MHSET_BLOCK_MIN == 1 && NTK_MHSET_STAGE == 2048 ? 0 : 1; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HEADER).read()) == ["needletail_amd.h"]
    from needletail_amd import minhash_sets as K
    assert C.sizeof(K.Stats) == 56


def test_struct_fields_are_the_binding():
    from needletail_amd import minhash_sets as K
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct ntk_mhset_stats \{(.*?)\};", hdr, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"(?:uint64_t|uint32_t|double) ([^;]+);", body) for f in decl.split(",")]
    assert fields == [name for name, _ in K.Stats._fields_]
    assert fields == ["n_sketches", "n_entries", "abundance", "block_pairs", "device_bytes", "n_launches", "n_uploads"]
    assert all(t is C.c_uint64 for _, t in K.Stats._fields_)
    # the compare call: two handles with their ranges, num and max_hash, five matrices and two vectors
    assert len(K.CALLS["compare"]) == 15 and list(K.CALLS) == list(CALLS)


def test_library_links_the_core_alone_by_rpath():
    out = subprocess.run(["readelf", "-d", _built()], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert "$ORIGIN" in out
    assert [n for n in needed if n.startswith("libneedletail_amd")] == ["libneedletail_amd.so"], needed
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^MINHASH_SET_OUT = \.\./libneedletail_amd_minhash_set\.so$", make, re.M)
    assert re.search(r"^all:.*\$\(MINHASH_SET_OUT\)", make, re.M) and re.search(r"rm -f.*\$\(MINHASH_SET_OUT\) ntk_minhash_set\.o", make)


def test_every_kernel_names_the_test_that_launches_it():
    names = B.library_kernels(_built())
    ours = {n for n in names if not n.startswith("rocprim::")}
    assert ours == set(SET_KERNELS), sorted(ours ^ set(SET_KERNELS))
    assert all(re.search(r"::ms_(?:cut|pair)_kernel\(", n) for n in ours)
    assert not any(re.search(r"(?:^|::)mh_|minhash", n) for n in names), "the MinHash library's ABI test greps the other libraries for these"
    src = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    for sym, test in SET_KERNELS.items():
        assert re.search(rf"^def {re.escape(test)}\(", src, re.M), (sym, test)


def test_no_set_kernel_leaks_into_the_other_libraries():
    _built()
    for name in OTHER_LIBS:
        leaked = {n for n in B.library_kernels(os.path.join(LIBDIR, name)) if re.search(r"(?:^|::)ms_", n)}
        assert not leaked, (name, leaked)


def test_product_files_never_name_the_checker():
    for path in (HEADER, HIP, RANK_HPP, os.path.join(ROOT, "needletail_amd", "minhash_sets.py"),
                 os.path.join(ROOT, "examples", "minhash_matrix.cpp"), os.path.join(ROOT, "tools", "minhash_set_bench.py")):
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
        nt.MinHashSet()
    assert e.value.status == 4   # NTK_ERR_NO_DEVICE


def test_the_shared_pieces_are_used_and_not_defined_again():
    """The rule tests/test_count_abi.py holds the other six sources to, for this one: the scaffold comes from ntk_consumer.hpp, the hash
    is not restated (this library never hashes), the byte walker is not included, and there is no inline assembly."""
    shared = ("fmix64", "wave_sum", "add_agent", "block_sum_u32", "grid_for", "alloc_status", "record_span", "uniform", "for_each_chunk")
    src, rank, consumer = open(HIP).read(), open(RANK_HPP).read(), open(CONSUMER).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_mhset_rank.hpp"' in src
    for name in shared:
        assert re.search(rf"\b{name}\([^)]*\)\s*\{{", consumer), (name, "not defined in ntk_consumer.hpp")
        for text in (src, rank):
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", text), (name, "defined again")
    assert '#include "ntk_device_mem.hpp"' in consumer
    for pat in MEM_DEFS:
        assert len(re.findall(pat, open(MEM).read())) == 1, (pat, "not defined in ntk_device_mem.hpp")
        for text in (src, rank):
            assert not re.search(pat, text), (pat, "defined again")
    for text in (src, rank):
        assert not re.search(r"struct (?:MaterialiseScratch|Consumer)\b\s*\{", text)
        assert "ntk_wide_walk.hpp" not in text and "needletail_amd_minhash.h" not in text
        code = _no_comments(text)
        assert not re.search(r"fmix64|0x9E3779B97F4A7C15|0xff51afd7ed558ccd|kXor", code), "the hash is somebody else's"
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
    assert re.search(r"\bwave_sum\(", _no_comments(src)) and re.search(r"\buniform\(", _no_comments(src)) and "grid_for(" in src
    assert len(re.findall(r"__global__", src)) == 2
    make = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^ntk_minhash_set\.o:(.*)$", make, re.M).group(1)
    assert "ntk_mhset_rank.hpp" in rule and "$(CONSUMER_HPP)" in rule and "needletail_amd_minhash_set.h" in rule


def test_constants_agree_everywhere():
    from needletail_amd import minhash_sets as K
    hdr, src = open(HEADER).read(), open(HIP).read()
    gpu_tests = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    stage = int(re.search(r"#define NTK_MHSET_STAGE (\d+)\b", hdr).group(1))
    assert stage == int(re.search(r"kStage = (\d+);", src).group(1)) == K.STAGE == SM.STAGE
    assert stage == int(re.search(r"^STAGE = (\d+)\b", gpu_tests, re.M).group(1))
    assert re.search(r"__shared__ uint64_t stage\[kStage\];", src) and re.search(r"staged = nb <= kStage;", src)
    default = 1 << int(re.search(r"#define NTK_MHSET_BLOCK_DEFAULT \(1ull << (\d+)\)", hdr).group(1))
    assert default == (1 << int(re.search(r"kBlockDefault = \(uint64_t\)1 << (\d+);", src).group(1))) == K.BLOCK_DEFAULT == SM.BLOCK_DEFAULT
    assert int(re.search(r"#define NTK_MHSET_BLOCK_MIN (\d+)ull", hdr).group(1)) == K.BLOCK_MIN == SM.BLOCK_MIN == 1
    assert 1 << int(re.search(r"#define NTK_MHSET_BLOCK_MAX \(1ull << (\d+)\)", hdr).group(1)) == K.BLOCK_MAX == SM.BLOCK_MAX
    assert int(re.search(r"kResultBytes = (\d+);", src).group(1)) == 32 and "block_pairs * 32 B" in hdr
    assert int(re.search(r"kPairThreads = (\d+);", src).group(1)) == int(re.search(r"^PAIR_THREADS = (\d+)\b", gpu_tests, re.M).group(1))
    assert K.MATRICES == SM.MATRICES
