"""CPU-side checks of the sketch-set library (include/needletail_amd_minhash_set.h, libneedletail_amd_minhash_set.so) beyond those every
library is held to (tests/test_consumer_abi.py): the struct fields of the binding, what of the shared scaffold it uses and what it
leaves alone, and the constants of the header, the source, the binding, the model and the GPU tests tied to each other."""
import ctypes as C
import os
import re

import _libraries as L
import _mhset_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_minhash_set.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RANK_HPP = (os.path.join(CSRC, f) for f in ("ntk_minhash_set.hip", "ntk_mhset_rank.hpp"))
GPU_TESTS = "test_gpu_minhash_set.py"
ROW = L.BY_NAME["minhash_set"]


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


def test_struct_fields_are_the_binding():
    from needletail_amd import minhash_sets as K
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct ntk_mhset_stats \{(.*?)\};", hdr, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"(?:uint64_t|uint32_t|double) ([^;]+);", body) for f in decl.split(",")]
    assert fields == [name for name, _ in K.Stats._fields_]
    assert fields == ["n_sketches", "n_entries", "abundance", "block_pairs", "device_bytes", "n_launches", "n_uploads"]
    assert all(t is C.c_uint64 for _, t in K.Stats._fields_)
    # the compare call: two handles with their ranges, num and max_hash, five matrices and two vectors
    assert len(K.CALLS["compare"]) == 15 and C.sizeof(K.Stats) == 56


def test_the_shared_pieces_are_used_and_not_defined_again():
    """Beyond the rule every library is held to: the hash is not restated (this library never hashes), the byte walker is not included,
    and there is no inline assembly."""
    src, rank = open(HIP).read(), open(RANK_HPP).read()
    for text in (src, rank):
        assert "ntk_wide_walk.hpp" not in text and "needletail_amd_minhash.h" not in text
        code = L.no_comments(text)
        assert not re.search(r"fmix64|0x9E3779B97F4A7C15|0xff51afd7ed558ccd|kXor", code), "the hash is somebody else's"
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
    assert re.search(r"\bwave_sum\(", L.no_comments(src)) and re.search(r"\buniform\(", L.no_comments(src)) and "grid_for(" in src


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
