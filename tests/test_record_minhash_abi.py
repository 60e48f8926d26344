"""CPU-side checks of the per-record MinHash library (include/needletail_amd_record_minhash.h, libneedletail_amd_record_minhash.so) beyond
the checks every library is held to (tests/test_consumer_abi.py): the loud error without a device next to the argument checks of create
that need none, what of the shared scaffold it uses, the wide byte walker neither named nor copied, and the constants of the header, the
sources, the binding and the model tied to each other."""
import ctypes as C
import os
import re

import _libraries as L
import _minhash_model as M
import _record_minhash_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_record_minhash.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RULE_HPP = (os.path.join(CSRC, f) for f in ("ntk_record_minhash.hip", "ntk_rmh_rule.hpp"))
BINDING = os.path.join(ROOT, "needletail_amd", "record_minhashing.py")
EXAMPLE = os.path.join(ROOT, "examples", "sketch_records.cpp")
STATS = ("n_records", "n_entries", "n_windows", "num", "scaled", "buffer_entries", "n_rounds", "n_retried_records", "n_redone",
         "device_bytes", "k", "path")
ERR_BAD_K, ERR_BAD_ARG = 1, 2
ROW = L.BY_NAME["record_minhash"]


def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


def test_header_compiles_as_c_and_includes_the_core_alone(tmp_path):
    L.check_header(ROW, tmp_path)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_struct_fields_and_constants_are_the_binding():
    from needletail_amd import minhashing
    from needletail_amd import record_minhashing as K
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"struct ntk_record_minhash_stats \{(.*?)\};", hdr, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"(?:uint64_t|uint32_t) ([^;]+);", body) for f in decl.split(",")]
    assert fields == [name for name, _ in K.Stats._fields_] == list(STATS)
    assert len(K.CALLS["read"]) == 7 and len(K.CALLS["run_device"]) == 7 and C.sizeof(K.Stats) == 88
    import needletail_amd as nt
    assert callable(nt.MinHashSet.add_record_sketches)
    define = lambda name: re.search(rf"#define NTK_RECORD_MINHASH_{name} (\S+(?: << \d+\))?)", text).group(1)
    shift = lambda s: 1 << int(re.fullmatch(r"\(1ull << (\d+)\)", s).group(1))
    assert int(define("XOR")[:-3], 16) == K.XOR == minhashing.XOR == M.XOR
    assert shift(define("MAX_NUM")) == K.MAX_NUM == minhashing.MAX_NUM == R.MAX_NUM
    assert int(define("ALLPASS")[:-3]) == K.ALLPASS == R.ALLPASS
    assert shift(define("BUFFER_DEFAULT")) == K.BUFFER_DEFAULT == R.BUFFER_DEFAULT
    assert int(define("BUFFER_MIN")[:-3]) == K.BUFFER_MIN == R.BUFFER_MIN
    assert shift(define("BUFFER_MAX")) == K.BUFFER_MAX == R.BUFFER_MAX
    src, rule = open(HIP).read(), open(RULE_HPP).read()
    assert int(re.search(r"kXor = (0x[0-9A-Fa-f]+)ull;", src).group(1), 16) == K.XOR
    assert re.search(r"record_minhash_hash\(uint64_t key\) \{ return fmix64\(key \^ kXor\); \}", src)
    assert int(re.search(r"kRmhAllPass = (\d+);", rule).group(1)) == K.ALLPASS
    assert "kTile = 64 * kPerLane;" in src and int(re.search(r"kPerLane = (\d+);", src).group(1)) * 64 == K.BUFFER_MIN
    assert "SYNCHRONOUS" in text, "the header says that the calls synchronise"


def test_no_device_is_a_loud_error_and_refused_arguments_need_none():
    """create checks its arguments before it looks for a device: those answers need no GPU.  Everything else is NTK_ERR_NO_DEVICE
    without one - a context cannot be made."""
    from needletail_amd import _lib as NL
    from needletail_amd import record_minhashing as K
    lib = K.lib()
    h = C.c_void_p()
    fake = C.c_void_p(16)   # never dereferenced: every case below is refused before the context is used
    create = lambda ctx, *a: lib.ntk_record_minhash_create(ctx, *a, C.byref(h))
    assert create(None, 21, 0, 16, 0, 0) == ERR_BAD_ARG and lib.ntk_record_minhash_create(fake, 21, 0, 16, 0, 0, None) == ERR_BAD_ARG
    assert create(fake, 0, 0, 16, 0, 0) == ERR_BAD_K and create(fake, 33, 0, 16, 0, 0) == ERR_BAD_K and create(fake, 63, 0, 16, 0, 0) == ERR_BAD_K
    assert create(fake, 33, 1, 16, 0, 0) == ERR_BAD_K and create(fake, 255, 2, 0, 7, 0) == ERR_BAD_K
    assert create(fake, 21, 3, 16, 0, 0) == ERR_BAD_ARG
    assert create(fake, 21, 0, 16, 7, 0) == ERR_BAD_ARG and create(fake, 21, 0, 0, 0, 0) == ERR_BAD_ARG
    assert create(fake, 21, 0, K.MAX_NUM + 1, 0, 0) == ERR_BAD_ARG
    assert create(fake, 21, 0, 16, 0, K.BUFFER_MIN - 1) == ERR_BAD_ARG and create(fake, 21, 0, 0, 7, K.BUFFER_MAX + 1) == ERR_BAD_ARG
    assert not h.value
    p = NL.Params(21, 0, 2, 0)
    n = C.c_uint64(0)
    assert lib.ntk_record_minhash_run_device(None, None, None, 0, None, 0, C.byref(p)) == ERR_BAD_ARG
    assert lib.ntk_record_minhash_read(None, None, None, None, None, 0, C.byref(n)) == ERR_BAD_ARG
    assert lib.ntk_record_minhash_stats(None, None) == ERR_BAD_ARG and lib.ntk_record_minhash_trim(None) == ERR_BAD_ARG
    lib.ntk_record_minhash_destroy(None)
    L.check_no_device(ROW, skip=False)   # (with a GPU the GPU tests take it from here)


def test_the_shared_pieces_are_used_and_not_defined_again():
    """Beyond the rule every library is held to: the chunk length is ntk_chunks.hpp's; the wide byte walker (k = 33..63, out of scope) is
    neither named - not even in a comment - nor copied; there is no inline assembly."""
    src = open(HIP).read()
    # rocPRIM's temporary storage grows with headroom (n + n/2 + 64), as every other array a run sizes: stats reports its bytes
    assert len(re.findall(r"\bwith_tmp\(", src)) == len(re.findall(r"\bwith_tmp\(m->tmp, st, grow_half_again, ", src)) == 5
    walker = "ntk_wide_" + "walk"
    for path in (HIP, RULE_HPP, HEADER, BINDING, EXAMPLE):
        text = open(path).read()
        assert walker not in text, path
        assert not re.search(r"walk_lane_run|kLaneRun|kPrime|hi_mask|rc_shift", text), (path, "a copy of the walker")
        assert not re.search(r"\basm\b|__asm", L.no_comments(text)), "plain HIP C++"
    assert not re.search(r"kChunkBases\s*=", src)
    assert "needletail_amd_minhash.h" not in src and "needletail_amd_minhash_set.h" not in src
    code = L.no_comments(src)
    for used in ("for_each_chunk(", "record_span(", "block_sum_u32(", "uniform(", "grid_for(", "check_batch_params(", "check_batch_pointers(",
                 "rmh_guess(", "rmh_accept(", "rmh_raise("):
        assert used in code, used
    assert re.search(r"kFilterThreads = 256;", src) and "__launch_bounds__(kFilterThreads)" in src
    # the filter's test is inclusive at both ends, and nothing pads the buffer
    assert "h >= hlo && h <= hhi" in src and "h >= rlo && h <= rhi" in src
