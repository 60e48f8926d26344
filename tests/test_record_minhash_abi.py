"""CPU-side checks of the per-record MinHash library (include/needletail_amd_record_minhash.h, libneedletail_amd_record_minhash.so):
exports, the C header, the link to the core alone, the kernels it ships (each names the test that launches it), the loud error without
a device, the argument checks of create that need none, the shared scaffold used and not restated, the wide byte walker neither named
nor copied, and the constants of the header, the sources, the binding and the model tied to each other."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _builds as B
import _minhash_model as M
import _record_minhash_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "needletail_amd")
SO = os.path.join(LIBDIR, "libneedletail_amd_record_minhash.so")
HEADER = os.path.join(ROOT, "include", "needletail_amd_record_minhash.h")
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
HIP, RULE_HPP, CONSUMER = (os.path.join(CSRC, f) for f in ("ntk_record_minhash.hip", "ntk_rmh_rule.hpp", "ntk_consumer.hpp"))
# the memory layer of the scaffold (ntk_device_mem.hpp, which ntk_consumer.hpp includes): what it defines, and nobody else does
MEM = os.path.join(CSRC, "ntk_device_mem.hpp")
MEM_DEFS = (r"struct DeviceArray\b\s*\{", r"struct Pinned\b\s*\{", r"\bint\s+with_tmp\s*\(")
BINDING = os.path.join(ROOT, "needletail_amd", "record_minhashing.py")
EXAMPLE = os.path.join(ROOT, "examples", "sketch_records.cpp")
GPU_TESTS = "test_gpu_record_minhash.py"
OTHER_LIBS = ("libneedletail_amd.so", "libneedletail_amd_count.so", "libneedletail_amd_wide_count.so", "libneedletail_amd_sketch.so",
              "libneedletail_amd_abundance.so", "libneedletail_amd_trim.so", "libneedletail_amd_minhash.so", "libneedletail_amd_minhash_set.so")
CALLS = ("create", "destroy", "run_device", "read", "stats", "trim")
STATS = ("n_records", "n_entries", "n_windows", "num", "scaled", "buffer_entries", "n_rounds", "n_retried_records", "n_redone",
         "device_bytes", "k", "path")
ERR_BAD_K, ERR_BAD_ARG, ERR_NO_DEVICE = 1, 2, 4

# every kernel of the library with the test that launches it
KERNELS = {
    "rmh_filter_kernel": "test_random_records_match_the_model",
    "rmh_windows_kernel": "test_random_records_match_the_model",
    "rmh_retry_kernel": "test_repetitive_records_are_retried_until_exact",
    "rmh_accept_kernel": "test_repetitive_records_are_retried_until_exact",
    "rmh_iota_kernel": "test_random_records_match_the_model",
    "rmh_gather_rec_kernel": "test_random_records_match_the_model",
    "rmh_heads_kernel": "test_random_records_match_the_model",
    "rmh_groups_kernel": "test_random_records_match_the_model",
    "rmh_segments_kernel": "test_random_records_match_the_model",
    "rmh_keep_kernel": "test_random_records_match_the_model",
}


def _built():
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return SO


def _no_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_every_declared_function_is_exported_and_listed():
    """The contract's calls - create, destroy, run_device, read, stats, trim - and nothing else."""
    from needletail_amd import record_minhashing
    lib = C.CDLL(_built())
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ntk_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted("ntk_record_minhash_" + c for c in CALLS)
    assert len(syms) == 6
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/needletail_amd_record_minhash.h but not exported"
    assert sorted(record_minhashing.SYMBOLS) == syms
    exported = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ntk_\w+)", exported))) == syms, "nothing else is exported under the project's prefix"
    import needletail_amd as nt
    assert nt.RecordMinHash is record_minhashing.RecordMinHash and "RecordMinHash" in nt.__all__
    assert callable(nt.MinHashSet.add_record_sketches)


def test_header_compiles_as_c_and_includes_the_core_alone(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "needletail_amd_record_minhash.h"\nint main(void) { struct ntk_record_minhash_stats s; s.n_records = '
                   "NTK_RECORD_MINHASH_BUFFER_MAX; return s.n_records == 1073741824 && sizeof s == 88 && NTK_RECORD_MINHASH_ALLPASS == 4 && "
                   "NTK_RECORD_MINHASH_BUFFER_DEFAULT == 16777216 && NTK_RECORD_MINHASH_BUFFER_MIN == 256 && "
                   "NTK_RECORD_MINHASH_MAX_NUM == 1048576 && NTK_RECORD_MINHASH_XOR == 0x9E3779B97F4A7C15ull ? 0 : 1; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HEADER).read()) == ["needletail_amd.h"]
    from needletail_amd import record_minhashing as K
    assert C.sizeof(K.Stats) == 88


def test_struct_fields_and_constants_are_the_binding():
    from needletail_amd import minhashing
    from needletail_amd import record_minhashing as K
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"struct ntk_record_minhash_stats \{(.*?)\};", hdr, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"(?:uint64_t|uint32_t) ([^;]+);", body) for f in decl.split(",")]
    assert fields == [name for name, _ in K.Stats._fields_] == list(STATS)
    assert list(K.CALLS) == list(CALLS) and len(K.CALLS["read"]) == 7 and len(K.CALLS["run_device"]) == 7
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


def test_library_links_the_core_alone_by_rpath():
    out = subprocess.run(["readelf", "-d", _built()], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert "$ORIGIN" in out
    assert [n for n in needed if n.startswith("libneedletail_amd")] == ["libneedletail_amd.so"], needed
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^RECORD_MINHASH_OUT = \.\./libneedletail_amd_record_minhash\.so$", make, re.M)
    assert re.search(r"^all:.*\$\(RECORD_MINHASH_OUT\)", make, re.M) and re.search(r"rm -f.*\$\(RECORD_MINHASH_OUT\) ntk_record_minhash\.o", make)
    rule = re.search(r"^ntk_record_minhash\.o:(.*)$", make, re.M).group(1)
    assert "ntk_rmh_rule.hpp" in rule and "$(CONSUMER_HPP)" in rule and "needletail_amd_record_minhash.h" in rule
    link = re.search(r"^\$\(RECORD_MINHASH_OUT\):.*\n\t(.*)$", make, re.M).group(1)
    assert re.findall(r"-l(\S+)", link) == ["needletail_amd"]


def test_every_kernel_names_the_test_that_launches_it():
    names = B.library_kernels(_built())
    ours = {n for n in names if not n.startswith("rocprim::")}
    short = {re.search(r"::(rmh_[a-z_]+_kernel)\b", n).group(1) for n in ours}
    assert short == set(KERNELS) and len(ours) == len(KERNELS), sorted(ours)
    prim = names - ours   # the fold's two sorts and three scans
    assert any("sort" in n for n in prim) and any("scan" in n for n in prim)
    src = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    for kernel, test in KERNELS.items():
        assert re.search(rf"^def {re.escape(test)}\(", src, re.M), (kernel, test)
    assert len(re.findall(r"__global__", open(HIP).read())) == len(KERNELS)


def test_no_kernel_leaks_into_the_other_libraries():
    _built()
    for name in OTHER_LIBS:
        leaked = {n for n in B.library_kernels(os.path.join(LIBDIR, name)) if re.search(r"(?:^|::)rmh_", n)}
        assert not leaked, (name, leaked)


def test_product_files_never_name_the_checker():
    for path in (HEADER, HIP, RULE_HPP, BINDING, EXAMPLE, os.path.join(ROOT, "tools", "record_minhash_bench.py")):
        txt = open(path).read()
        assert not re.search(r"\boracle\b|ntko_", txt), path


def test_no_device_is_a_loud_error_and_refused_arguments_need_none():
    """create checks its arguments before it looks for a device: those answers need no GPU.  Everything else is NTK_ERR_NO_DEVICE
    without one - a context cannot be made."""
    import torch
    import needletail_amd as nt
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
    if torch.cuda.is_available():
        return   # (the GPU tests take it from here)
    from needletail_amd import engine
    engine._default_ctx = None
    with pytest.raises(nt.NtkError) as e:
        nt.RecordMinHash(21, nt.PATH_BYTES_CANONICAL, num=16)
    assert e.value.status == ERR_NO_DEVICE


def test_the_shared_pieces_are_used_and_not_defined_again():
    """The scaffold comes from ntk_consumer.hpp, the chunk length from ntk_chunks.hpp, the rule from ntk_rmh_rule.hpp; the wide byte walker
    (k = 33..63, out of scope) is neither named - not even in a comment - nor copied; there is no inline assembly."""
    shared = ("fmix64", "wave_sum", "add_agent", "block_sum_u32", "grid_for", "alloc_status", "record_span", "uniform", "for_each_chunk")
    src, rule, consumer = open(HIP).read(), open(RULE_HPP).read(), open(CONSUMER).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_rmh_rule.hpp"' in src
    for name in shared:
        assert re.search(rf"\b{name}\([^)]*\)\s*\{{", consumer), (name, "not defined in ntk_consumer.hpp")
        for text in (src, rule):
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", text), (name, "defined again")
    assert '#include "ntk_device_mem.hpp"' in consumer
    # rocPRIM's temporary storage grows with headroom (n + n/2 + 64), as every other array a run sizes: stats reports its bytes
    assert len(re.findall(r"\bwith_tmp\(", src)) == len(re.findall(r"\bwith_tmp\(m->tmp, st, grow_half_again, ", src)) == 5
    for pat in MEM_DEFS:
        assert len(re.findall(pat, open(MEM).read())) == 1, (pat, "not defined in ntk_device_mem.hpp")
        for text in (src, rule):
            assert not re.search(pat, text), (pat, "defined again")
    walker = "ntk_wide_" + "walk"
    for path in (HIP, RULE_HPP, HEADER, BINDING, EXAMPLE):
        text = open(path).read()
        assert walker not in text, path
        assert not re.search(r"walk_lane_run|kLaneRun|kPrime|hi_mask|rc_shift", text), (path, "a copy of the walker")
        assert not re.search(r"\basm\b|__asm", _no_comments(text)), "plain HIP C++"
    assert not re.search(r"struct (?:MaterialiseScratch|Consumer)\b\s*\{", src) and not re.search(r"kChunkBases\s*=", src)
    assert "needletail_amd_minhash.h" not in src and "needletail_amd_minhash_set.h" not in src
    code = _no_comments(src)
    for used in ("for_each_chunk(", "record_span(", "block_sum_u32(", "uniform(", "grid_for(", "check_batch_params(", "check_batch_pointers(",
                 "rmh_guess(", "rmh_accept(", "rmh_raise("):
        assert used in code, used
    assert re.search(r"kFilterThreads = 256;", src) and "__launch_bounds__(kFilterThreads)" in src
    # the filter's test is inclusive at both ends, and nothing pads the buffer
    assert "h >= hlo && h <= hhi" in src and "h >= rlo && h <= rhi" in src
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "record_minhashing.lib()" in entry and "sketch_records" in entry
    assert "examples/sketch_records" in open(os.path.join(ROOT, ".gitignore")).read().split()
