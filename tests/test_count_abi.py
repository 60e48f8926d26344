"""CPU-side checks of the count library (include/needletail_amd_count.h, libneedletail_amd_count.so) beyond those every library is held to
(tests/test_consumer_abi.py): the core entry it needs, the shared pieces defined once across all the libraries, who allocates, and the
host model of the table (tests/_count_model.py) with its constants tied to the kernel source."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _count_model as M
import _libraries as L

CSRC, CORE = L.CSRC, L.CORE_SO
HIP = L.BY_NAME["count"].hip
COMMON = os.path.join(CSRC, "ntk_count_common.hpp")   # what the narrow and the wide table share
CONSUMER = os.path.join(CSRC, "ntk_consumer.hpp")     # what every library on the core's ABI shares
CHUNKS = os.path.join(CSRC, "ntk_chunks.hpp")         # the chunk geometry
# the memory layer of the scaffold (ntk_device_mem.hpp, which ntk_consumer.hpp includes): what it defines, and nobody else does
MEM = os.path.join(CSRC, "ntk_device_mem.hpp")
MEM_DEFS = (r"struct DeviceArray\b\s*\{", r"struct Pinned\b\s*\{", r"\bint\s+with_tmp\s*\(")
ROW = L.BY_NAME["count"]


def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


@pytest.mark.parametrize("header", ["needletail_amd.h", "needletail_amd_count.h"])
def test_headers_compile_as_c(header, tmp_path):
    src = tmp_path / "t.c"
    src.write_text(f'#include "{header}"\nint main(void) {{ return 0; }}\n')
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + L.INCLUDE, "-c", "-o", str(tmp_path / "t.o"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if header == os.path.basename(ROW.header):
        L.check_header(ROW, tmp_path)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    L.check_no_device(ROW)


def test_core_exports_ctx_stream():
    out = subprocess.run(["nm", "-D", "--defined-only", CORE], capture_output=True, text=True).stdout
    assert re.search(r"\bT ntk_ctx_stream\b", out)
    lib = C.CDLL(CORE)
    dev, stream = C.c_int(-1), C.c_void_p(1)
    lib.ntk_ctx_stream.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    assert lib.ntk_ctx_stream(None, C.byref(dev), C.byref(stream)) == 2   # NTK_ERR_BAD_ARG


def test_the_shared_pieces_are_defined_once():
    """The hash, the reductions, the host helpers, the record rule and the chunk walk live in ntk_consumer.hpp only, the extract count /
    scan and spectrum kernels in ntk_count_common.hpp only: no library source defines its own copy again."""
    shared = ("fmix64", "wave_sum", "add_agent", "block_sum_u32", "grid_for", "alloc_status", "record_span", "uniform", "for_each_chunk")
    kernel = r"__global__[^{;]*?\bvoid\s+\w*(?:extract_count|extract_scan|spectrum)_kernel\s*\("
    common, consumer = open(COMMON).read(), open(CONSUMER).read()
    for name in shared:
        assert re.search(rf"\b{name}\([^)]*\)\s*\{{", consumer), (name, "not defined in ntk_consumer.hpp")
        assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", common), (name, "defined again in ntk_count_common.hpp")
    assert re.search(r"struct MaterialiseScratch \{", consumer) and '#include "ntk_consumer.hpp"' in common
    mem = open(MEM).read()
    assert '#include "ntk_device_mem.hpp"' in consumer
    for pat in MEM_DEFS:
        assert len(re.findall(pat, mem)) == 1 and not re.search(pat, consumer) and not re.search(pat, common), pat
    assert len(re.findall(kernel, common)) == 3 and not re.search(kernel, consumer)
    for row in L.LIBRARIES:
        path, src = row.hip, open(row.hip).read()
        for name in shared:
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", src), (name, "defined again in", path)
        assert not re.search(kernel, src), ("an extract count / scan or spectrum kernel defined again in", path)
        assert not re.search(r"struct MaterialiseScratch\b", src), path
        for pat in MEM_DEFS:
            assert not re.search(pat, src), (pat, "defined again in", path)
        # the two tables take the shared pieces through their own header, the others directly
        want = "ntk_count_common.hpp" if row.name in ("count", "wide_count") else "ntk_consumer.hpp"
        assert f'#include "{want}"' in src, path


def test_only_the_memory_layer_allocates():
    """Device and pinned memory of the core and of the consumer libraries is allocated and freed in ntk_device_mem.hpp alone, comments
    included: no other source under csrc/ names hipMalloc or hipFree, and the two pinned calls occur outside it once each, in
    ntk_pinned_alloc / ntk_pinned_free of ntk_api.hip, which hand the memory to the caller.  The core's own buffer struct and the
    separate capacity of its pinned stage are gone."""
    sources = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if re.search(r"\.(?:hip|hpp|cpp|h)$", name)}
    found = {name for name, text in sources.items() if re.search(r"hip(?:Host)?(?:Malloc|Free)\b", text)}
    assert found == {"ntk_device_mem.hpp", "ntk_api.hip"}
    api = sources["ntk_api.hip"]
    assert not re.search(r"hip(?:Malloc|Free)\b", api)
    assert len(re.findall(r"hipHostMalloc\b", api)) == 1 and len(re.findall(r"hipHostFree\b", api)) == 1
    assert re.search(r"int ntk_pinned_alloc\([^)]*\)\s*\{[^}]*hipHostMalloc\b[^}]*\}", api)
    assert re.search(r"void ntk_pinned_free\([^)]*\)\s*\{[^}]*hipHostFree\b[^}]*\}", api)
    assert '#include "ntk_device_mem.hpp"' in api
    for pat in MEM_DEFS:
        assert not re.search(pat, api), pat
    for name, text in sources.items():
        assert not re.search(r"struct Scratch\b|h_stage_bytes", text), name


# ---- the host model of the table (tests/_count_model.py), which the edge tests aim with --------------------------------------

def _fmix64_int(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M.M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M.M64
    return x ^ (x >> 33)


def test_model_fmix64_and_its_inverse():
    rng = np.random.default_rng(0xF3)
    x = rng.integers(0, 1 << 64, 200_000, dtype=np.uint64)
    x[:4] = [0, 1, M.M64, 1 << 63]
    assert np.array_equal(M.fmix64_inv(M.fmix64(x)), x) and np.array_equal(M.fmix64(M.fmix64_inv(x)), x)
    assert [int(v) for v in M.fmix64(x[:64])] == [_fmix64_int(int(v)) for v in x[:64]]
    assert all(m * i & M.M64 == 1 for m, i in zip(M.FMIX_MUL, M.FMIX_INV))


def test_model_revcomp_is_the_oracles():
    import oracle as O
    rng = np.random.default_rng(0xF4)
    for k in (1, 2, 13, 16, 31, 32):
        v = rng.integers(0, 1 << (2 * k), 64, dtype=np.uint64)
        assert [int(r) for r in M.revcomp(v, k)] == [O.bit_reverse_complement(int(a), k) for a in v], k


@pytest.mark.parametrize("k,canonical", [(32, False), (32, True), (16, False), (16, True), (13, False)])
def test_model_keys_with_home(k, canonical):
    slots = 8192
    for h in (0, 1000, slots - 7, slots - 1):
        keys = M.keys_with_home(h, slots, k, 120, canonical)
        assert keys.size == 120 and np.unique(keys).size == 120
        assert (M.home(keys, slots) == h).all()
        assert (keys != np.uint64(M.EMPTY)).all()
        if k < 32:
            assert (keys < np.uint64(1 << (2 * k))).all()
        if canonical:
            assert (keys <= M.revcomp(keys, k)).all()
        assert np.array_equal(M.keys_with_home(h, slots, k, 30, canonical), keys[:30])   # a shorter list is a prefix


def test_model_records_emit_exactly_the_keys():
    import oracle as O
    keys = np.array([0, 5, (1 << 42) - 1, 12345678], dtype=np.uint64)
    buf = M.records_for(keys, [3, 1, 2, 7], 21, seed=1)
    assert len(buf) == 13 * 22
    got = np.unique(O.bit_kmers_arrays(buf, 21, False)[1], return_counts=True)
    assert np.array_equal(got[0], np.sort(keys)) and list(got[1]) == [3, 1, 7, 2]


def test_model_sizing_rule():
    assert [M.slots_for(c) for c in (1, 2, 3, 4, 6, 7, 12, 13)] == [2, 4, 4, 8, 8, 16, 16, 32]
    for j in range(1, 37):
        assert M.slots_for(3 << j) == 4 << j and M.slots_for((3 << j) + 1) == 8 << j


def test_table_hash_probe_bound_and_chunk_are_the_models():
    """The edge tests aim keys at home slots and records at chunk seams with tests/_count_model.py.  If the table's hash, probe
    bound or chunk length changes, say so here, on the CPU, rather than as a puzzling count mismatch on the GPU."""
    src, common, consumer = open(HIP).read(), open(COMMON).read(), open(CONSUMER).read()
    m = re.search(r"inline uint64_t fmix64\(uint64_t x\)\s*\{(.*?)\}", consumer, re.S)
    assert m, "fmix64 not found in ntk_consumer.hpp"
    steps = re.findall(r"x \^= x >> (\d+);|x \*= (0x[0-9a-fA-F]+)ull;", m.group(1))
    got = [int(a) if a else int(b, 16) for a, b in steps]
    want = [M.FMIX_SHIFT, M.FMIX_MUL[0], M.FMIX_SHIFT, M.FMIX_MUL[1], M.FMIX_SHIFT]
    assert got == want, f"ntk_consumer.hpp's fmix64 is {got}, tests/_count_model.py's is {want}: update the model with the hash"
    assert re.search(r"fmix64\(key\) & a\.mask", src) and re.search(r"fmix64\(q\) & mask", src), "home slot is not fmix64 & mask"
    assert len(re.findall(r"slot = \(slot \+ 1\) & (?:a\.)?mask", src)) == 2, "probing is not linear with wrap-around"
    assert int(re.search(r"kProbeMax = (\d+);", common).group(1)) == M.PROBE_MAX
    chunk = re.search(r"kChunkBases = \(uint64_t\)(\d+) << (\d+);", open(CHUNKS).read())
    assert int(chunk.group(1)) << int(chunk.group(2)) == M.CHUNK
    assert not re.search(r"kChunkBases\s*=", src), "the chunk length is ntk_chunks.hpp's alone"
