"""CPU-side checks of the count library (include/needletail_amd_count.h, libneedletail_amd_count.so): exports, C headers, the core entry
it needs, the kernels it ships (each names the test that launches it) and the loud error without a device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import _builds as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "needletail_amd", "libneedletail_amd_count.so")
CORE = os.path.join(ROOT, "needletail_amd", "libneedletail_amd.so")
HEADER = os.path.join(ROOT, "include", "needletail_amd_count.h")

# every kernel of the count library with the test that launches it (file, test function); rocPRIM's sort kernels by namespace
COUNT_KERNELS = {
    "(anonymous namespace)::kt_insert_kernel((anonymous namespace)::InsertArgs)": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
    "(anonymous namespace)::kt_extract_count_kernel": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
    "(anonymous namespace)::kt_extract_scan_kernel": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
    "(anonymous namespace)::kt_extract_scatter_kernel": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
    "(anonymous namespace)::kt_spectrum_kernel": ("test_gpu_count.py", "test_genome_sampled_reads_spectrum"),
    "(anonymous namespace)::kt_lookup_kernel": ("test_gpu_count.py", "test_golden_28s_and_prjna271013"),
}
SORT_NAMESPACE = "rocprim::"


def _built():
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "needletail_amd", "csrc")])
    return SO


def _header_symbols(path):
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ntk_[a-z0-9_]+)\s*\(", hdr)))


def test_every_declared_function_is_exported_and_listed():
    from needletail_amd import counting
    lib = C.CDLL(_built())
    syms = _header_symbols(HEADER)
    assert len(syms) == 8
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/needletail_amd_count.h but not exported"
    assert sorted(counting.SYMBOLS) == syms


def test_core_exports_ctx_stream():
    out = subprocess.run(["nm", "-D", "--defined-only", CORE], capture_output=True, text=True).stdout
    assert re.search(r"\bT ntk_ctx_stream\b", out)
    lib = C.CDLL(CORE)
    dev, stream = C.c_int(-1), C.c_void_p(1)
    lib.ntk_ctx_stream.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    assert lib.ntk_ctx_stream(None, C.byref(dev), C.byref(stream)) == 2   # NTK_ERR_BAD_ARG


def test_count_library_links_the_core_by_rpath():
    out = subprocess.run(["readelf", "-d", _built()], capture_output=True, text=True).stdout
    assert "libneedletail_amd.so" in out and "$ORIGIN" in out


@pytest.mark.parametrize("header", ["needletail_amd.h", "needletail_amd_count.h"])
def test_headers_compile_as_c(header):
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.c")
        with open(src, "w") as f:
            f.write(f'#include "{header}"\nint main(void) {{ return 0; }}\n')
        r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", "-o",
                            os.path.join(td, "t.o"), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_every_kernel_names_the_test_that_launches_it():
    names = B.library_kernels(_built())
    ours = {n for n in names if not n.startswith(SORT_NAMESPACE)}
    assert ours == set(COUNT_KERNELS), sorted(ours ^ set(COUNT_KERNELS))
    assert any("radix" in n for n in names - ours)   # the extract's sort
    for sym, (fname, test) in COUNT_KERNELS.items():
        src = open(os.path.join(ROOT, "tests", fname)).read()
        assert re.search(rf"^def {re.escape(test)}\(", src, re.M), (sym, fname, test)


def test_product_files_never_name_the_checker():
    for path in (HEADER, os.path.join(ROOT, "needletail_amd", "csrc", "ntk_count.hip"), os.path.join(ROOT, "needletail_amd", "counting.py"),
                 os.path.join(ROOT, "examples", "count_kmers.cpp")):
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
        nt.KmerTable(21, nt.PATH_BITS_CANONICAL, 1000)
    assert e.value.status == 4   # NTK_ERR_NO_DEVICE
