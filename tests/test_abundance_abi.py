"""CPU-side checks of the abundance library (include/needletail_amd_abundance.h, libneedletail_amd_abundance.so) beyond those every library
is held to (tests/test_consumer_abi.py): the row layout, the constants the GPU tests aim at, the refusal of a wide table, and the host
model (tests/_abundance_model.py) on hand-made counts."""
import os
import re

import numpy as np
import pytest

import _abundance_model as A
import _libraries as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "needletail_amd_abundance.h")
HIP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_abundance.hip")
CHUNKS = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_chunks.hpp")   # the chunk geometry every library walks

A_REG_WINDOWS, A_LONG_RECORD = 192, 65536   # tests/test_gpu_abundance.py REG_WINDOWS, LONG_RECORD
ROW = L.BY_NAME["abundance"]


def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


def test_header_compiles_as_c(tmp_path):
    L.check_header(ROW, tmp_path)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    L.check_no_device(ROW)


def test_row_layout_is_the_columns():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct ntk_read_abundance_row \{(.*?)\};", hdr, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]+);", body) for f in decl.split(",")]
    assert tuple(fields) == A.COLUMNS
    from needletail_amd import abundance
    assert abundance.COLUMNS == A.COLUMNS


def test_kernel_constants_are_the_tests():
    """The GPU tests aim at the wave kernel's register seam, the long-record threshold and the chunk length; hold them to the source."""
    import _count_model as CM
    src = open(HIP).read()
    chunk = re.search(r"kChunkBases = \(uint64_t\)(\d+) << (\d+);", open(CHUNKS).read())
    assert int(chunk.group(1)) << int(chunk.group(2)) == CM.CHUNK
    assert not re.search(r"kChunkBases\s*=", src), "the chunk length is ntk_chunks.hpp's alone"
    assert int(re.search(r"kRegRounds = (\d+);", src).group(1)) * 64 == A_REG_WINDOWS
    assert int(re.search(r"kLongRecord = (\d+);", src).group(1)) == A_LONG_RECORD
    assert not re.search(r"\basm\b|__asm", src), "plain HIP C++"


def test_wide_table_is_a_type_error():
    import needletail_amd as nt
    wide = object.__new__(nt.WideKmerTable)   # no device needed: the argument's type alone decides
    wide._h = None
    with pytest.raises(TypeError, match=r"k <= 32.*33\.\.63"):
        nt.ReadAbundance(wide)
    with pytest.raises(TypeError):
        nt.ReadAbundance("table")


# ---- the host model (tests/_abundance_model.py), which the GPU tests hold the rows to ------------------------------------------------

def _plain(counts, min_count=1):
    """The issue's recipe in Python integers."""
    c = sorted(int(x) for x in counts)
    n, mc = len(c), max(min_count, 1)
    if n == 0:
        return [0] * 6
    return [n, sum(1 for x in c if x >= mc), c[0], c[n // 2], c[-1], sum(c) % (1 << 64)]


def test_model_rows_on_hand_made_counts():
    assert list(A.row([])) == [0, 0, 0, 0, 0, 0]
    assert list(A.row([7])) == [1, 1, 7, 7, 7, 7]
    assert list(A.row([9, 2])) == [2, 2, 2, 9, 9, 11]                      # n = 2: the upper median
    assert list(A.row([5, 1, 3])) == [3, 3, 1, 3, 5, 9]
    assert list(A.row([4, 1, 3, 2])) == [4, 4, 1, 3, 4, 10]                # n = 4: c[2], the upper of the middle two
    assert list(A.row([6, 6, 6, 6, 6])) == [5, 5, 6, 6, 6, 30]             # all equal
    assert list(A.row([0, 0, 5])) == [3, 1, 0, 0, 5, 5]                    # absent k-mers count 0
    big = (1 << 63) + 1
    assert list(A.row([1, 2, big, 3, 1])) == [5, 5, 1, 2, big, (big + 7) % (1 << 64)]
    assert list(A.row([big, big, 1])) == [3, 3, 1, big, big, (2 * big + 1) % (1 << 64)] == [3, 3, 1, big, big, 3]   # the sum wraps
    assert list(A.row([0, 1, 2, 3], 0)) == list(A.row([0, 1, 2, 3], 1)) == [4, 3, 0, 2, 3, 6]   # min_count 0 = 1
    assert list(A.row([0, 1, 2, 3], 3)) == [4, 1, 0, 2, 3, 6]
    assert A.row([1]).dtype == np.uint64
    rng = np.random.default_rng(0xAB)
    for n in list(range(0, 12)) + [63, 64, 65, 191, 192, 193, 1000, 5000]:
        for top in (1, 2, 3, 50, 1 << 40, 1 << 64):
            c = rng.integers(0, top, n, dtype=np.uint64)
            for mc in (0, 1, 3):
                assert [int(x) for x in A.row(c, mc)] == _plain(c, mc), (n, top, mc)


def test_model_weighted_rows_equal_the_written_out_ones():
    rng = np.random.default_rng(0xAC)
    for n in (1, 2, 5, 40):
        for top in (2, 4, 1000, 1 << 63):
            c = rng.integers(0, top, n, dtype=np.uint64)
            w = rng.integers(0, 6, n)
            for mc in (0, 1, 3):
                assert np.array_equal(A.weighted_row(c, w, mc), A.row(np.repeat(c, w), mc)), (n, top, mc)


def test_model_lookup_and_lines():
    items = (np.array([2, 5, 9], dtype=np.uint64), np.array([7, 1, 3]))
    assert list(A.lookup(np.array([9, 0, 5, 10, 2, 2], dtype=np.uint64), items)) == [3, 0, 1, 0, 7, 7]
    assert list(A.lookup(np.array([1], dtype=np.uint64), (np.zeros(0, np.uint64), np.zeros(0, np.int64)))) == [0]
    assert list(A.offsets([b"ACG", b"", b"T"])) == [0, 4, 5, 7]
    assert A.mean_text([0, 0, 0, 0, 0, 0]) == "0.000"
    assert A.mean_text([3, 0, 0, 0, 0, 10]) == "3.333" and A.mean_text([3, 0, 0, 0, 0, 11]) == "3.667"
    assert A.mean_text([2000, 0, 0, 0, 0, 1]) == "0.001" and A.mean_text([2001, 0, 0, 0, 0, 1]) == "0.000"
    assert A.mean_text([2000, 0, 0, 0, 0, 3999]) == "2.000"                 # 1.9995 rounds up into the next whole
    assert A.cli_line("r1", [130, 120, 0, 4, 9, 520]) == "r1\t130\t120\t0\t4\t9\t4.000"
