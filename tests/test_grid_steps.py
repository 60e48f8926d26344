"""tests/_grid_steps.py held to the sources: every capped or fixed launch of the twelve k-mer libraries has a row, every row's numbers are
what the source's text evaluates to, and every GPU test a row names exists."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grid_steps as G  # noqa: E402
import _libraries as L  # noqa: E402

TESTS = os.path.dirname(os.path.abspath(__file__))


def balanced(text: str, at: int) -> str:
    """text[at:] up to the parenthesis that closes the first one opened."""
    depth = 0
    for j in range(at, len(text)):
        depth += text[j] == "("
        if text[j] == ")":
            depth -= 1
            if depth == 0:
                return text[at:j + 1]
    raise AssertionError(text[at:at + 80])


def statement(text: str, at: int) -> str:
    """The statement around text[at]."""
    begin = max(text.rfind(c, 0, at) for c in ";{}") + 1
    return text[begin:text.index(";", at) + 1]


def constant(name: str, file: str) -> int:
    """`constexpr TYPE name = value;` in `file`, in the scaffold's header, or (an ML_ name) in the minimizer list's rule."""
    for f in (file, "ntk_consumer.hpp") + (("ntk_ml_rule.hpp",) if name.startswith("ML_") else ()):
        m = re.search(rf"^constexpr \w+ {name} = (\d+)u?;", L.no_comments(G.source(f)), re.M)
        if m:
            return int(m.group(1))
    raise AssertionError((name, file))


def evaluate(expr: str, file: str) -> int:
    """A C expression of integers, casts and named constants."""
    expr = re.sub(r"\((?:unsigned|uint64_t|uint32_t)\)", "", expr)
    expr = re.sub(r"\b\w+->n_cu\b|\bn_cu\b", "1", expr)
    expr = re.sub(r"\bk[A-Z]\w*|\bML_[A-Z_]+", lambda m: str(constant(m.group(0), file)), expr)
    expr = re.sub(r"0x[0-9A-Fa-f]+", lambda m: str(int(m.group(0), 16)), expr)
    expr = re.sub(r"(\d)u\b", r"\1", expr).replace("/", "//")
    assert re.fullmatch(r"[\d\s()*/+-]+", expr), expr
    return int(eval(expr))   # noqa: S307  (digits and operators only)


def sites(text: str):
    """(at, expression) of every grid the device's CU count shapes: each grid_for call, and each dim3 of an expression that names n_cu
    or a local defined from it."""
    text = L.no_comments(text)
    locals_ = set(re.findall(r"const unsigned (\w+) = (?![^;]*grid_for\()[^;]*n_cu[^;]*;", text))   # (a grid_for is a site itself)
    out = []
    for m in re.finditer(r"\bgrid_for\(", text):
        if not re.search(r"inline unsigned $", text[max(0, m.start() - 16):m.start()]):   # (its definition)
            out.append((m.start(), balanced(text, m.start())))
    for m in re.finditer(r"\bdim3\(", text):
        expr = balanced(text, m.start())
        inner = expr[5:-1]
        if "grid_for(" not in inner and (re.search(r"\bn_cu\b", inner) or inner in locals_):
            out.append((m.start(), expr))
    return text, out


@pytest.mark.parametrize("lib", G.LIBS)
def test_every_capped_launch_has_its_rows(lib):
    """`sites` decides what needs a row: a grid_for call, or a dim3 that names n_cu or a local made from it.  Of the minimizer list's four
    launches that leaves out ml_scan_kernel (dim3(1): one block scans a chunk's tile counts, whatever the device) and ml_offsets_kernel
    (dim3(blocks_for(n_records + 1)): one thread per record start, no cap and no loop), so neither has a row."""
    rows = [r for r in G.ROWS if r.lib == lib]
    for file in G.files_of(lib):
        text, found = sites(G.source(file))
        here = [r for r in rows if r.file == file]
        assert {expr for _, expr in found} == {r.site for r in here}, (file, sorted({e for _, e in found} ^ {r.site for r in here}))
        for site in {r.site for r in here}:
            want = sorted(r.kernel for r in here if r.site == site)
            got = []
            for at, expr in found:
                if expr != site:
                    continue
                st = statement(text, at)
                direct = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", st)
                if direct:
                    got += direct
                else:   # a local or a member function carries the grid to its launches
                    patterns = {r.launch for r in here if r.site == site}
                    assert len(patterns) == 1 and "" not in patterns, (file, site, st)
                    got += re.findall(patterns.pop(), text)
            assert sorted(set(got)) == want and len(got) >= len(want), (file, site, got, want)
    assert {r.file for r in rows} <= set(G.files_of(lib)), lib


def test_the_rows_are_the_twelve_libraries_and_no_launch_is_listed_twice():
    assert len(G.LIBS) == 12 and {r.lib for r in G.ROWS} == set(G.LIBS)
    keys = [(r.lib, r.kernel) for r in G.ROWS]
    assert len(set(keys)) == len(keys)
    for r in G.ROWS:   # a kernel the inventory names is one the library ships (tests/_libraries.py holds those to the binaries)
        if r.lib == "minimizer_list":   # (its row is tests/test_minimizer_list_abi.py's)
            import test_minimizer_list_abi as ml
            assert r.kernel in ml.ROW.kernels and G.files_of(r.lib) == (os.path.basename(ml.ROW.hip),) + ml.ROW.headers, r.kernel
        elif r.lib != "colors":
            assert any(L.bare(k).split("<")[0] == r.kernel for k in L.BY_NAME[r.lib].kernels), r.kernel


@pytest.mark.parametrize("row", G.ROWS, ids=lambda r: f"{r.lib}-{r.kernel}")
def test_a_rows_numbers_are_what_its_source_says(row):
    text = L.no_comments(G.source(row.file))
    assert row.site in text and row.grid in ("capped", "fixed")
    if row.grid == "capped":
        args = row.site[len("grid_for("):-1]
        assert args.endswith(f", {row.per_block_text}, {row.cap_text}")
    else:
        assert row.site == f"dim3({row.cap_text})"
    assert evaluate(row.per_block_text, row.file) == row.per_block
    cap = row.cap_text
    if row.cap_def:
        assert row.cap_def in text and row.cap_def.startswith(f"const unsigned {cap} = ")
        cap = row.cap_def.split(" = ", 1)[1].rstrip(";")
    if row.factor is None:
        assert evaluate(cap, row.file) == 0x7FFFFFFF and row.test is None and "not capped" in row.note
    else:
        assert re.search(r"\bn_cu\b", cap), "the cap is a multiple of the CU count"
        assert evaluate(cap, row.file) == row.factor
        assert G.items_per_step(row, 256) == row.per_block * row.factor * 256
    assert re.search(rf"\b{row.kernel}\b", text if row.file.endswith(".hip") else text + G.source(f"ntk_{row.lib}.hip"))


def test_the_kernels_stride_by_what_the_rows_say():
    """The loop of a record kernel steps by its grid's items: the text of the strides the new GPU tests rely on."""
    src = {f: L.no_comments(G.source(f)) for f in ("ntk_abundance.hip", "ntk_colors.hip", "ntk_trim.hip", "ntk_record_minhash.hip",
                                                   "ntk_kmer_sets.hip", "ntk_dbg.hip", "ntk_minimizer_list.hip")}
    assert "for (uint64_t i = blockIdx.x; i < n_long; i += gridDim.x)" in src["ntk_abundance.hip"]
    assert "for (uint64_t r = first; r < a.n_records; r += waves)" in src["ntk_colors.hip"]
    assert "screen_rounds(a, lo, hi, first, waves, lane, acc);" in src["ntk_colors.hip"]
    assert "r0 < a.n_records; r0 += waves * kPerWave)" in src["ntk_trim.hip"]
    assert "r < a.b.n_records; r += (uint64_t)gridDim.x * kPerBlock)" in src["ntk_trim.hip"]
    assert "for (uint64_t r = a.r0 + blockIdx.x; r < a.r1; r += gridDim.x)" in src["ntk_record_minhash.hip"]
    assert len(re.findall(r"const uint64_t stride = \(uint64_t\)gridDim\.x \* kThreads", src["ntk_dbg.hip"])) == 10
    # the minimizer list: the select kernel strides over the tiles, the scatter kernel takes a contiguous run of `per` of them
    ml = src["ntk_minimizer_list.hip"]
    assert "for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x)" in ml
    assert "const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x, t_begin = blockIdx.x * per" in ml
    assert "for (uint64_t t = t_begin; t < t_end; t++)" in ml


def test_the_units_of_the_notes():
    file, name, value = G.K_LANE_RUN
    assert constant(name, file) == value
    for file, name, value in G.K_PER_LANE:
        assert constant(name, file) == value
    assert re.search(r"kChunkBases = \(uint64_t\)64 << 20;", G.source("ntk_chunks.hpp")) and G.K_CHUNK == 64 << 20
    rmh = L.no_comments(G.source("ntk_record_minhash.hip"))
    assert "constexpr uint64_t kTile = 64 * kPerLane;" in rmh and "constexpr uint64_t kSegment = 4 * kTile * 4;" in rmh
    assert G.K_RMH_SEGMENT == 4 * (64 * 4) * 4
    file, name, value = G.K_ML_TILE
    assert constant(name, file) == value


def test_every_named_gpu_test_exists():
    for row in G.ROWS:
        if row.test is None:
            assert row.note, (row.kernel, "a row without a test says why")
            continue
        for fname, test in filter(None, (row.test, row.also)):
            text = open(os.path.join(TESTS, fname)).read()
            assert re.search(rf"^def {re.escape(test)}\(", text, re.M), (row.kernel, fname, test)
            assert re.search(r"^pytestmark = pytest\.mark\.gpu", text, re.M), fname


def test_items_per_step():
    assert G.items_per_step(G.rows_of("ra_wave_kernel"), 256) == 8192
    assert G.items_per_step(G.rows_of("ra_block_kernel"), 256) == 256
    assert G.items_per_step(G.rows_of("kc_long_kernel"), 256) == 262144
    assert G.items_per_step(G.rows_of("dbg_rows_kernel"), 256) == 1 << 20
    assert G.items_per_step(G.rows_of("rt_interval_kernel"), 304) == 32 * 8 * 304
    assert G.items_per_step(G.rows_of("ks_split_kernel"), 256) is None
    assert G.items_per_step(G.rows_of("ml_select_kernel"), 256) == G.items_per_step(G.rows_of("ml_scatter_kernel"), 256) == 2048
