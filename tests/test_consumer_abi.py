"""CPU-side checks every library on the core's public ABI is held to, written once over the rows of tests/_libraries.py.

Parametrised here, one case per row: the link, no leak of a kernel into another library, the shared scaffold used and not restated,
and the build rule as make expands it.  The check_* functions of tests/_libraries.py - exports, the C header, the kernels it ships
(each names the GPU test that launches it), product files that never name the checker, the loud error without a device - are
called with its row by the test of that name in each tests/test_NAME_abi.py, which keeps its test ids and what is the library's
own: its model, its constants, its allocation arithmetic.  test_every_row_is_put_through_every_check holds every file to that."""
import os
import re
import subprocess

import pytest

import _builds as B
import _libraries as L

ROWS = pytest.mark.parametrize("row", L.LIBRARIES, ids=[r.name for r in L.LIBRARIES])
SHARED = ("fmix64", "wave_sum", "add_agent", "block_sum_u32", "grid_for", "alloc_status", "record_span", "uniform", "for_each_chunk")
MEM_DEFS = (r"struct DeviceArray\b\s*\{", r"struct Pinned\b\s*\{", r"\bint\s+with_tmp\s*\(")


@ROWS
def test_library_links_exactly_what_it_needs_by_rpath(row):
    out = subprocess.run(["readelf", "-d", L.built(row.so)], capture_output=True, text=True).stdout
    needed = [n for n in re.findall(r"NEEDED.*\[(.*?)\]", out) if n.startswith("libneedletail_amd")]
    assert "$ORIGIN" in out
    assert needed == [os.path.basename(L.so_path(n)) for n in row.links + ("",)], needed


@pytest.mark.parametrize("owner", [""] + [r.name for r in L.LIBRARIES], ids=["core"] + [r.name for r in L.LIBRARIES])
def test_no_kernel_leaks_into_another_library(owner):
    """For every ordered pair of the eleven shared objects.  A library's kernels are what its pattern names - it matches every one of
    them - and the core's are its own, name for name.  The ct_ family is the count and the wide count library's together."""
    own = B.library_kernels(L.built(L.so_path(owner)))
    if owner:
        pattern = L.BY_NAME[owner].leak
        assert all(re.search(pattern, n) for n in L.own_kernels(own)), "the pattern no longer names the library's own kernels"
        names_own = lambda n: re.search(pattern, n)   # noqa: E731
    else:
        names_own = own.__contains__
    for other in [""] + [r.name for r in L.LIBRARIES]:
        if other == owner:
            continue
        leaked = {n for n in B.library_kernels(L.so_path(other)) if names_own(n)}
        if {owner, other} == L.SHARED_KERNELS[0]:
            leaked = {n for n in leaked if not re.search(L.SHARED_KERNELS[1], n)}
        assert not leaked, (owner or "core", other or "core", sorted(leaked))


def test_shared_headers_never_name_the_checker():
    for name in L.CONSUMER_HPP:
        assert not re.search(r"\boracle\b|ntko_", open(os.path.join(L.CSRC, name)).read()), name


@ROWS
def test_the_shared_pieces_are_used_and_not_defined_again(row):
    """The scaffold comes from ntk_consumer.hpp (for the two tables through ntk_count_common.hpp), memory from ntk_device_mem.hpp:
    neither the source nor the library's own headers define a piece of them again, or allocate."""
    src = open(row.hip).read()
    consumer, mem = (open(os.path.join(L.CSRC, f)).read() for f in L.CONSUMER_HPP[:2])
    assert '#include "%s"' % ("ntk_count_common.hpp" if "ntk_count_common.hpp" in row.headers else "ntk_consumer.hpp") in src
    assert '#include "ntk_device_mem.hpp"' in consumer
    for h in row.headers:
        assert f'#include "{h}"' in src, h
    for name in SHARED:
        assert re.search(rf"\b{name}\([^)]*\)\s*\{{", consumer), (name, "not defined in ntk_consumer.hpp")
    for pat in MEM_DEFS:
        assert len(re.findall(pat, mem)) == 1, (pat, "not defined in ntk_device_mem.hpp")
    for text in [src] + [open(os.path.join(L.CSRC, h)).read() for h in row.headers]:
        for name in SHARED:
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", text), (name, "defined again")
        for pat in MEM_DEFS:
            assert not re.search(pat, text), (pat, "defined again")
        assert not re.search(r"struct (?:MaterialiseScratch|Consumer)\b\s*\{", text)
        assert not re.search(r"hip(?:Host)?(?:Malloc|Free)\b", text), "the memory layer allocates"


def test_the_core_takes_its_memory_from_the_same_layer():
    """ntk_api.hip includes ntk_device_mem.hpp (with its own check macro and status) and defines none of its pieces again."""
    api, mem = (open(os.path.join(L.CSRC, f)).read() for f in ("ntk_api.hip", L.CONSUMER_HPP[1]))
    assert '#include "ntk_device_mem.hpp"' in api and "#define CT_HIPCHK" in api and re.search(r"\balloc_status\([^)]*\)\s*\{", api)
    for pat in MEM_DEFS:
        assert len(re.findall(pat, mem)) == 1 and not re.search(pat, api), pat


CHECKS = ("check_exports", "check_header", "check_kernels", "check_product_files_never_name_the_checker", "check_no_device")


@ROWS
def test_every_row_is_put_through_every_check(row):
    """The five checks of tests/_libraries.py that are not parametrised here are called, with the library's row, by tests of the old
    names in tests/test_NAME_abi.py: a row whose file leaves one out fails here."""
    text = open(os.path.join(L.ROOT, "tests", f"test_{row.name}_abi.py")).read()
    assert re.search(rf'^ROW = L\.BY_NAME\["{row.name}"\]$', text, re.M)
    for check in CHECKS:
        assert re.search(rf"^def test_\w+\((?:[\w, ]*)\):\n(?:    [^\n]*\n)*?    +L\.{check}\(ROW\b", text, re.M), check


@ROWS
def test_build_rule_is_the_rows(row):
    """csrc/Makefile as make expands it: what the object depends on, what the library links, and that all builds and clean removes both."""
    db = L.make_database()
    obj, so = f"ntk_{row.name}.o", f"../libneedletail_amd_{row.name}.so"
    assert tuple(db.variables["CONSUMER_HPP"].split()) == L.CONSUMER_HPP
    assert db.prerequisites[obj] == {f"ntk_{row.name}.hip", *row.headers, *L.CONSUMER_HPP, *(L.public_header(n) for n in (row.name, "") + row.uses)}
    assert db.prerequisites[so] == {obj, *(f"../libneedletail_amd_{n}.so" for n in row.links), "../libneedletail_amd.so"}
    assert so in db.prerequisites["all"]
    compile_, = [ln for ln in db.build if f" -c -o {obj} " in ln]
    link, = [ln for ln in db.build if f" -o {so} " in ln]
    assert compile_.endswith(f" ntk_{row.name}.hip") and "--offload-arch=gfx950" in compile_
    assert re.findall(r"-l(\S+)", link) == [f"needletail_amd_{n}" for n in row.links] + ["needletail_amd"] and f" {obj} " in link
    removed, = [ln.split() for ln in db.clean if ln.startswith("rm -f")]
    assert obj in removed and so in removed


def test_three_lists_name_the_same_libraries():
    """csrc/Makefile's CONSUMER lines, the two tables of __graft_entry__.py and the rows of tests/_libraries.py."""
    import __graft_entry__ as G
    names = [r.name for r in L.LIBRARIES]
    assert L.make_database().variables["CONSUMERS"].split() == names and len(set(names)) == 10
    assert list(G.BINDINGS) == [r.binding for r in L.LIBRARIES]
    assert {lib for libs in G.EXAMPLES.values() for lib in libs} == set(names)
    ignored = open(os.path.join(L.ROOT, ".gitignore")).read().split()
    for r in L.LIBRARIES:
        assert r.name in G.EXAMPLES[r.example], (r.name, "its example program does not link it")
        assert os.path.exists(os.path.join(L.ROOT, "examples", r.example + ".cpp")) and "examples/" + r.example in ignored
    for example, libs in G.EXAMPLES.items():
        assert any(r.example == example for r in L.LIBRARIES), (example, "an example program of no library")
