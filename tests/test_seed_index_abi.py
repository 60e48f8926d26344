"""CPU-side checks of the seed-index library (include_staged/needletail_amd/seed_index.h, libneedletail_amd_seed_index.so).

The library is stated beside the thirteen before it (csrc/Makefile STAGED_LIBS, __graft_entry__.py STAGED_BINDINGS / STAGED_EXAMPLES),
and its public header waits in include_staged/needletail_amd/ - the header inventories of the earlier test files take no row - under
the include spelling it will have in include/needletail_amd/.  Its row is made here from a Library whose `header` is that path and put
through the check_* functions of tests/_libraries.py; check_header, which names a header by its base name below include/, is restated
for this layout, as are the checks tests/test_consumer_abi.py parametrises over the ten.  ROWS is derived from STAGED_LIBS, so the next
staged library is a name there and a row in STAGED here, and no new set of lists.  Then what is the library's own: the stream contract
of its calls, the refusals that need no device, and the header's memory statement against the `ensure` calls."""
import ctypes as C
import os
import re
import subprocess

import _builds as B
import _libraries as L
import _seed_index_model as M
import _stream_contract as SC

ROOT = L.ROOT
STAGED_INCLUDE = os.path.join(ROOT, "include_staged")
GPU_TESTS = "test_gpu_seed_index.py"


class StagedLibrary(L.Library):
    """A row whose public header is include_staged/needletail_amd/NAME.h."""
    __slots__ = ()
    header = property(lambda s: os.path.join(STAGED_INCLUDE, "needletail_amd", s.name + ".h"))
    include = property(lambda s: "needletail_amd/" + s.name + ".h")                              # as a program names it with both -I
    make_header = property(lambda s: "../../include_staged/needletail_amd/" + s.name + ".h")    # as csrc/Makefile names it


_SMALL, _RANDOM, _ROUTES = "test_small_lists_under_every_max_occ", "test_random_lists_match_the_model", "test_both_sort_routes_around_the_tile"
STAGED = {
    "seed_index": StagedLibrary(
        "seed_index", binding="seeding", cls="SeedIndex",
        calls=("create", "destroy", "build_device", "spectrum", "match_device", "read", "result_device", "stats", "trim"),
        headers=("ntk_si_rule.hpp",), example="seed_reads", bench="seed_index_bench", gpu_tests=GPU_TESTS, kernels={
            "si_verify_kernel": "test_refusals_leave_the_held_result_unchanged",
            "si_owner_kernel": _SMALL, "si_heads_kernel": _SMALL, "si_pack_kernel": _SMALL,
            "si_spectrum_kernel": _RANDOM,
            "si_lookup_kernel": _SMALL, "si_rows_kernel": _SMALL, "si_fill_kernel": "test_one_seed_with_20000_occurrences_among_seeds_with_one",
            "si_sort_kernel": _ROUTES, "si_widen_kernel": _ROUTES, "si_narrow_kernel": _ROUTES,
        }, leak=r"(?:^|::)si_",
        c_main="struct ntk_seed_index_stats s; s.device_bytes = 8; return sizeof s == 64 && sizeof s.max_occ == s.device_bytes ? 0 : 1;",
        no_device=lambda nt: nt.SeedIndex(), prim=("radix", "scan", "segmented"), shape=r"::si_[a-z]+_kernel\b", n_global=11),
}


def _staged_names():
    return L.make_database().variables["STAGED_LIBS"].split()


ROWS = [STAGED[name] for name in _staged_names()]
ROW = STAGED["seed_index"]
HEADER, HIP, RULE_HPP = ROW.header, ROW.hip, os.path.join(L.CSRC, "ntk_si_rule.hpp")


# ---- the checks of tests/_libraries.py ------------------------------------------------------------------------------------------------

def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    L.check_no_device(ROW)


def test_header_compiles_as_c_and_states_the_struct_sizes(tmp_path):
    """check_header for a staged header: a C11 program names it as users do, with both include directories; its only include is the
    core's; the public headers its object depends on are itself and the core's."""
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(f'#include "{ROW.include}"\nint main(void) {{ {ROW.c_main} }}\n')
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + L.INCLUDE, "-I" + STAGED_INCLUDE, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0, "a struct size or a constant is not the stated one"
    includes = lambda path: re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(path).read())   # noqa: E731
    assert includes(HEADER) == ["needletail_amd.h"]
    # followed through both include directories, as check_header follows them through one: the public headers the Makefile's object
    # rule names are the library's and the core's
    seen, todo = set(), [ROW.include]
    while todo:
        h = todo.pop()
        found = [os.path.join(d, h) for d in (L.INCLUDE, STAGED_INCLUDE) if os.path.exists(os.path.join(d, h))]
        if h not in seen and found:
            assert len(found) == 1, (h, "in both include directories")
            seen.add(h)
            todo += includes(found[0])
    assert seen == {ROW.include, "needletail_amd.h"}
    named = {p for p in L.make_database().prerequisites["ntk_seed_index.o"] if p.startswith("../../include")}
    assert named == {ROW.make_header, L.public_header("")}
    from needletail_amd import seeding as SD
    assert C.sizeof(SD.Stats) == 64 and [n for n, _ in SD.Stats._fields_] == list(M.STATS) == _struct_fields("ntk_seed_index_stats")
    assert all(t is C.c_uint64 for _, t in SD.Stats._fields_)
    assert SD.SORT_TILE == M.SORT_TILE == 2048 and SD.ERR_CAPACITY == M.ERR_CAPACITY == 5
    assert "NTK_SEED_INDEX_SORT_TILE" not in open(HEADER).read(), "an untuned first choice is no public constant"


def _struct_fields(struct):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct %s \{(.*?)\};" % struct, hdr, re.S).group(1)
    return [f.strip() for decl in re.findall(r"uint(?:64|32)_t ([^;]+);", body) for f in decl.split(",")]


# ---- the checks tests/test_consumer_abi.py parametrises over the rows, for this layout -------------------------------------------------

def test_library_links_the_core_alone_by_rpath():
    out = subprocess.run(["readelf", "-d", L.built(ROW.so)], capture_output=True, text=True).stdout
    needed = [n for n in re.findall(r"NEEDED.*\[(.*?)\]", out) if n.startswith("libneedletail_amd")]
    assert "$ORIGIN" in out and needed == ["libneedletail_amd.so"], needed


def _other_libraries():
    """name -> leak pattern of the thirteen shared objects before this one ("" is the core, which has no pattern)."""
    import test_colors_abi as colors
    import test_minimizer_list_abi as ml
    others = {"": None, **{r.name: r.leak for r in L.LIBRARIES}, colors.ROW.name: colors.ROW.leak, **{r.name: r.leak for r in ml.ROWS}}
    assert len(others) == 13
    return others


def test_no_kernel_leaks_into_or_out_of_the_library():
    """No si_ kernel in any of the thirteen other shared objects, and none of theirs in this one."""
    own = L.own_kernels(B.library_kernels(L.built(ROW.so)))
    assert own and all(re.search(ROW.leak, n) for n in own), "the pattern no longer names the library's own kernels"
    for other, leak in _other_libraries().items():
        theirs = B.library_kernels(L.built(L.so_path(other)))
        assert not {n for n in theirs if re.search(ROW.leak, n)}, other or "core"
        assert not own & theirs, other or "core"
        if leak:
            assert not {n for n in own if re.search(leak, n)}, other
    names = " ".join(re.findall(r"\b(?:struct|void|int)\s+(\w+)", L.no_comments(open(HIP).read() + open(RULE_HPP).read())))
    assert not re.search(r"abundance|sketch|minhash|read_trim", names), "a name another library's leak pattern would match"


def test_the_shared_pieces_are_used_and_not_defined_again():
    """The scaffold comes from ntk_consumer.hpp and memory from ntk_device_mem.hpp; neither new file defines a piece of them again or
    names an allocation call, comments included.  Plain HIP C++, no inline assembly, no floating point; rocPRIM's temporary storage
    goes through with_tmp, and so through a DeviceArray."""
    from test_consumer_abi import MEM_DEFS, SHARED
    src, rule = open(HIP).read(), open(RULE_HPP).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_si_rule.hpp"' in src
    assert '#include "../../include_staged/needletail_amd/seed_index.h"' in src
    for text in (src, rule):
        for name in SHARED:
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", text), (name, "defined again")
        for pat in MEM_DEFS:
            assert not re.search(pat, text), (pat, "defined again")
        assert not re.search(r"struct (?:MaterialiseScratch|Consumer)\b\s*\{", text)
        assert not re.search(r"hip(?:Host)?(?:Malloc|Free)\b", text), "the memory layer allocates"
        code = L.no_comments(text)
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
        assert not re.search(r"\b(?:double|float)\b", code), "no floating point anywhere in the library"
    code = L.no_comments(src)
    for name in ("add_agent", "wave_sum", "grid_for", "with_tmp", "si_find", "si_classify", "si_ref", "si_ref_rev", "si_sort_key", "si_before",
                 "si_at_or_before"):
        assert re.search(rf"\b{name}\(", code), name
    assert "struct ntk_seed_index : Consumer {" in src and "m->bind(ctx, 0, 0)" in src
    assert len(re.findall(r"rocprim::\w+\(", code)) == len(re.findall(r"with_tmp\(m->d_tmp, st, grow_exact,", code)) == 5
    assert "ntk_materialize" not in code and "MaterialiseScratch" not in code, "the library never reads a base"
    for f in ("ntk_consumer.hpp", "ntk_chunks.hpp", "ntk_device_mem.hpp"):
        assert "seed_index" not in open(os.path.join(L.CSRC, f)).read() and "ntk_si_" not in open(os.path.join(L.CSRC, f)).read(), f
    assert "ntk_minimizer_list" not in code, "it takes the lists as arrays and does not link the library that makes them"


# the command lines of the thirteen objects and libraries before this one, as make expanded them in the parent commit
_CC = "/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "
_LD = "/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o "
_TAIL = "-lneedletail_amd -Wl,-rpath,'$ORIGIN'"
OLDER = {name: ("", "") for name in ("count", "wide_count", "sketch", "minhash", "minhash_set", "record_minhash", "kmer_sets", "dbg", "colors")}
OLDER.update(abundance=("", "-lneedletail_amd_count "), trim=("", "-lneedletail_amd_count "), minimizer_list=(" -I../../include", ""))
OLDER_LINES = [_CC + " -c -o ntk_api.o ntk_api.hip",
               _LD + "../libneedletail_amd.so ntk_api.o ntk_scan2.o ntk_scan2_q.o ntk_scan2_min.o ntk_scan2_min2.o ntk_fastx.o ntk_fastx_codecs.o "
               "ntk_fastx_api.o ntk_pgzip.o -lz -ldl -lpthread"]
for _name, (_inc, _libs) in OLDER.items():
    OLDER_LINES += [f"{_CC}{_inc} -c -o ntk_{_name}.o ntk_{_name}.hip", f"{_LD}../libneedletail_amd_{_name}.so ntk_{_name}.o -L.. {_libs}{_TAIL}"]


def test_build_rule_is_the_rows_and_the_older_command_lines_are_unchanged():
    db = L.make_database()
    for row in ROWS:
        obj, so = f"ntk_{row.name}.o", f"../libneedletail_amd_{row.name}.so"
        assert db.prerequisites[obj] == {f"ntk_{row.name}.hip", *row.headers, *L.CONSUMER_HPP, row.make_header, L.public_header("")}
        assert db.prerequisites[so] == {obj, "../libneedletail_amd.so"}
        assert so in db.prerequisites["all"]
        compile_, = [ln for ln in db.build if f" -c -o {obj} " in ln]
        link, = [ln for ln in db.build if f" -o {so} " in ln]
        # the command lines of the library before it, name for name
        assert compile_ == f"{_CC} -I../../include -c -o {obj} ntk_{row.name}.hip" and link == f"{_LD}{so} {obj} -L.. {_TAIL}"
        removed, = [ln.split() for ln in db.clean if ln.startswith("rm -f")]
        assert obj in removed and so in removed
    assert len(OLDER) == 12 and len(OLDER_LINES) == 26
    for line in OLDER_LINES:
        assert db.build.count(line) == 1, line
    # nothing else is built but the core's other objects
    rest = [ln for ln in db.build if ln not in OLDER_LINES and not any(f"ntk_{r.name}." in ln for r in ROWS)]
    assert len(rest) == 8 and all(re.search(r" -c -o ntk_(?:scan2|scan2_q|scan2_min|scan2_min2|fastx|fastx_codecs|fastx_api|pgzip)\.o ", ln) for ln in rest)
    assert len([ln for ln in db.clean if ln.startswith("rm -f")]) == 1


def test_the_staged_lists_name_the_same_libraries():
    """csrc/Makefile STAGED_LIBS, __graft_entry__.py STAGED_BINDINGS and STAGED_EXAMPLES, and the rows here, over whatever names they
    hold; the lists before them stay what they were."""
    import __graft_entry__ as G
    db = L.make_database()
    names = _staged_names()
    assert names == [r.name for r in ROWS] and len(set(names)) == len(names) >= 1 and set(names) <= set(STAGED)
    assert len(db.variables["CONSUMERS"].split()) == 10 and db.variables["MORE_LIBS"].split() == ["colors"]
    assert db.variables["LATER_LIBS"].split() == ["minimizer_list"]
    assert list(G.STAGED_BINDINGS) == [r.binding for r in ROWS]
    assert {lib for libs in G.STAGED_EXAMPLES.values() for lib in libs} >= set(names)
    earlier = set(_other_libraries()) - {""}
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    for r in ROWS:
        assert r.name not in earlier and r.name not in L.BY_NAME
        assert r.binding not in G.BINDINGS + G.MORE_BINDINGS + G.LATER_BINDINGS
        assert not any(r.example in d for d in (G.EXAMPLES, G.MORE_EXAMPLES, G.LATER_EXAMPLES, G.HOST_EXAMPLES))
        assert r.name in G.STAGED_EXAMPLES[r.example] and set(G.STAGED_EXAMPLES[r.example]) - set(names) <= earlier
        assert "examples/" + r.example in ignored
        for path in r.product_files():
            assert os.path.exists(path), path
        assert not os.path.exists(os.path.join(L.INCLUDE, f"needletail_amd_{r.name}.h"))
        assert not os.path.exists(os.path.join(L.INCLUDE, "needletail_amd", r.name + ".h")), "a staged header is not yet below include/"
        example = open(os.path.join(ROOT, "examples", r.example + ".cpp")).read()
        assert f'#include "{r.include}"' in example
    for example in G.STAGED_EXAMPLES:
        assert any(r.example == example for r in ROWS), (example, "an example program of no library")
    assert sorted(os.listdir(os.path.join(STAGED_INCLUDE, "needletail_amd"))) == sorted(r.name + ".h" for r in ROWS)
    assert os.listdir(STAGED_INCLUDE) == ["needletail_amd"]
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"-I" + os.path.join(ROOT, "include_staged")' in entry and "LATER_BINDINGS + STAGED_BINDINGS" in entry and "**STAGED_EXAMPLES" in entry


# ---- the stream contract ----------------------------------------------------------------------------------------------------------------

_SYNC = "(synchronous)"
CONTRACT = [
    SC.Row("ntk_seed_index_build_device", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_seed_index_spectrum", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_seed_index_match_device", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_seed_index_read", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_seed_index_result_device", SC.ASYNC, HEADER, "host-side only: queues nothing and waits for nothing", "decl", "test_stream_order"),
    SC.Row("ntk_seed_index_stats", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_seed_index_trim", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
]
FACADE = {"build_device": "si.build(", "spectrum": "si.spectrum(", "match_device": "si.match(", "read": "si.read", "result_device": "si.device_arrays",
          "stats": "si.stats", "trim": "si.trim"}


def test_stream_contract_of_the_seven_calls():
    text = open(HEADER).read()
    decl = {name: (params, near) for name, params, near in SC.declarations(text)}
    assert sorted(decl) == sorted(ROW.module.PREFIX + c for c in ROW.calls if c != "destroy")
    with_pointer = {name for name, (params, _) in decl.items() if SC.takes_device_pointer(params)}
    assert with_pointer == {"ntk_seed_index_build_device", "ntk_seed_index_match_device", "ntk_seed_index_result_device"}
    rows = {r.function: r for r in CONTRACT}
    assert len(rows) == len(CONTRACT) == 7 and with_pointer <= set(rows)
    assert set(rows) == set(decl) - {"ntk_seed_index_create"}, "every call that queues work or waits for the stream has a row"
    gpu = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    assert re.search(r"^pytestmark = pytest\.mark\.gpu", gpu, re.M)
    for r in CONTRACT:
        assert r.where == "decl" and SC.plain(r.words) in SC.plain(decl[r.function][1]), (r.function, "the words are not at the declaration")
        said = SC.plain(r.words).lower()
        if r.cls == SC.ASYNC:
            assert re.search(r"async|queued on the stream|queues nothing", said), r.function
        else:
            assert r.cls == SC.SYNC and re.search(r"synchronises|synchronise it|synchronous", said) and "may" not in said, r.function
        body = re.search(rf"^def {re.escape(r.test)}\(.*?(?=^def |^class |\Z)", gpu, re.M | re.S)
        assert body and FACADE[r.function.replace(ROW.module.PREFIX, "")] in body.group(0), (r.function, r.test)
    head = SC.plain(SC.head_comment(text))
    assert "build_device, spectrum, match_device, read, stats and trim are SYNCHRONOUS" in head and "result_device is host-side only" in head
    assert "stay valid until the next build_device, match_device, trim or destroy" in SC.plain(decl["ntk_seed_index_result_device"][1])
    # the earlier inventories see no header of this library
    assert not any("seed_index" in h for h in SC.shipped_headers()) and sorted(SC.shipped_headers()) == sorted(SC.HEADERS)


# ---- the library's own --------------------------------------------------------------------------------------------------------------------

def test_refusals_that_need_no_device():
    from needletail_amd import seeding as SD
    lib = SD.lib()
    bogus = C.c_void_p(8)   # never touched: the refusal comes first
    h, n = C.c_void_p(), C.c_uint64(5)
    assert lib.ntk_seed_index_create(None, C.byref(h)) == 2 and lib.ntk_seed_index_create(bogus, None) == 2 and not h.value
    assert lib.ntk_seed_index_build_device(None, bogus, bogus, bogus, bogus, 1, 1) == 2
    assert lib.ntk_seed_index_match_device(None, bogus, bogus, bogus, bogus, 1, 1, 0, 0) == 2
    assert lib.ntk_seed_index_spectrum(None, None, 8) == 2
    assert lib.ntk_seed_index_read(None, None, None, None, None, None, 0, C.byref(n)) == 2 and n.value == 5
    assert lib.ntk_seed_index_result_device(None, None, None, None, None, None, C.byref(n)) == 2
    assert lib.ntk_seed_index_stats(None, None) == 2 and lib.ntk_seed_index_trim(None) == 2
    lib.ntk_seed_index_destroy(None)
    # a handle's own refusals come before any device call, and the verification on the device before anything held is touched
    src = L.no_comments(open(HIP).read())
    check = re.search(r"int check_list\(.*?\n\}", src, re.S).group(0)
    assert "(n >> 32) || (n_records >> 31)" in check and "(uintptr_t)d_offsets & 7" in check and "(uintptr_t)d_info & 3" in check and "hip" not in check
    for call, starts in (("build_device", "m->built = m->matched = false"), ("match_device", "m->matched = true")):
        body = re.search(rf"int ntk_seed_index_{call}\(.*?\n\}}", src, re.S).group(0)
        order = [body.index(s) for s in ("check_list(m, d_offsets", "verify(m, d_offsets", starts, f"rc = {call.split('_')[0]}(m,")]
        assert order == sorted(order) and "hip" not in body, call
    match = re.search(r"int ntk_seed_index_match_device\(.*?\n\}", src, re.S).group(0)
    assert match.index("if (!m->built) return NTK_ERR_BAD_ARG;") < match.index("verify(m, d_offsets")
    verify = re.search(r"\nint verify\(.*?\n\}", src, re.S).group(0)
    assert re.findall(r"m->(\w+)\.ensure", verify) == ["d_ctr"] and "release" not in verify
    assert verify.index("SI_BAD_OFFSETS) return NTK_ERR_BAD_ARG") < verify.index("SI_BAD_POS) return NTK_ERR_UNSUPPORTED")
    cap = re.search(r"\nint match\(.*?\n\}", src, re.S).group(0)
    assert cap.index("return NTK_ERR_CAPACITY;") < cap.index("m->d_a_ref_rev.ensure("), "the capacity rule comes before any anchor array is grown"


def test_allocation_arithmetic_is_the_headers_memory_statement():
    """The header's memory statement, term by term, against the `ensure` calls of the source and the model's arithmetic."""
    src, hdr = open(HIP).read(), SC.plain(SC.head_comment(open(HEADER).read()))
    ensures = re.findall(r"\b(d_\w+)\.ensure\((?:m->stream|st), (.+?), (grow_\w+)\)", src)
    assert ensures == [
        ("d_ctr", "kCtrWords", "grow_exact"),
        ("d_sorted", "n", "grow_exact"), ("d_idx", "n", "grow_exact"), ("d_perm", "n", "grow_exact"), ("d_owner", "n", "grow_exact"),
        ("d_head", "n", "grow_exact"), ("d_rank", "n", "grow_exact"),
        ("d_keys", "n_keys", "grow_exact"), ("d_start", "n_keys + 1", "grow_exact"), ("d_ref", "n", "grow_exact"), ("d_rpos", "n", "grow_exact"),
        ("d_key_a", "n", "grow_exact"), ("d_key_b", "n", "grow_exact"), ("d_qpos_a", "n", "grow_exact"), ("d_qpos_b", "n", "grow_exact"),
        ("d_hit", "n_seeds", "grow_exact"), ("d_count", "n_seeds + 1", "grow_exact"), ("d_base", "n_seeds + 1", "grow_exact"),
        ("d_seg_begin", "n_reads", "grow_exact"), ("d_seg_end", "n_reads", "grow_exact"), ("d_a_offsets", "n_reads + 1", "grow_exact"), ("d_rows", "4 * n_reads", "grow_exact"),
        ("d_a_ref_rev", "total", "grow_half_again"), ("d_a_rpos", "total", "grow_half_again"), ("d_a_qpos", "total", "grow_half_again"),
        ("d_hist", "n_bins", "grow_exact"), ("d_ctr", "kCtrWords", "grow_exact")]
    for decl in ("DeviceArray<uint64_t> d_keys;", "DeviceArray<uint32_t> d_start, d_ref, d_rpos;", "DeviceArray<uint32_t> d_a_ref_rev, d_a_rpos, d_a_qpos;",
                 "DeviceArray<uint64_t> d_a_offsets;", "DeviceArray<uint32_t> d_rows;", "DeviceArray<uint64_t> d_sorted;",
                 "DeviceArray<uint32_t> d_idx, d_perm, d_owner, d_head, d_rank;", "DeviceArray<uint32_t> d_hit, d_count;",
                 "DeviceArray<uint64_t> d_base, d_seg_begin, d_seg_end;", "DeviceArray<uint64_t> d_key_a, d_key_b;", "DeviceArray<uint32_t> d_qpos_a, d_qpos_b;",
                 "DeviceArray<uint64_t> d_hist, d_ctr;", "DeviceArray<char> d_tmp;", "kCtrWords = 4;"):
        assert decl in src, decl
    assert "12 B per key and 4 more" in hdr and "8 B per occurrence" in hdr and M.index_bytes(1, 1) - M.index_bytes(0, 0) == 20
    assert "12 B per anchor and 8 + 16 B per read and 8 more" in hdr
    assert "the build's, 28 B per entry" in hdr and M.device_bytes(0, 1) - M.device_bytes(0, 0) == 8 + 28
    assert "the match's, 16 B per seed and 12 more" in hdr and "16 B per read (the long reads' segments)" in hdr
    assert M.device_bytes(0, 0, n_reads=0) - M.device_bytes(0, 0) == 12 + 8
    assert M.device_bytes(0, 0, n_reads=1, n_seeds=1) - M.device_bytes(0, 0, n_reads=0) == 16 + 16 + 24
    assert "24 B per anchor of the reads that have more than 2048" in hdr and "the spectrum's bins, 8 B each" in hdr and "4 counter words" in hdr
    assert M.device_bytes(0, 0, n_reads=0, long_anchors=1) - M.device_bytes(0, 0, n_reads=0) == 24
    assert "The anchor arrays grow by half again and 64 to the largest batch so far" in hdr and M.half_again(100) == 214
    assert "every other array but the index's grows to exactly the largest size needed so far" in hdr
    # rocPRIM's temporary storage is held inside a call only, so device_bytes between calls has no term of unknown size: both calls
    # that use it drop it on every way out, and a build replaces the index arrays instead of growing them
    assert "is held INSIDE a build_device or match_device only and freed before the call returns" in hdr
    code = L.no_comments(src)
    for call, run in (("build_device", "rc = build(m,"), ("match_device", "rc = match(m,")):
        body = re.search(rf"int ntk_seed_index_{call}\(.*?\n\}}", code, re.S).group(0)
        after = body[body.index(run):]
        assert 0 < after.index("drop_tmp(m);") < after.index("if (rc") and "return" not in after[: after.index("drop_tmp(m);")], call
    assert len(re.findall(r"\bdrop_tmp\(m\)", code)) == 2 and "m->d_tmp.release();" in re.search(r"void drop_tmp\(.*?\n\}", code, re.S).group(0)
    assert "with_tmp" not in re.search(r"int ntk_seed_index_spectrum\(.*?\n\}", code, re.S).group(0) and "with_tmp" not in re.search(r"int occ_pass\(.*?\n\}", code, re.S).group(0)
    build = re.search(r"int ntk_seed_index_build_device\(.*?\n\}", code, re.S).group(0)
    assert build.index("verify(m, d_offsets") < build.index("m->release_index();") < build.index("rc = build(m,")
    # the only arrays of the handle are those above; device_bytes names every one, and trim frees all but the index
    struct = re.search(r"struct ntk_seed_index : Consumer \{(.*?)\n\};", src, re.S).group(1)
    arrays = set(re.findall(r"\b(d_[a-z_]+)[;,]", struct.split("uint64_t device_bytes")[0]))
    index = {"d_keys", "d_start", "d_ref", "d_rpos"}
    assert arrays == index | {"d_a_ref_rev", "d_a_rpos", "d_a_qpos", "d_a_offsets", "d_rows", "d_sorted", "d_idx", "d_perm", "d_owner", "d_head",
                              "d_rank", "d_hit", "d_count", "d_base", "d_seg_begin", "d_seg_end", "d_key_a", "d_key_b", "d_qpos_a", "d_qpos_b", "d_hist", "d_ctr", "d_tmp"}
    count = re.search(r"uint64_t device_bytes\(\) const\s*\{(.*?)\n    \}", src, re.S).group(1)
    work = re.search(r"void release_work\(\)\s*\{(.*?)\n    \}", src, re.S).group(1)
    held = re.search(r"void release_index\(\) \{(.*?)\}", src).group(1)
    for a in arrays:
        assert count.count(a + ".bytes()") == 1, (a, "counted once")
        assert (a + ".release()" in held) == (a in index) and (a + ".release()" in work) == (a not in index), a
    assert "out->device_bytes = m->device_bytes();" in src
    trim = re.search(r"int ntk_seed_index_trim\(.*?\n\}", src, re.S).group(0)
    assert "release_work()" in trim and "release_index" not in trim, "THE INDEX STAYS"
    gpu = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    assert 'st["device_bytes"] == M.index_bytes(index.n_keys, index.n_entries)' in gpu and "n_cu() * M.BLOCKS_PER_CU * M.THREADS" in gpu
