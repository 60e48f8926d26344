"""CPU-side checks of the minimizer-list library (include/needletail_amd/minimizer_list.h, libneedletail_amd_minimizer_list.so).

The library is stated beside the ten rows of tests/_libraries.py and beside the coloured index (csrc/Makefile LATER_LIBS,
__graft_entry__.py LATER_BINDINGS / LATER_EXAMPLES), and its public header lies in include/needletail_amd/, where a library's header goes
from now on.  Its row is made here from a Library whose `header` is that path, put through the check_* functions every row is held to,
and check_header and the four checks tests/test_consumer_abi.py parametrises over the ten are restated for this layout.  ROWS is a list:
the checks of the later lists are written over it, so the next library adds a row (in a file of its own or here) and no fourth copy.
Then what is the library's own: the stream contract of its five calls, the refusals that need no device, the header's memory statement
against the `ensure` calls, and the model's restatement of it."""
import ctypes as C
import os
import re
import subprocess

import _builds as B
import _libraries as L
import _minimizer_list_model as MM
import _stream_contract as SC

ROOT = L.ROOT
GPU_TESTS = "test_gpu_minimizer_list.py"


class LaterLibrary(L.Library):
    """A row whose public header is include/needletail_amd/NAME.h."""
    __slots__ = ()
    header = property(lambda s: os.path.join(L.INCLUDE, "needletail_amd", s.name + ".h"))
    include = property(lambda s: "needletail_amd/" + s.name + ".h")                       # as a program names it with -Iinclude
    make_header = property(lambda s: "../../include/needletail_amd/" + s.name + ".h")    # as csrc/Makefile names it


ROW = LaterLibrary(
    "minimizer_list", binding="minimizer_lists", cls="MinimizerList",
    calls=("create", "destroy", "run_device", "read", "result_device", "stats", "trim"),
    headers=("ntk_ml_rule.hpp",), example="minimizers", bench="minimizer_list_bench", gpu_tests=GPU_TESTS, kernels={
        "ml_select_kernel": "test_tile_seams_of_the_select_kernel",
        "ml_scan_kernel": "test_more_tiles_than_one_step_of_the_grid",
        "ml_scatter_kernel": "test_more_tiles_than_one_step_of_the_grid",
        "ml_offsets_kernel": "test_random_records_match_the_model",
    }, leak=r"(?:^|::)ml_",
    c_main="struct ntk_minimizer_list_stats s; s.w = NTK_MINIMIZER_LIST_W_MAX; s.order = NTK_MINIMIZER_LIST_HASH; "
    "return sizeof s == 56 && s.w == 256 && s.order == 1 && NTK_MINIMIZER_LIST_LEX == 0 && "
    "NTK_MINIMIZER_LIST_XOR == 0x9E3779B97F4A7C15ull ? 0 : 1;",
    no_device=lambda nt: nt.MinimizerList(21, nt.PATH_BYTES_CANONICAL, 11), prim=None, shape=r"::ml_[a-z_]+_kernel\b", n_global=4)
ROWS = [ROW]
HEADER, HIP, RULE_HPP = ROW.header, ROW.hip, os.path.join(L.CSRC, "ntk_ml_rule.hpp")


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
    """check_header for a header below include/needletail_amd/: a C11 program names it as users do, its only include is the core's, and
    the public headers its object depends on are itself and the core's."""
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(f'#include "{ROW.include}"\nint main(void) {{ {ROW.c_main} }}\n')
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + L.INCLUDE, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0, "a struct size or a constant is not the stated one"
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HEADER).read()) == ["needletail_amd.h"]
    named = {p for p in L.make_database().prerequisites["ntk_minimizer_list.o"] if p.startswith("../../include/")}
    assert named == {ROW.make_header, L.public_header("")}
    from needletail_amd import minimizer_lists as ML
    assert C.sizeof(ML.Stats) == 56 and [n for n, _ in ML.Stats._fields_] == list(MM.STATS) == _struct_fields("ntk_minimizer_list_stats")
    assert (ML.LEX, ML.HASH, ML.W_MAX, ML.XOR) == (MM.LEX, MM.HASH, MM.W_MAX, MM.XOR) == (0, 1, 256, 0x9E3779B97F4A7C15)


def _struct_fields(struct):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct %s \{(.*?)\};" % struct, hdr, re.S).group(1)
    return [f.strip() for decl in re.findall(r"uint(?:64|32)_t ([^;]+);", body) for f in decl.split(",")]


# ---- the four checks tests/test_consumer_abi.py parametrises over the rows, for this layout -------------------------------------------------

def test_library_links_exactly_what_it_needs_by_rpath():
    out = subprocess.run(["readelf", "-d", L.built(ROW.so)], capture_output=True, text=True).stdout
    needed = [n for n in re.findall(r"NEEDED.*\[(.*?)\]", out) if n.startswith("libneedletail_amd")]
    assert "$ORIGIN" in out
    assert needed == [os.path.basename(L.so_path(n)) for n in ROW.links + ("",)], needed


def test_no_kernel_leaks_into_or_out_of_the_library():
    """No ml_ kernel in any of the twelve other shared objects, and none of theirs in this one."""
    import test_colors_abi as colors
    own = B.library_kernels(L.built(ROW.so))
    assert own and all(re.search(ROW.leak, n) for n in own), "the pattern no longer names the library's own kernels"
    assert not own & B.library_kernels(L.built(L.so_path("")))
    others = {"": None, **{r.name: r.leak for r in L.LIBRARIES}, colors.ROW.name: colors.ROW.leak}
    assert len(others) == 12
    for other, leak in others.items():
        theirs = B.library_kernels(L.built(L.so_path(other)))
        assert not {n for n in theirs if re.search(ROW.leak, n)}, other or "core"
        if leak:
            assert not {n for n in own if re.search(leak, n)}, other
    names = " ".join(re.findall(r"\b(?:struct|void|int)\s+(\w+)", L.no_comments(open(HIP).read() + open(RULE_HPP).read())))
    assert not re.search(r"abundance|sketch|minhash|read_trim", names), "a name another library's leak pattern would match"


def test_the_shared_pieces_are_used_and_not_defined_again():
    """The scaffold comes from ntk_consumer.hpp and memory from ntk_device_mem.hpp; neither new file defines a piece of them again or
    names an allocation call, comments included, or the wide walk.  Plain HIP C++, no inline assembly, no floating point."""
    from test_consumer_abi import MEM_DEFS, SHARED
    src, rule = open(HIP).read(), open(RULE_HPP).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_ml_rule.hpp"' in src
    assert '#include "../../include/needletail_amd/minimizer_list.h"' in src
    for text in (src, rule):
        for name in SHARED:
            assert not re.search(rf"\b{name}\([^)]*\)\s*\{{", text), (name, "defined again")
        for pat in MEM_DEFS:
            assert not re.search(pat, text), (pat, "defined again")
        assert not re.search(r"struct (?:MaterialiseScratch|Consumer)\b\s*\{", text)
        assert not re.search(r"hip(?:Host)?(?:Malloc|Free)\b", text), "the memory layer allocates"
        assert "ntk_wide_walk" not in text and "rocprim" not in text
        code = L.no_comments(text)
        assert not re.search(r"\basm\b|__asm", code), "plain HIP C++"
        assert not re.search(r"\b(?:double|float)\b", code), "no floating point anywhere in the library"
    code = L.no_comments(src)
    for name in ("add_agent", "block_sum_u32", "grid_for", "chunk_at", "chunk_scratch_bases", "check_batch_params", "check_batch_pointers",
                 "ml_key", "ml_pair", "ml_double_at", "ml_window_at", "ml_sel_word", "ml_span", "ml_info"):
        assert re.search(rf"\b{name}\(", code), name
    assert not re.search(r"\bfor_each_chunk\(", code), "the halo of for_each_chunk is k - 1: this library walks the chunks itself"
    assert "chunk_at(n_bytes, reach, start)" in code and "const uint32_t reach = m->k + m->w;" in code
    assert "MaterialiseScratch scratch;" in src and "struct ntk_minimizer_list : Consumer {" in src
    assert not re.search(r"kChunkBases\s*=", src), "the chunk length is ntk_chunks.hpp's alone"
    for f in ("ntk_consumer.hpp", "ntk_chunks.hpp", "ntk_device_mem.hpp"):
        assert "minimizer_list" not in open(os.path.join(L.CSRC, f)).read() and "ntk_ml_" not in open(os.path.join(L.CSRC, f)).read(), f


def test_build_rule_is_the_rows():
    db = L.make_database()
    for row in ROWS:
        obj, so = f"ntk_{row.name}.o", f"../libneedletail_amd_{row.name}.so"
        assert db.prerequisites[obj] == {f"ntk_{row.name}.hip", *row.headers, *L.CONSUMER_HPP, row.make_header, L.public_header("")}
        assert db.prerequisites[so] == {obj, "../libneedletail_amd.so"}
        assert so in db.prerequisites["all"]
        compile_, = [ln for ln in db.build if f" -c -o {obj} " in ln]
        link, = [ln for ln in db.build if f" -o {so} " in ln]
        assert compile_.endswith(f" ntk_{row.name}.hip") and "--offload-arch=gfx950" in compile_
        assert re.findall(r"-l(\S+)", link) == ["needletail_amd"] and f" {obj} " in link
        # the command lines of a library of the ten, name for name, but for include/ on the search path of the object
        as_dbg = lambda ln: ln.replace(row.name, "dbg")   # noqa: E731
        assert as_dbg(compile_).replace(" -I../../include", "") in db.build and " -I../../include " in compile_ and as_dbg(link) in db.build
        removed, = [ln.split() for ln in db.clean if ln.startswith("rm -f")]
        assert obj in removed and so in removed


def test_the_later_lists_name_the_same_libraries():
    """csrc/Makefile LATER_LIBS, __graft_entry__.py LATER_BINDINGS and LATER_EXAMPLES, and the rows here; the ten stay the ten and the
    second list stays the coloured index."""
    import __graft_entry__ as G
    db = L.make_database()
    names = [r.name for r in ROWS]
    assert db.variables["LATER_LIBS"].split() == names and len(set(names)) == len(names)
    assert len(db.variables["CONSUMERS"].split()) == 10 and db.variables["MORE_LIBS"].split() == ["colors"]
    assert list(G.LATER_BINDINGS) == [r.binding for r in ROWS]
    assert {lib for libs in G.LATER_EXAMPLES.values() for lib in libs} >= set(names)
    earlier = {r.name for r in L.LIBRARIES} | {"colors"}
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    for r in ROWS:
        assert r.name not in db.variables["CONSUMERS"].split() + db.variables["MORE_LIBS"].split() and r.name not in L.BY_NAME
        assert r.binding not in G.BINDINGS + G.MORE_BINDINGS and r.example not in G.EXAMPLES and r.example not in G.MORE_EXAMPLES
        assert r.name in G.LATER_EXAMPLES[r.example] and set(G.LATER_EXAMPLES[r.example]) - set(names) <= earlier
        assert "examples/" + r.example in ignored
        for path in r.product_files():
            assert os.path.exists(path), path
        assert not os.path.exists(os.path.join(L.INCLUDE, f"needletail_amd_{r.name}.h")), "a later library's header lies in include/needletail_amd/"
    for example in G.LATER_EXAMPLES:
        assert any(r.example == example for r in ROWS), (example, "an example program of no library")
    assert sorted(os.listdir(os.path.join(L.INCLUDE, "needletail_amd"))) == sorted(r.name + ".h" for r in ROWS)


# ---- the stream contract ----------------------------------------------------------------------------------------------------------------

_SYNC = "(synchronous)"
CONTRACT = [
    SC.Row("ntk_minimizer_list_run_device", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_minimizer_list_read", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_minimizer_list_result_device", SC.ASYNC, HEADER, "host-side only: queues nothing and waits for nothing", "decl", "test_stream_order"),
    SC.Row("ntk_minimizer_list_stats", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_minimizer_list_trim", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
]
FACADE = {"run_device": "ml.run_device(", "read": "ml.read", "result_device": "ml.device_arrays", "stats": "ml.stats", "trim": "ml.trim"}


def test_stream_contract_of_the_five_calls():
    text = open(HEADER).read()
    decl = {name: (params, near) for name, params, near in SC.declarations(text)}
    assert sorted(decl) == sorted(ROW.module.PREFIX + c for c in ROW.calls if c != "destroy")
    with_pointer = {name for name, (params, _) in decl.items() if SC.takes_device_pointer(params)}
    assert with_pointer == {"ntk_minimizer_list_run_device", "ntk_minimizer_list_result_device"}
    rows = {r.function: r for r in CONTRACT}
    assert len(rows) == len(CONTRACT) == 5 and with_pointer <= set(rows)
    assert set(rows) == set(decl) - {"ntk_minimizer_list_create"}, "every call that queues work or waits for the stream has a row"
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
    assert "run_device, read, stats and trim are SYNCHRONOUS" in head and "result_device is host-side only" in head
    assert "stay valid until the next run_device, trim or destroy" in SC.plain(decl["ntk_minimizer_list_result_device"][1])


# ---- the library's own --------------------------------------------------------------------------------------------------------------------

def test_refusals_that_need_no_device():
    import needletail_amd as nt
    from needletail_amd import minimizer_lists as ML
    lib = ML.lib()
    bogus = C.c_void_p(8)   # never touched: the refusal comes first
    for k in (0, 33, 64):
        h = C.c_void_p()
        assert lib.ntk_minimizer_list_create(bogus, k, 0, 11, 0, C.byref(h)) == 1 and not h.value, k
    for k, path, w, order in ((21, 3, 11, 0), (21, 0, 0, 0), (21, 0, 257, 0), (21, 0, 11, 2), (32, 2, 1000, 1)):
        h = C.c_void_p()
        assert lib.ntk_minimizer_list_create(bogus, k, path, w, order, C.byref(h)) == 2 and not h.value
    h = C.c_void_p()
    assert lib.ntk_minimizer_list_create(None, 21, 0, 11, 0, C.byref(h)) == 2 and lib.ntk_minimizer_list_create(bogus, 21, 0, 11, 0, None) == 2
    p = nt._lib.Params(21, 0, 2, 0)
    n = C.c_uint64(5)
    assert lib.ntk_minimizer_list_run_device(None, None, None, 0, None, 0, C.byref(p)) == 2
    assert lib.ntk_minimizer_list_read(None, None, None, None, None, 0, C.byref(n)) == 2 and n.value == 5
    assert lib.ntk_minimizer_list_result_device(None, None, None, None, None, C.byref(n)) == 2
    assert lib.ntk_minimizer_list_stats(None, None) == 2 and lib.ntk_minimizer_list_trim(None) == 2
    lib.ntk_minimizer_list_destroy(None)
    # a handle's own refusals come before any device call: they are the scaffold's, on a struct that says k, path (text for text below)
    src = L.no_comments(open(HIP).read())
    run = re.search(r"int ntk_minimizer_list_run_device\(.*?\n\}", src, re.S).group(0)
    order = [run.index(s) for s in ("check_batch_params(m, p)", "n_records >> 32", "check_batch_pointers(d_seq, d_qual)", "(uintptr_t)d_offsets & 7",
                                    "m->held = true", "hold_empty(m, n_records) : run(m,")]
    assert order == sorted(order) and "hip" not in run[: run.index("m->held = true")]
    create = re.search(r"int ntk_minimizer_list_create\(.*?\n\}", src, re.S).group(0)
    assert create.index("NTK_ERR_BAD_K") < create.index("w > NTK_MINIMIZER_LIST_W_MAX") < create.index("m->bind(ctx, k, path)")
    consumer = open(os.path.join(L.CSRC, "ntk_consumer.hpp")).read()
    assert "if (p->path == NTK_PATH_BYTES_CANONICAL && p->pre < NTK_PRE_NORMALIZE) return NTK_ERR_UNSUPPORTED;" in consumer
    assert "p->k != h->k || p->path != h->path || (p->flags & ~0xFF00u) != 0" in consumer


def test_allocation_arithmetic_is_the_headers_memory_statement():
    """The header's memory statement, term by term, against the `ensure` calls of the source: one chunk of the materialise face with its
    halo and tail, the held list and the record ranges, and the compaction's work arrays.  Nothing else is allocated, so nothing is
    proportional to the bases of the batch beyond one chunk."""
    src, hdr = open(HIP).read(), SC.plain(SC.head_comment(open(HEADER).read()))
    ensures = re.findall(r"\b(d_\w+)\.ensure\((?:m->stream|st), (.+?), (grow_\w+)(?:, ([^)]+))?\)", src)
    assert ensures == [
        ("d_offsets_out", "n_records + 1", "grow_half_again", ""),           # an empty run holds n_records empty ranges
        ("d_ctr", "kCtrWords", "grow_exact", ""), ("d_offsets_out", "n_records + 1", "grow_half_again", ""),
        ("d_sel", "(bases + 15) & ~(uint64_t)15", "grow_exact", ""),
        ("d_count", "tiles_max + 1", "grow_exact", ""), ("d_tile_base", "tiles_max + 1", "grow_exact", ""),
        ("d_pos", "need", "grow_half_again", "m->n_entries"), ("d_value", "need", "grow_half_again", "m->n_entries"),
        ("d_info", "need", "grow_half_again", "m->n_entries"), ("d_end", "need", "grow_half_again", "m->n_entries")]
    assert "(rc = m->scratch.ensure(st, bases))" in src
    assert "const uint64_t bases = chunk_scratch_bases(n_bytes, reach) + (n_bytes > kChunkBases ? m->w - 1 : 0);" in src
    assert "const uint64_t tiles_max = (chunk_bases(n_bytes) + m->w - 1 + ML_TILE - 1) / ML_TILE;" in src
    for decl in ("DeviceArray<uint64_t> d_pos, d_value;", "DeviceArray<uint32_t> d_info;", "DeviceArray<uint64_t> d_offsets_out;", "DeviceArray<uint64_t> d_end;",
                 "DeviceArray<uint16_t> d_sel;", "DeviceArray<uint32_t> d_count, d_tile_base;", "DeviceArray<uint64_t> d_ctr;", "kCtrWords = 2;"):
        assert decl in src, decl
    assert "8.25 B per base; 64 Mi bases plus a halo of at most 288 and a tail of at most 255 bases" in hdr and MM.halo(32, 256) == 288
    assert "the held list, 20 B per entry plus 8 B per record" in hdr
    assert "the first window ends, 8 B per entry" in hdr and "the window ends' words, 2 B per base of one chunk" in hdr
    assert "the tiles' counts and their scan, 8 B per 1024 bases of one chunk" in hdr and "2 counter words" in hdr and MM.TILE == 1024
    assert "grow by half again and 64" in hdr and "No array is proportional to the bases of the batch beyond one chunk" in hdr
    # the only arrays of the handle are those above, and device_bytes and release_all name every one of them
    struct = re.search(r"struct ntk_minimizer_list : Consumer \{(.*?)\n\};", src, re.S).group(1)
    arrays = set(re.findall(r"\b(d_[a-z_]+)[;,]", struct.split("uint64_t device_bytes")[0]))
    assert arrays == {"d_pos", "d_value", "d_info", "d_offsets_out", "d_end", "d_sel", "d_count", "d_tile_base", "d_ctr"}
    count = re.search(r"uint64_t device_bytes\(\) const\s*\{(.*?)\n    \}", src, re.S).group(1)
    free = re.search(r"void release_all\(\)\s*\{(.*?)\n    \}", src, re.S).group(1)
    for a in arrays | {"scratch"}:
        assert a + ".bytes()" in count or a + ".device_bytes()" in count, a
        assert a + ".release()" in free, a
    assert "out->device_bytes = m->device_bytes();" in src


def test_the_models_device_bytes_is_the_statement():
    """What the GPU test holds stats.device_bytes to: the same terms, in numbers."""
    assert MM.device_bytes(0, 0, 21, 11, []) == 65 * 8
    assert MM.device_bytes(1600, 9, 21, 11, [100]) == 1600 * 8 + 2 * 100 * 2 + 1600 * 2 + 2 * 3 * 4 + 16 + (10 + 5 + 64) * 8 + (100 + 50 + 64) * 28
    assert MM.device_bytes(1600, 9, 21, 11, [0]) == MM.device_bytes(1600, 9, 21, 11, [100]) - 214 * 28
    rule = open(RULE_HPP).read()
    assert f"ML_TILE = {MM.TILE};" in rule and f"ML_BLOCKS_PER_CU = {MM.BLOCKS_PER_CU};" in rule and f"ML_W_MAX = {MM.W_MAX};" in rule
    chunks = open(os.path.join(L.CSRC, "ntk_chunks.hpp")).read()
    assert "kChunkBases = (uint64_t)64 << 20;" in chunks and MM.CHUNK == 64 << 20
    gpu = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    assert "MM.device_bytes(I.CHUNK_BYTES, 1, k, w, per_chunk)" in gpu and "n_cu() * MM.BLOCKS_PER_CU" in gpu
