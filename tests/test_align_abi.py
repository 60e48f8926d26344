"""CPU-side checks of the alignment library (include_pending/needletail_amd/align.h, libneedletail_amd_align.so).

The library is stated in the pending place beside the chain and mapping libraries (csrc/Makefile PENDING_LIBS and its goal `pending`,
__graft_entry__.py PENDING_BINDINGS / PENDING_EXAMPLES), and its public header waits in include_pending/needletail_amd/ under the include
spelling it will have in include/needletail_amd/.  Its row is made here from a Library whose `header` is that path - the PendingLibrary
row of tests/test_mapping_abi.py restated - and put through the check_* functions of tests/_libraries.py; check_header and the checks
tests/test_consumer_abi.py parametrises over the ten are restated for this layout.  THE PLACE STAYS OPEN: every check here is about
this library's own row, so the next pending library changes nothing in this file.  Then what is the library's own: the stream contract
of its calls, the refusals that need no device, and the header's memory statement against the `ensure` calls."""
import ctypes as C
import os
import re
import subprocess

import _align_model as M
import _builds as B
import _libraries as L
import _stream_contract as SC

ROOT = L.ROOT
STAGED_INCLUDE = os.path.join(ROOT, "include_staged")
PENDING_INCLUDE = os.path.join(ROOT, "include_pending")
INCLUDE_DIRS = (L.INCLUDE, STAGED_INCLUDE, PENDING_INCLUDE)
GPU_TESTS = "test_gpu_align.py"


class PendingLibrary(L.Library):
    """A row whose public header is include_pending/needletail_amd/NAME.h."""
    __slots__ = ()
    header = property(lambda s: os.path.join(PENDING_INCLUDE, "needletail_amd", s.name + ".h"))
    include = property(lambda s: "needletail_amd/" + s.name + ".h")                               # as a program names it with the three -I
    make_header = property(lambda s: "../../include_pending/needletail_amd/" + s.name + ".h")    # as csrc/Makefile names it


ROW = PendingLibrary(
    "align", binding="aligning", cls="ChainAlignments", calls=("create", "destroy", "run_device", "read", "result_device", "stats", "trim"),
    headers=("ntk_align_rule.hpp",), example="align_reads", bench="align_bench", gpu_tests=GPU_TESTS, kernels={
        "aln_verify_kernel": "test_refusals_leave_the_held_result_unchanged", "aln_plan_kernel": "test_max_seg", "aln_dp_kernel": "test_strip_seams",
        "aln_trace_kernel": "test_band", "aln_emit_kernel": "test_ties_and_bases",
    }, leak=r"(?:^|::)aln_",
    c_main="struct ntk_align_stats s; struct ntk_align_params p; s.device_bytes = 8; p.work_mib = 32; "
    "return sizeof s == 72 && sizeof s.dp_cells == s.device_bytes && sizeof p == p.work_mib ? 0 : 1;",
    no_device=lambda nt: nt.ChainAlignments(), prim=("scan",), shape=r"::aln_[a-z]+_kernel\b", n_global=5)
HEADER, HIP, RULE_HPP = ROW.header, ROW.hip, os.path.join(L.CSRC, "ntk_align_rule.hpp")


def built(path):
    """`path`, a built library: the libraries, the pending ones among them, are built first if it is not there."""
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", L.CSRC, "all", "pending"])
    return path


def _pending_names():
    return L.make_database().variables["PENDING_LIBS"].split()


def _built_other(path):
    """A library before this one: those of the default goal by tests/_libraries.py, the pending ones by this file's `built`."""
    return built(path) if os.path.basename(path) in ("libneedletail_amd_%s.so" % n for n in _pending_names()) else L.built(path)


# ---- the checks of tests/_libraries.py ------------------------------------------------------------------------------------------------

def test_every_declared_function_is_exported_and_listed():
    built(ROW.so)
    L.check_exports(ROW)


def test_every_kernel_names_the_test_that_launches_it():
    built(ROW.so)
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    built(ROW.so)
    L.check_no_device(ROW)


def _struct_fields(struct):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct %s \{(.*?)\};" % struct, hdr, re.S).group(1)
    return [re.sub(r"\[\d+\]", "", f.strip()) for decl in re.findall(r"uint(?:64|32)_t ([^;]+);", body) for f in decl.split(",")]


def test_header_compiles_as_c_and_states_the_struct_sizes(tmp_path):
    """check_header for a pending header: a C11 program names it as users do, with the three include directories; its only include is
    the core's; the public headers its object depends on are itself and the core's."""
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(f'#include "{ROW.include}"\nint main(void) {{ {ROW.c_main} }}\n')
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", *("-I" + d for d in INCLUDE_DIRS), "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0, "a struct size or a constant is not the stated one"
    includes = lambda path: re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(path).read())   # noqa: E731
    assert includes(HEADER) == ["needletail_amd.h"]
    seen, todo = set(), [ROW.include]
    while todo:
        h = todo.pop()
        found = [os.path.join(d, h) for d in INCLUDE_DIRS if os.path.exists(os.path.join(d, h))]
        if h not in seen and found:
            assert len(found) == 1, (h, "in more than one include directory")
            seen.add(h)
            todo += includes(found[0])
    assert seen == {ROW.include, "needletail_amd.h"}
    named = {p for p in L.make_database().prerequisites["ntk_align.o"] if p.startswith("../../include")}
    assert named == {ROW.make_header, L.public_header("")}
    from needletail_amd import aligning as AL
    assert C.sizeof(AL.Stats) == 72 and [n for n, _ in AL.Stats._fields_] == list(M.STATS) == _struct_fields("ntk_align_stats")
    assert all(t is C.c_uint64 for _, t in AL.Stats._fields_)
    assert C.sizeof(AL.Params) == 32 and [n for n, _ in AL.Params._fields_] == _struct_fields("ntk_align_params") == list(M.Params._fields)
    assert AL.ERR_CAPACITY == M.ERR_CAPACITY == 5 and AL.SEG_MAX == M.SEG_MAX == 4095 and AL.SPAN_MAX == M.SPAN_MAX == 1 << 28
    assert AL.ROW == M.ROW and AL.OPS == M.OPS and (AL.ALIGNED, AL.TOO_LONG) == (M.ALIGNED, M.TOO_LONG)
    assert AL.cigar_string([3 << 4 | 7, 1 << 4 | 8, 2 << 4 | 1, 5 << 4 | 2]) == "3=1X2I5D" == M.cigar_string([55, 24, 33, 82])
    import inspect
    sig = inspect.signature(AL.ChainAlignments.run)
    assert [sig.parameters[n].default for n in M.Params._fields[1:]] == list(M.Params(7))[1:], "the defaults of run are the header's"


# ---- the checks tests/test_consumer_abi.py parametrises over the rows, for this layout -------------------------------------------------

def test_library_links_the_core_alone_by_rpath():
    out = subprocess.run(["readelf", "-d", built(ROW.so)], capture_output=True, text=True).stdout
    needed = [n for n in re.findall(r"NEEDED.*\[(.*?)\]", out) if n.startswith("libneedletail_amd")]
    assert "$ORIGIN" in out and needed == ["libneedletail_amd.so"], needed


def _other_libraries():
    """name -> leak pattern of the sixteen shared objects before this one ("" is the core, which has no pattern)."""
    import test_mapping_abi as mapping
    others = {**mapping._other_libraries(), mapping.ROW.name: mapping.ROW.leak}
    assert len(others) >= 16 and ROW.name not in others
    return others


def test_no_kernel_leaks_into_or_out_of_the_library():
    """No aln_ kernel in any of the shared objects before this one, and none of theirs in this one."""
    own = L.own_kernels(B.library_kernels(built(ROW.so)))
    assert own and all(re.search(ROW.leak, n) for n in own), "the pattern no longer names the library's own kernels"
    for other, leak in _other_libraries().items():
        theirs = B.library_kernels(_built_other(L.so_path(other)))
        assert not {n for n in theirs if re.search(ROW.leak, n)}, other or "core"
        assert not own & theirs, other or "core"
        if leak:
            assert not {n for n in own if re.search(leak, n)}, other
    names = " ".join(re.findall(r"\b(?:struct|void|int)\s+(\w+)", L.no_comments(open(HIP).read() + open(RULE_HPP).read())))
    assert not re.search(r"abundance|sketch|minhash|read_trim", names), "a name another library's leak pattern would match"


def test_the_shared_pieces_are_used_and_not_defined_again():
    """The scaffold comes from ntk_consumer.hpp and memory from ntk_device_mem.hpp; neither new file defines a piece of them again or
    names an allocation call, comments included.  Plain HIP C++, no inline assembly, no floating point; rocPRIM's temporary storage
    goes through with_tmp, and so through a DeviceArray.  The library reads bases only through the two batches it is given and names no
    other library."""
    from test_consumer_abi import MEM_DEFS, SHARED
    src, rule = open(HIP).read(), open(RULE_HPP).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_align_rule.hpp"' in src
    assert '#include "../../include_pending/needletail_amd/align.h"' in src
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
        assert not re.search(r"bitop3<|perm\(", text)
    code = L.no_comments(src)
    for name in ("grid_for", "with_tmp", "wave_sum", "add_agent", "aln_step", "aln_m0", "aln_band", "aln_in_band", "aln_border_h", "aln_row_width",
                 "aln_row_start", "aln_cell", "aln_trace", "aln_score", "aln_code", "aln_query_code", "aln_match", "aln_record_len", "aln_at_or_before"):
        assert re.search(rf"\b{name}\(", code), name
    assert "struct ntk_align : Consumer {" in src and "m->bind(ctx, 0, 0)" in src
    assert len(re.findall(r"rocprim::exclusive_scan\(", code)) == len(re.findall(r"with_tmp\(m->d_tmp, st, grow_exact,", code)) == 4
    assert "ntk_materialize" not in code and "MaterialiseScratch" not in code, "it reads the batches' bytes itself"
    # the only bytes read are those of the two batches: through a Chain's two record pointers, made from a.ref and a.seq alone
    assert re.findall(r"\ba\.(?:ref|seq)\b(?!_)", code) == ["a.ref", "a.seq", "a.ref", "a.seq"], "set in run_device, used in chain_of"
    assert "ch.ref = a.ref + a.ref_offsets[ref_rev >> 1];" in code and "ch.read = a.seq + a.seq_offsets[q];" in code
    for f in ("ntk_consumer.hpp", "ntk_chunks.hpp", "ntk_device_mem.hpp"):
        assert "ntk_align" not in open(os.path.join(L.CSRC, f)).read() and "aln_" not in open(os.path.join(L.CSRC, f)).read(), f
    assert not re.search(r"ntk_seed_index|ntk_minimizer_list|ntk_chain|ntk_mapping|mp_", code + L.no_comments(rule)), \
        "it takes chains, anchors and the selection as arrays and links no library that makes them"
    assert "__shfl_up(" in code and "extern __shared__" in code and "__ballot(" in code, "the DP kernel's wave shift and row in LDS"


_CC = "/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "
_LD = "/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o "
_TAIL = "-lneedletail_amd -Wl,-rpath,'$ORIGIN'"


def _make_lines(*goals):
    out = subprocess.run(["make", "-n", "-B", "-C", L.CSRC, "ARCH=gfx950", *goals], capture_output=True, text=True, check=True).stdout
    return [ln for ln in out.splitlines() if ln and not ln.startswith(("make", "#"))]


def test_build_rule_and_command_lines_of_the_library():
    """The object's and the library's prerequisites and command lines are those of the library before it, name for name; the goal
    `pending` builds it and the default goal does not; `clean` removes it in its one rm line."""
    db = L.make_database()
    obj, so = "ntk_align.o", "../libneedletail_amd_align.so"
    assert db.prerequisites[obj] == {"ntk_align.hip", *ROW.headers, *L.CONSUMER_HPP, ROW.make_header, L.public_header("")}
    assert db.prerequisites[so] == {obj, "../libneedletail_amd.so"}
    assert so in db.prerequisites["pending"] and so not in db.prerequisites["all"] and "pending" not in db.prerequisites["all"]
    assert not any("ntk_align" in ln for ln in db.build), "the default goal does not build a pending library"
    both = _make_lines("all", "pending")
    compile_, = [ln for ln in both if f" -c -o {obj} " in ln]
    link, = [ln for ln in both if f" -o {so} " in ln]
    assert compile_ == f"{_CC} -I../../include -c -o {obj} ntk_align.hip" and link == f"{_LD}{so} {obj} -L.. {_TAIL}"
    assert set(db.build) <= set(both), "the goal `pending` adds to what the default goal builds and changes none of its lines"
    removed, = [ln.split() for ln in db.clean if ln.startswith("rm -f")]
    assert obj in removed and so in removed


def test_the_pending_lists_name_this_library():
    """csrc/Makefile PENDING_LIBS, __graft_entry__.py PENDING_BINDINGS and PENDING_EXAMPLES and the files of the row: membership, not
    equality, so that the lists stay open."""
    import __graft_entry__ as G
    names = _pending_names()
    assert ROW.name in names and len(set(names)) == len(names)
    assert ROW.binding in G.PENDING_BINDINGS and ROW.example in G.PENDING_EXAMPLES and ROW.name in G.PENDING_EXAMPLES[ROW.example]
    earlier = set(_other_libraries()) - {""}
    assert ROW.name not in earlier and ROW.name not in L.BY_NAME
    assert set(G.PENDING_EXAMPLES[ROW.example]) - {ROW.name} <= earlier and G.PENDING_EXAMPLES[ROW.example][0] == ROW.name
    assert ROW.binding not in G.BINDINGS + G.MORE_BINDINGS + G.LATER_BINDINGS + G.STAGED_BINDINGS
    assert not any(ROW.example in d for d in (G.EXAMPLES, G.MORE_EXAMPLES, G.LATER_EXAMPLES, G.STAGED_EXAMPLES, G.HOST_EXAMPLES))
    assert "examples/" + ROW.example in open(os.path.join(ROOT, ".gitignore")).read().split()
    for path in ROW.product_files():
        assert os.path.exists(path), path
    assert os.path.basename(HEADER) in os.listdir(os.path.join(PENDING_INCLUDE, "needletail_amd"))
    for d in (L.INCLUDE, STAGED_INCLUDE):
        assert not os.path.exists(os.path.join(d, "needletail_amd", ROW.name + ".h")), "a pending header is in no other include directory"
    assert not os.path.exists(os.path.join(L.INCLUDE, f"needletail_amd_{ROW.name}.h"))
    assert f'#include "{ROW.include}"' in open(os.path.join(ROOT, "examples", ROW.example + ".cpp")).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"-I" + os.path.join(ROOT, "include_pending")' in entry and "STAGED_BINDINGS + PENDING_BINDINGS" in entry and "**PENDING_EXAMPLES" in entry
    assert '"ARCH=gfx950", "all", "pending"]' in entry and entry.count('"pending"') == 1 and 'make + ["SCAN2_FLAGS="]' in entry, "both attempts make `all pending`"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "The pending lists" in design and "PENDING_LIBS" in design and "_smoke_alignments(nt, ctx, dev, L)" in entry
    assert "## 26." in design and "7n" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ChainAlignments" in open(os.path.join(ROOT, "README.md")).read() and "align_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "align", "README.md"))


# ---- the stream contract ----------------------------------------------------------------------------------------------------------------

_SYNC = "(synchronous)"
CONTRACT = [
    SC.Row("ntk_align_run_device", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_align_read", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_align_result_device", SC.ASYNC, HEADER, "host-side only: queues nothing and waits for nothing", "decl", "test_stream_order"),
    SC.Row("ntk_align_stats", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
    SC.Row("ntk_align_trim", SC.SYNC, HEADER, _SYNC, "decl", "test_stream_order"),
]
FACADE = {"run_device": "al.run(", "read": "al.read", "result_device": "al.device_arrays", "stats": "al.stats", "trim": "al.trim"}


def test_stream_contract_of_the_five_calls():
    text = open(HEADER).read()
    decl = {name: (params, near) for name, params, near in SC.declarations(text)}
    assert sorted(decl) == sorted(ROW.module.PREFIX + c for c in ROW.calls if c != "destroy")
    with_pointer = {name for name, (params, _) in decl.items() if SC.takes_device_pointer(params)}
    assert with_pointer == {"ntk_align_run_device", "ntk_align_result_device"}
    rows = {r.function: r for r in CONTRACT}
    assert len(rows) == len(CONTRACT) == 5 and with_pointer <= set(rows)
    assert set(rows) == set(decl) - {"ntk_align_create"}, "every call that queues work or waits for the stream has a row"
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
    assert "stay valid until the next run_device, trim or destroy" in SC.plain(decl["ntk_align_result_device"][1])
    assert "a call it refuses on a handle that held nothing - before any run, or behind a trim - frees them again" in head
    code = L.no_comments(open(HIP).read())
    assert "if (m->held || !m->d_ctr.p) return;" in code and re.search(r"if \(\(rc = verify\(m, a\)\)\) \{\s*drop_counters\(m\);\s*return rc;", code)
    for words in ("Extension beyond a chain's ends and soft clips", "z-drop", "a two-piece gap cost", "re-ranking chains by alignment score", "tools/lib_fuzz.py"):
        assert words in head, ("Not here", words)
    # the earlier inventories see no header of this library
    assert not any("align" in os.path.basename(h) for h in SC.shipped_headers())


# ---- the library's own --------------------------------------------------------------------------------------------------------------------

def test_refusals_that_need_no_device():
    from needletail_amd import aligning as AL
    lib = AL.lib()
    bogus = C.c_void_p(8)   # never touched: the refusal comes first
    h, n, m = C.c_void_p(), C.c_uint64(5), C.c_uint64(6)
    good = AL.Params(15, 2, 4, 4, 2, 64, 2048, 0)
    args = (bogus, 1, bogus, 1, bogus, 1, bogus, 1, bogus, bogus, bogus, bogus, bogus, bogus, 1, 1, 1, bogus, 1)
    assert lib.ntk_align_create(None, C.byref(h)) == 2 and lib.ntk_align_create(bogus, None) == 2 and not h.value
    assert lib.ntk_align_run_device(None, *args, C.byref(good)) == 2
    assert lib.ntk_align_read(None, None, None, None, None, 0, 0, C.byref(n), C.byref(m)) == 2 and (n.value, m.value) == (5, 6)
    assert lib.ntk_align_result_device(None, None, None, None, None, C.byref(n), C.byref(m)) == 2
    assert lib.ntk_align_stats(None, None) == 2 and lib.ntk_align_trim(None) == 2
    lib.ntk_align_destroy(None)
    # a handle's own refusals come before any device call, and the verification on the device before anything held is touched
    src = L.no_comments(open(HIP).read())
    arrays = re.search(r"int check_arrays\(.*?\n\}", src, re.S).group(0)
    assert "(n_chains >> 32) || (n_reads >> 32) || (n_refs >> 31) || (n_sel >> 32)" in arrays and "hip" not in arrays
    for name in ("d_ref_offsets", "d_seq_offsets", "d_c_offsets", "d_m_offsets"):
        assert f"(uintptr_t){name} & 7" in arrays, name
    for name in ("d_chain_rows", "d_members", "d_rpos", "d_qpos", "d_sel"):
        assert f"(uintptr_t){name} & 3" in arrays, name
    params = re.search(r"int check_params\(.*?\n\}", src, re.S).group(0)
    for term in ("p->k < 1 || p->k > ALN_BYTE_MAX", "p->a < 1 || p->a > ALN_BYTE_MAX", "p->b < 1 || p->b > ALN_BYTE_MAX", "p->q > ALN_BYTE_MAX",
                 "p->e < 1 || p->e > ALN_BYTE_MAX", "p->band_pad > ALN_SEG_MAX", "p->max_seg < 1 || p->max_seg > ALN_SEG_MAX",
                 "p->work_mib && (p->work_mib < ALN_WORK_MIB_MIN || p->work_mib > ALN_WORK_MIB_MAX)"):
        assert term in params, term
    assert "hip" not in params
    rule = open(RULE_HPP).read()
    assert "ALN_BYTE_MAX = 255;" in rule and "ALN_SEG_MAX = 4095;" in rule and "ALN_WORK_MIB_MIN = 16, ALN_WORK_MIB_MAX = 4096, ALN_WORK_MIB_DEFAULT = 256;" in rule
    assert "ALN_NEG = -(1 << 29);" in rule and "ALN_SPAN_MAX = (uint64_t)1 << 28;" in rule
    body = re.search(r"int ntk_align_run_device\(.*?\n\}", src, re.S).group(0)
    order = [body.index(s) for s in ("check_arrays(m, d_ref", "check_params(params)", "verify(m, a)", "m->held = true", "rc = align(m,")]
    assert order == sorted(order) and "hip" not in body
    verify = re.search(r"\nint verify\(.*?\n\}", src, re.S).group(0)
    assert re.findall(r"m->(\w+)\.ensure", verify) == ["d_ctr"] and "release" not in verify
    assert verify.index("ALN_BAD_ARG_FLAGS) return NTK_ERR_BAD_ARG") < verify.index("ALN_UNSUPPORTED_FLAGS) return NTK_ERR_UNSUPPORTED")
    kernel = re.search(r"void aln_verify_kernel\(.*?\n\}", src, re.S).group(0)
    assert not re.search(r"\ba\.(?:rows|scores|g_offsets|cigar|seg_\w+|dir\w*|runs|run_offsets)\b", kernel), "the verification writes the flag word alone"
    assert "ch.ref[" not in kernel and "ch.read[" not in kernel and "aln_code" not in kernel, "and reads no base"
    grow = re.search(r"\nint align\(.*?\n\}", src, re.S).group(0)
    assert grow.index("n_cigar = stage[kStageTotals + 3]") < grow.index("m->d_cigar.ensure("), "cigar grows once the total is read back"
    # no kernel holds inline assembly; the only stores are plain C++
    assert not re.search(r"\basm\b|__asm|__builtin_amdgcn_s_", src)


def test_allocation_arithmetic_is_the_headers_memory_statement():
    """The header's memory statement, term by term, against the `ensure` calls of the source and the model's arithmetic."""
    src, hdr = open(HIP).read(), SC.plain(SC.head_comment(open(HEADER).read()))
    ensures = re.findall(r"\b(d_\w+)\.ensure\((?:m->stream|st), (.+?), (grow_\w+)\)", src)
    assert ensures == [
        ("d_ctr", "kCtrWords", "grow_exact"),
        ("d_rows", "8 * n_sel", "grow_exact"), ("d_scores", "n_sel", "grow_exact"), ("d_g_offsets", "n_sel + 1", "grow_exact"),
        ("d_seg_offsets", "n_sel + 1", "grow_exact"),
        ("d_seg_entry", "n_seg", "grow_exact"), ("d_seg_cells", "n_seg + 1", "grow_exact"), ("d_dir_offsets", "n_seg + 1", "grow_exact"),
        ("d_seg_runs", "n_seg + 1", "grow_exact"), ("d_run_offsets", "n_seg + 1", "grow_exact"),
        ("d_runs", "n_runs", "grow_exact"), ("d_dir", "dir_bytes", "grow_exact"), ("d_dir", "most", "grow_exact"), ("d_cigar", "n_cigar", "grow_exact")]
    for decl in ("DeviceArray<uint32_t> d_rows;", "DeviceArray<int64_t> d_scores;", "DeviceArray<uint64_t> d_g_offsets;", "DeviceArray<uint32_t> d_cigar;",
                 "DeviceArray<uint64_t> d_seg_offsets;", "DeviceArray<uint32_t> d_seg_entry;", "DeviceArray<uint64_t> d_seg_cells, d_dir_offsets;",
                 "DeviceArray<uint32_t> d_seg_runs;", "DeviceArray<uint64_t> d_run_offsets;", "DeviceArray<uint8_t> d_dir;", "DeviceArray<uint32_t> d_runs;",
                 "DeviceArray<uint64_t> d_ctr;", "DeviceArray<char> d_tmp;", "kCtrWords = 7;"):
        assert decl in src, decl
    assert M.CTR_WORDS == 7 and "7 counter words" in hdr
    assert "32 + 8 + 8 B per selected chain and 8 more (the rows, scores and g_offsets)" in hdr and "4 B per CIGAR word" in hdr
    assert "8 B per selected chain and 8 more (its first segment)" in hdr and M.device_bytes(1) - M.device_bytes(0) == 48 + 8
    assert "32 B per segment of a selected chain and 28 more" in hdr and M.device_bytes(0, n_seg=1) - M.device_bytes(0) == 32
    assert "4 B per run bound, n + m per DP segment (the run lists)" in hdr and M.device_bytes(0, n_runs=1) - M.device_bytes(0) == 4
    assert "the direction bytes of the largest group" in hdr and M.device_bytes(0, dir_bytes=1) - M.device_bytes(0) == 1
    assert M.device_bytes(0, n_cigar=1) - M.device_bytes(0) == 4 and M.device_bytes(0) == 8 * 7 + 8 + 8 + 28
    assert "Every array grows to exactly the largest size needed so far" in hdr and "all of it freed by trim" in hdr
    assert "at most 4095 * 4095 < 16 MiB" in hdr and 4095 * 4095 < 16 << 20
    # rocPRIM's temporary storage is held inside a call only, so device_bytes between calls has no term of unknown size
    assert "is held INSIDE a run_device only and freed before the call returns" in hdr
    code = L.no_comments(src)
    body = re.search(r"int ntk_align_run_device\(.*?\n\}", code, re.S).group(0)
    after = body[body.index("rc = align(m,"):]
    assert 0 < after.index("drop_tmp(m);") < after.index("if (rc") and "return" not in after[: after.index("drop_tmp(m);")]
    assert len(re.findall(r"\bdrop_tmp\(m\)", code)) == 1 and "m->d_tmp.release();" in re.search(r"void drop_tmp\(.*?\n\}", code, re.S).group(0)
    # the only arrays of the handle are those above; device_bytes names every one, and trim frees them all
    struct = re.search(r"struct ntk_align : Consumer \{(.*?)\n\};", src, re.S).group(1)
    arrays = set(re.findall(r"\b(d_[a-z_]+)[;,]", struct.split("uint64_t device_bytes")[0]))
    assert arrays == {"d_rows", "d_scores", "d_g_offsets", "d_cigar", "d_seg_offsets", "d_seg_entry", "d_seg_cells", "d_dir_offsets", "d_seg_runs",
                      "d_run_offsets", "d_dir", "d_runs", "d_ctr", "d_tmp"}
    count = re.search(r"uint64_t device_bytes\(\) const\s*\{(.*?)\n    \}", src, re.S).group(1)
    freed = re.search(r"void release_all\(\)\s*\{(.*?)\n    \}", src, re.S).group(1)
    for a in arrays:
        assert len(re.findall(rf"\b{a}\.bytes\(\)", count)) == 1 and len(re.findall(rf"\b{a}\.release\(\)", freed)) == 1, a
    assert "out->device_bytes = m->device_bytes();" in src
    assert "release_all()" in re.search(r"int ntk_align_trim\(.*?\n\}", src, re.S).group(0)
    gpu = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    assert 'al.stats()["device_bytes"] == M.device_bytes(**big)' in gpu and "n_cu() * M.BLOCKS_PER_CU * (M.THREADS // 64)" in gpu
