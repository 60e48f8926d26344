"""CPU-side checks of the coloured k-mer index (include/needletail_amd_colors.h, libneedletail_amd_colors.so).

The library is stated beside the ten rows of tests/_libraries.py, not among them (csrc/Makefile MORE_LIBS, __graft_entry__.py
MORE_BINDINGS / MORE_EXAMPLES): its row is made here, put through the five check_* functions every row is held to, and the four checks
tests/test_consumer_abi.py parametrises over the ten are restated for it.  Then what is the library's own: the struct fields of the
header, the binding and the model, the refusals that need no device, the header's memory statement against the `ensure` calls, and the
threshold the GPU tests aim at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _builds as B
import _colors_model as KM
import _libraries as L

ROOT = L.ROOT
HEADER = os.path.join(L.INCLUDE, "needletail_amd_colors.h")
HIP, RULE_HPP = (os.path.join(L.CSRC, f) for f in ("ntk_colors.hip", "ntk_colors_rule.hpp"))
GPU_TESTS = "test_gpu_colors.py"

ROW = L.Library(
    "colors", binding="coloring", cls="KmerColors",
    calls=("create", "destroy", "reset", "add_device", "stats", "lookup_device", "run_device", "release"),
    headers=("ntk_colors_rule.hpp",), example="screen_reads", bench="colors_bench", gpu_tests=GPU_TESTS, kernels={
        "kc_add_kernel": "test_index_edges_through_lookup",
        "kc_lookup_kernel": "test_index_edges_through_lookup",
        "kc_census_kernel": "test_index_edges_through_lookup",
        "kc_wave_kernel": "test_random_records_match_the_model",
        "kc_best_kernel": "test_best_and_second",
        "kc_long_kernel": "test_long_records_on_both_sides_of_the_threshold",
    }, leak=r"(?:^|::)kc_",
    c_main="struct ntk_kmer_colors_row r; struct ntk_kmer_colors_stats s; r.best = NTK_COLORS_NONE; s.n_colors = NTK_COLORS_MAX; "
    "return sizeof r == 40 && sizeof s == 576 && r.best == 0xFFFFFFFFFFFFFFFFull && s.n_colors == 64 ? 0 : 1;",
    no_device=lambda nt: nt.KmerColors(21, nt.PATH_BITS_CANONICAL, 3, 1000), prim=None, shape=r"::kc_[a-z_]+_kernel\(", n_global=6)


# ---- the five checks of tests/_libraries.py -------------------------------------------------------------------------------------------

def test_every_declared_function_is_exported_and_listed():
    L.check_exports(ROW)


def test_header_compiles_as_c_and_states_the_struct_sizes(tmp_path):
    L.check_header(ROW, tmp_path)


def test_every_kernel_names_the_test_that_launches_it():
    L.check_kernels(ROW)


def test_product_files_never_name_the_checker():
    L.check_product_files_never_name_the_checker(ROW)


def test_no_device_is_a_loud_error():
    L.check_no_device(ROW)


# ---- the four checks tests/test_consumer_abi.py parametrises over the rows, for this one ---------------------------------------------------

def test_library_links_exactly_what_it_needs_by_rpath():
    out = subprocess.run(["readelf", "-d", L.built(ROW.so)], capture_output=True, text=True).stdout
    needed = [n for n in re.findall(r"NEEDED.*\[(.*?)\]", out) if n.startswith("libneedletail_amd")]
    assert "$ORIGIN" in out
    assert needed == [os.path.basename(L.so_path(n)) for n in ROW.links + ("",)], needed


def test_no_kernel_leaks_into_or_out_of_the_library():
    """No kc_ kernel in any of the eleven other shared objects, and none of theirs in this one."""
    own = B.library_kernels(L.built(ROW.so))
    assert own and all(re.search(ROW.leak, n) for n in own), "the pattern no longer names the library's own kernels"
    core = B.library_kernels(L.built(L.so_path("")))
    assert not own & core
    others = [""] + [r.name for r in L.LIBRARIES]
    assert len(others) == 11
    for other in others:
        theirs = B.library_kernels(L.built(L.so_path(other)))
        assert not {n for n in theirs if re.search(ROW.leak, n)}, other or "core"
        if other:
            assert not {n for n in own if re.search(L.BY_NAME[other].leak, n)}, other
    names = " ".join(re.findall(r"\b(?:struct|void)\s+(\w+)", L.no_comments(open(HIP).read() + open(RULE_HPP).read())))
    assert not re.search(r"abundance|sketch|minhash|read_trim", names), "a name another library's leak pattern would match"


def test_the_shared_pieces_are_used_and_not_defined_again():
    """The scaffold comes from ntk_consumer.hpp and memory from ntk_device_mem.hpp; neither new file defines a piece of them again or
    names an allocation call, comments included.  Beyond that: the count libraries' header is left alone, plain HIP C++, no floating
    point."""
    from test_consumer_abi import MEM_DEFS, SHARED
    src, rule = open(HIP).read(), open(RULE_HPP).read()
    assert '#include "ntk_consumer.hpp"' in src and '#include "ntk_colors_rule.hpp"' in src
    assert "ntk_count_common.hpp" not in src + rule and "needletail_amd_count.h" not in src + rule
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
    for name in ("wave_sum", "add_agent", "grid_for", "record_span", "uniform", "for_each_chunk", "check_batch_params", "check_batch_pointers"):
        assert re.search(rf"\b{name}\(", code), name
    assert "MaterialiseScratch scratch;" in src and "struct ntk_kmer_colors : Consumer {" in src
    assert not re.search(r"#include\s+[<\"]hip", rule), "the rule header compiles without HIP"


def test_build_rule_is_the_rows():
    db = L.make_database()
    obj, so = "ntk_colors.o", "../libneedletail_amd_colors.so"
    assert db.prerequisites[obj] == {"ntk_colors.hip", "ntk_colors_rule.hpp", *L.CONSUMER_HPP, L.public_header("colors"), L.public_header("")}
    assert db.prerequisites[so] == {obj, "../libneedletail_amd.so"}
    assert so in db.prerequisites["all"]
    compile_, = [ln for ln in db.build if f" -c -o {obj} " in ln]
    link, = [ln for ln in db.build if f" -o {so} " in ln]
    assert compile_.endswith(" ntk_colors.hip") and "--offload-arch=gfx950" in compile_
    assert re.findall(r"-l(\S+)", link) == ["needletail_amd"] and f" {obj} " in link
    # the same command lines as a library of the ten, name for name
    as_dbg = lambda ln: ln.replace("colors", "dbg")   # noqa: E731
    assert as_dbg(compile_) in db.build and as_dbg(link) in db.build
    removed, = [ln.split() for ln in db.clean if ln.startswith("rm -f")]
    assert obj in removed and so in removed


def test_the_second_lists_name_the_same_one_library():
    """csrc/Makefile MORE_LIBS, __graft_entry__.py MORE_BINDINGS and MORE_EXAMPLES, and this file's row; the ten stay the ten."""
    import __graft_entry__ as G
    db = L.make_database()
    assert db.variables["MORE_LIBS"].split() == [ROW.name]
    assert ROW.name not in db.variables["CONSUMERS"].split() and len(db.variables["CONSUMERS"].split()) == 10
    assert tuple(G.MORE_BINDINGS) == (ROW.binding,) and ROW.binding not in G.BINDINGS
    assert list(G.MORE_EXAMPLES) == [ROW.example] and ROW.name in G.MORE_EXAMPLES[ROW.example] and ROW.example not in G.EXAMPLES
    assert set(G.MORE_EXAMPLES[ROW.example]) - {ROW.name} <= {r.name for r in L.LIBRARIES}
    assert ROW.name not in L.BY_NAME
    assert "examples/" + ROW.example in open(os.path.join(ROOT, ".gitignore")).read().split()
    for path in ROW.product_files():
        assert os.path.exists(path), path


# ---- the library's own ------------------------------------------------------------------------------------------------------------------

def _struct_fields(struct):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct %s \{(.*?)\};" % struct, hdr, re.S).group(1)
    return [re.sub(r"\[.*", "", f.strip()) for decl in re.findall(r"uint(?:64|32)_t ([^;]+);", body) for f in decl.split(",")]


def test_struct_fields_are_the_binding_and_the_model():
    from needletail_amd import coloring as K
    assert _struct_fields("ntk_kmer_colors_row") == list(K.COLUMNS) == list(KM.COLUMNS)
    assert _struct_fields("ntk_kmer_colors_stats") == [n for n, _ in K.Stats._fields_] == list(KM.STATS)
    assert C.sizeof(K.Stats) == 576 and len(K.COLUMNS) * 8 == 40   # the header's, which its C program states
    assert (K.COLORS_MAX, K.NONE) == (KM.COLORS_MAX, KM.NONE) == (64, 2 ** 64 - 1)
    rule = open(RULE_HPP).read()
    assert "KC_COLORS_MAX = 64;" in rule and "KC_PROBE_MAX = 4096;" in rule and "KC_EMPTY = ~(uint64_t)0;" in rule


def test_refusals_that_need_no_device():
    import needletail_amd as nt
    from needletail_amd import coloring as K
    lib = K.lib()
    bogus = C.c_void_p(8)   # never touched: the refusal comes first
    for k in (0, 33, 64):
        h = C.c_void_p()
        assert lib.ntk_kmer_colors_create(bogus, k, 0, 3, 100, C.byref(h)) == 1 and not h.value, k
    for k, path, n_colors, capacity in ((21, 0, 0, 100), (21, 0, 65, 100), (21, 3, 3, 100), (21, 0, 3, 0), (21, 0, 3, (3 << 38) + 1)):
        h = C.c_void_p()
        assert lib.ntk_kmer_colors_create(bogus, k, path, n_colors, capacity, C.byref(h)) == 2 and not h.value
    h = C.c_void_p()
    assert lib.ntk_kmer_colors_create(None, 21, 0, 3, 100, C.byref(h)) == 2 and lib.ntk_kmer_colors_create(bogus, 21, 0, 3, 100, None) == 2
    assert lib.ntk_kmer_colors_reset(None) == 2 and lib.ntk_kmer_colors_release(None) == 2 and lib.ntk_kmer_colors_stats(None, None) == 2
    assert lib.ntk_kmer_colors_add_device(None, None, None, 1, 0) == 2 and lib.ntk_kmer_colors_lookup_device(None, None, 0, None) == 2
    p = nt._lib.Params(21, 0, 2, 0)
    assert lib.ntk_kmer_colors_run_device(None, None, None, 0, None, 0, C.byref(p), None, None, None) == 2
    lib.ntk_kmer_colors_destroy(None)
    ctx = object()   # never used
    wide = nt.KmerSet(None, None, 0, 40, nt.PATH_BYTES_CANONICAL, ctx)
    narrow = nt.KmerSet(None, None, 0, 21, nt.PATH_BYTES_CANONICAL, ctx)
    with pytest.raises(nt.NtkError) as e:
        nt.KmerColors.from_sets([narrow, wide])
    assert e.value.status == 1
    with pytest.raises(nt.NtkError) as e:
        nt.KmerColors.from_sets([narrow, nt.KmerSet(None, None, 0, 21, nt.PATH_BITS, ctx)])
    assert e.value.status == 2
    with pytest.raises(TypeError):
        nt.KmerColors.from_sets([])
    kc = object.__new__(nt.KmerColors)   # no device: add refuses on the argument alone
    kc.k, kc.path, kc.n_colors, kc._h = 21, nt.PATH_BYTES_CANONICAL, 3, None
    for source, status in ((wide, 1), (nt.KmerSet(None, None, 0, 20, nt.PATH_BYTES_CANONICAL, ctx), 2),
                           (nt.KmerSet(None, None, 0, 21, nt.PATH_BITS, ctx), 2)):
        with pytest.raises(nt.NtkError) as e:
            kc.add(source, 0)
        assert e.value.status == status
    for color in (-1, 3):
        with pytest.raises(nt.NtkError) as e:
            kc.add(narrow, color)
        assert e.value.status == 2
    with pytest.raises(TypeError):
        kc.add([1, 2, 3], 0)


def test_classify_compares_in_integers():
    from needletail_amd import coloring as K
    none = KM.NONE
    rows = np.array([[130, 130, 100, 1, 0], [130, 3, 3, 2, none], [0, 0, 0, none, none], [3, 1, 1, 0, none], [2 ** 62, 2 ** 61, 0, 1, 0]],
                    dtype=np.uint64)
    hits = np.array([[30, 100, 0], [0, 0, 3], [0, 0, 0], [1, 0, 0], [2 ** 60, 2 ** 61, 0]], dtype=np.uint64)
    for min_hits, frac in ((1, (0, 1)), (4, (0, 1)), (1, (1, 3)), (1, (1, 2)), (1, (10, 13)), (1, (101, 130)), (2, (1, 1000))):
        want = KM.classify(rows, hits, min_hits, *frac)
        assert np.array_equal(K.classify(rows, hits, min_hits, frac), want), (min_hits, frac)
    assert K.classify(rows, hits).tolist() == [1, 2, -1, 0, 1]
    assert K.classify(rows, hits, 1, (1, 3)).tolist() == [1, -1, -1, 0, 1]   # 1 of 3 is a third exactly
    assert K.classify(rows, hits, 1, (1, 2)).tolist() == [1, -1, -1, -1, 1]   # 2^61 of 2^62 is a half exactly: no rounding
    assert K.classify(rows.view(np.int64), hits.view(np.int64), 1, 0.5).tolist() == [1, -1, -1, -1, 1]


def test_model_on_hand_made_masks():
    ix = KM.Index(3)
    ix.add([5, 6, 7, 5], [1, 2, 4, 4])
    ix.add([8, 9], 7)
    ix.add([10, 11], [0, 8])
    assert ix.masks == {5: 5, 6: 2, 7: 4, 8: 7, 9: 7} and ix.n_masked_bits == 1 and ix.per_color() == [3, 3, 4]
    row, hits, single = KM.screen_masks(ix.lookup([5, 6, 7, 7, 8, 99]), 3)
    assert row.tolist() == [6, 5, 3, 2, 0] and hits.tolist() == [2, 2, 4] and single.tolist() == [0, 1, 2]
    assert KM.best_second([0, 0, 0]) == (KM.NONE, KM.NONE) and KM.best_second([2, 0, 2]) == (0, 2) and KM.best_second([0, 9, 0]) == (1, KM.NONE)
    assert KM.screen_masks([], 2)[0].tolist() == [0, 0, 0, KM.NONE, KM.NONE]


def test_allocation_arithmetic_is_the_headers_memory_statement():
    """The header's memory statement, term by term, against the `ensure` calls of the source: the index, the statistics, one chunk of
    the materialise face, and the list of long records.  Nothing else is allocated, so nothing is proportional to the batch's bases."""
    src, hdr = open(HIP).read(), open(HEADER).read()
    ensures = re.findall(r"(\w+)\.ensure\(h->stream, ([^,]+), grow_exact\)", src)
    assert ensures == [("d_keys", "h->slots"), ("d_masks", "h->slots"), ("d_stats", "kStAll"), ("d_long", "n_bytes / kLongRecord + 2")]
    assert "DeviceArray<uint64_t> d_keys, d_masks;" in src and "DeviceArray<uint64_t> d_stats;" in src and "DeviceArray<uint64_t> d_long;" in src
    assert "16 B per slot" in hdr and "68 words of statistics" in hdr and "kStAll = kStWords + (int)KC_COLORS_MAX" in src and "kStWords = 4" in src
    long_record = int(re.search(r"kLongRecord = (\d+);", src).group(1))
    assert f"8 B per {long_record // 1000} {long_record % 1000:03d} bases of the batch, plus 16 B" in hdr
    assert "8.25 B per base of at most 64 MiB of bases plus a halo of at most 32 bases" in hdr
    assert "No array is proportional to the bases of the batch" in hdr
    # the scratch is the scaffold's, grown by for_each_chunk; the only arrays of the handle are those above
    arrays = set(re.findall(r"\b(d_[a-z_]+)[;,]", re.search(r"struct ntk_kmer_colors : Consumer \{(.*?)\n\};", src, re.S).group(1)))
    assert arrays == {"d_keys", "d_masks", "d_stats", "d_long"}
    count = re.search(r"uint64_t device_bytes\(\) const\s*\{(.*?)\n    \}", src, re.S).group(1)
    for a in arrays | {"scratch"}:
        assert a in count, a
    assert re.search(r"void release_scratch\(\) \{ scratch\.release\(\); d_long\.release\(\); \}", src)
    assert "for_each_chunk(*h, h->scratch, d_seq, d_qual, n_bytes, p," in src and src.count("for_each_chunk(") == 1


def test_threshold_constants_are_the_gpu_tests():
    src = open(HIP).read()
    assert int(re.search(r"kLongRecord = (\d+);", src).group(1)) == KM.LONG_RECORD
    gpu = open(os.path.join(ROOT, "tests", GPU_TESTS)).read()
    assert "LONG_RECORD = KM.LONG_RECORD" in gpu
    assert not re.search(r"kChunkBases\s*=", src), "the chunk length is ntk_chunks.hpp's alone"
    # the model's restatement of the header's memory statement, which the GPU test holds stats.device_bytes to
    assert KM.device_bytes(2, 0, 21) == 32 + 544 and KM.device_bytes(2, 160, 21) == 32 + 544 + 160 * 8 + 40 + 16
